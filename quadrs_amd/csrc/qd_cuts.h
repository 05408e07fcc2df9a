// qd_cuts.h — the cut list (include/quadrs_hip.h, "cut list"): many (shift, lowpass, decimate, range) cuts of one stream in one launch.
//
// The geometry and the LDS layout are stated in qd_cuts_plan.h, which also holds everything of the call that needs no HIP.  Two kernels:
//   k_cuts_tables  the NCO tables of a launch.  For every tile of a shifted cut the RowBase entries of the absolute rows of 512 samples
//                  the tile's reads touch (kCutsTileRows slots per tile; a table per CUT would be 2^32 entries for the longest admissible
//                  cut, and consecutive tiles share a boundary row at most), and once per call a lane table of 512 entries per distinct
//                  shift: all through nco_table_entry, with qd_shift's operands, so the multipliers are qd_shift's bit for bit.
//   k_cuts<FMT>    one workgroup per tile.  Phase 1 loads the tile's source samples through the format loaders of qd_device.h - 16-byte
//                  loads over the 16-byte aligned middle of the span, a per-sample path over its ragged head and tail, since a cut starts
//                  at any sample -, multiplies by nco_mul<...> where the cut has a shift and writes the LDS tile.  Phase 2: one lane per
//                  output, ascending taps, the block's truncation by jmax, one 8-byte store per output.
// The job table (one entry per cut), the taps table (identical (lowpass_hz, taps) pairs designed once) and the tile table are plain
// device memory written with ordinary copies.
#pragma once

#include "qd_cuts_plan.h"

#if defined(__HIPCC__)
#include "qd_device.h"

namespace qd {

constexpr uint32_t kCutShift = 1, kCutSecondOrder = 2;

struct __attribute__((aligned(16))) CutJob {
    double ratio;                    // qd_shift_ratio(shift_hz, sample_rate)
    uint64_t span0, valid;           // first D and count D + T: the cut's source span [span0, span0 + valid)
    uint64_t taps_at, lane_at;       // elements into the taps table and the lane table
    uint32_t D, T, flags, _pad;
};

// the source samples a tile reads, relative to its cut's span: [*lo, *hi)
__device__ __forceinline__ void cut_tile_reads(const CutJob &jb, const CutTile &tl, uint64_t *lo, uint64_t *hi) {
    const uint64_t ctr = jb.T - jb.T / 2;
    *lo = (uint64_t)tl.first * jb.D + ctr;
    const uint64_t end = (uint64_t)(tl.first + tl.count - 1) * jb.D + ctr + jb.T;
    *hi = end < jb.valid ? end : jb.valid;
}

__global__ __launch_bounds__(256) void k_cuts_tables(const CutJob *__restrict__ jobs, const CutTile *__restrict__ tiles, uint32_t n_tiles, RowBase *__restrict__ rowtab,
                                                    const double *__restrict__ lane_ratio, uint32_t n_lane, LaneEntry *__restrict__ lanetab) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_row = (uint64_t)n_tiles * kCutsTileRows;
    if (i < n_row) {
        const uint32_t t = (uint32_t)(i / kCutsTileRows), r = (uint32_t)(i % kCutsTileRows);
        const CutTile tl = tiles[t];
        const CutJob jb = jobs[tl.job];
        if (!(jb.flags & kCutShift)) return;
        uint64_t lo, hi;
        cut_tile_reads(jb, tl, &lo, &hi);
        const uint64_t row = (jb.span0 + lo) / kCutsNcoRow + r;
        if (row * kCutsNcoRow >= jb.span0 + hi) return;
        rowtab[i] = nco_row_entry((double)(row * kCutsNcoRow), jb.ratio);
    } else if (i - n_row < (uint64_t)n_lane * kCutsNcoRow) {
        const uint64_t u = (i - n_row) / kCutsNcoRow, j = (i - n_row) % kCutsNcoRow;
        lanetab[u * kCutsNcoRow + j] = nco_lane_entry((double)j, lane_ratio[u]);
    }
}

template <int FMT> constexpr int cuts_bps() { return FMT == QD_FMT_CF32 ? 8 : (FMT == QD_FMT_CS16 ? 4 : 2); }

// FileFormat::to_cf32 of one sample at p (src/lib.rs:231-255)
template <int FMT>
__device__ __forceinline__ float2 cuts_load(const uint8_t *p) {
    if constexpr (FMT == QD_FMT_CF32) {
        return *reinterpret_cast<const float2 *>(p);
    } else if constexpr (FMT == QD_FMT_CS16) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
        return make_float2(unpack_cs16(w & 0xffffu), unpack_cs16(w >> 16));
    } else {
        const uint32_t w = *reinterpret_cast<const uint16_t *>(p);
        return FMT == QD_FMT_CS8 ? make_float2(unpack_cs8(w & 0xffu), unpack_cs8(w >> 8)) : make_float2(unpack_cu8(w & 0xffu), unpack_cu8(w >> 8));
    }
}

// ... of the 16 / bps samples of one 16-byte aligned load
template <int FMT>
__device__ __forceinline__ void cuts_load_vec(const uint8_t *p, float2 *s) {
    const uint4 q = *reinterpret_cast<const uint4 *>(p);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    if constexpr (FMT == QD_FMT_CF32) {
        s[0] = make_float2(__builtin_bit_cast(float, w[0]), __builtin_bit_cast(float, w[1]));
        s[1] = make_float2(__builtin_bit_cast(float, w[2]), __builtin_bit_cast(float, w[3]));
    } else if constexpr (FMT == QD_FMT_CS16) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] = make_float2(unpack_cs16(w[u] & 0xffffu), unpack_cs16(w[u] >> 16));
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t h = (w[u >> 1] >> (16 * (u & 1))) & 0xffffu;
            s[u] = FMT == QD_FMT_CS8 ? make_float2(unpack_cs8(h & 0xffu), unpack_cs8(h >> 8)) : make_float2(unpack_cu8(h & 0xffu), unpack_cu8(h >> 8));
        }
    }
}

template <int FMT>
__global__ __launch_bounds__(kCutsThreads) void k_cuts(const uint8_t *__restrict__ src, const CutJob *__restrict__ jobs, const CutTile *__restrict__ tiles,
                                                       const float *__restrict__ taps, const RowBase *__restrict__ rowtab,
                                                       const LaneEntry *__restrict__ lanetab, float2 *__restrict__ out) {
    extern __shared__ __attribute__((aligned(32))) char smem_cuts[];
    RowBase *rows = reinterpret_cast<RowBase *>(smem_cuts);                                  // kCutsTileRows entries
    float2 *xs = reinterpret_cast<float2 *>(smem_cuts + kCutsTileRows * sizeof(RowBase));    // kCutsLdsSamples elements
    constexpr int BPS = cuts_bps<FMT>(), SPV = 16 / BPS;
    const uint32_t tid = threadIdx.x;
    const CutTile tl = tiles[blockIdx.x];
    const CutJob jb = jobs[tl.job];
    uint64_t rel0, rel1;
    cut_tile_reads(jb, tl, &rel0, &rel1);
    uint32_t len = (uint32_t)(rel1 - rel0);
    if (len > kCutsTileSamples) len = kCutsTileSamples;           // never: cuts_tile_outputs keeps a tile's reads inside the LDS tile
    const uint64_t abs0 = jb.span0 + rel0, row0 = abs0 / kCutsNcoRow;
    const bool shift = (jb.flags & kCutShift) != 0, second = (jb.flags & kCutSecondOrder) != 0;
    if (shift && tid < kCutsTileRows) rows[tid] = rowtab[(uint64_t)blockIdx.x * kCutsTileRows + tid];
    __syncthreads();

    // phase 1: source -> [NCO] -> LDS
    auto put = [&](uint32_t k, float2 v) {
        if (shift) {
            const uint64_t n = abs0 + k;
            const uint32_t j = (uint32_t)(n % kCutsNcoRow);
            const RowBase rb = rows[(uint32_t)(n / kCutsNcoRow - row0)];
            const LaneRot lr = nco_lane_rot((double)j, lanetab[jb.lane_at + j]);
            const float2 m = second ? nco_mul<true>(rb, lr, jb.ratio) : nco_mul<false>(rb, lr, jb.ratio);
            v = cmul(v, m);
        }
        xs[cuts_lds_index(k)] = v;
    };
    const uint8_t *p0 = src + ((int64_t)abs0 + tl.src_off) * BPS;
    uint32_t head = (uint32_t)(((16u - (uint32_t)((uintptr_t)p0 & 15u)) & 15u) / BPS);      // samples ahead of the first 16-byte boundary
    if (head > len || ((uintptr_t)p0 & (BPS - 1))) head = len;                              // (a source that is not even sample-aligned: no wide loads)
    const uint32_t n_vec = (len - head) / SPV, tail = head + n_vec * SPV;
    for (uint32_t k = tid; k < head; k += kCutsThreads) put(k, cuts_load<FMT>(p0 + (size_t)k * BPS));
    for (uint32_t v = tid; v < n_vec; v += kCutsThreads) {
        float2 s[SPV];
        cuts_load_vec<FMT>(p0 + ((size_t)head + (size_t)v * SPV) * BPS, s);
#pragma unroll
        for (int u = 0; u < SPV; ++u) put(head + v * SPV + u, s[u]);
    }
    for (uint32_t k = tail + tid; k < len; k += kCutsThreads) put(k, cuts_load<FMT>(p0 + (size_t)k * BPS));
    __syncthreads();

    // phase 2: LowPass::read_at's kept outputs (src/filter.rs:68-83, complex_convolve :107-124), one per lane
    if (tid < tl.count) {
        const uint32_t T = jb.T;
        const uint64_t base = (uint64_t)(tl.first + tid) * jb.D + (T - T / 2);
        const uint64_t left = jb.valid - base;
        const uint32_t jmax = left < T ? (uint32_t)left : T;
        const uint32_t k0 = tid * jb.D;
        const float *__restrict__ h = taps + jb.taps_at;
        float ar = 0.f, ai = 0.f;
        for (uint32_t j = 0; j < jmax; ++j) {
            const float2 x = xs[cuts_lds_index(k0 + j)];
            const float hj = h[j];
            ar = ar + x.x * hj;
            ai = ai + x.y * hj;
        }
        out[tl.out_at + tid] = make_float2(ar, ai);
    }
}

}  // namespace qd
#endif  // __HIPCC__
