// qd_cascade.h — the fused CASCADE kernel:  unpack -> [NCO] -> FIR1/D1 -> [NCO] -> [FIR2/D2 -> [NCO]] -> FFT -> |X| -> epilogue
//
// Chains the one-stage description (qd_chain_desc) cannot hold: a shift after the filter (`lowpass ... shift ...`) and two
// cascaded lowpass stages (`lowpass -decimate 4 ... lowpass -decimate 8 ...`), at most one shift at each rate.  The reference
// nests its stages (src/lib.rs:83-175): per sink window the outer stage reads read_exact_at(w S, W), a LowPass(D, T) asked for
// (off, n) reads (off D, n D + T) from its inner stage and filters with ITS OWN per-call truncation (src/filter.rs:54-83), a
// Shift multiplies sample off + i by e^{i (off + i) ratio} at its own rate (src/shift.rs:48-52).
//
// One workgroup (256 threads) owns one window at a time and walks the windows of the launch grid-stride.  Per window:
//   1  the inter block: FIR1 outputs i = 0 .. n2 - 1 (n2 = W D2 + T2 with a second lowpass, else W) of the window's first
//      stage read, b2 = w S D2 the absolute index of output 0 at rate r / D1.  The source is streamed through LDS in
//      sub-tiles of M outputs ((M - 1) D1 + T1 samples: unpacked, NCO'd at the source rate on the absolute index); each lane
//      forms one output with jmax = min(T1, n1 - (i D1 + c1)), n1 = n2 D1 + T1 — the truncation of THIS window's inner read —
//      and the inter NCO (absolute index b2 + i) is applied as the output is parked;
//   2  FIR2 (jmax against n2) + its NCO on the absolute outer index w S + k, or the inter block itself without a second
//      lowpass, into the FFT buffer in rustfft's digit-reversed order;
//   3  one wave: Radix4 (wave_fft_epilogue_fn, qd_chain.h) and the norm / glyph / bucket epilogue.
// Every FIR product and sum is a separately rounded f32 operation in ascending-tap order (the reference's
// complex_convolve, src/filter.rs:107-124; -ffp-contract=off); the NCO multipliers are the exact-product table scheme of
// qd_device.h (second order), laid out on 512-sample rows of each stage's OWN absolute index (row bases from k_rowtab, one table
// per NCO over the launch's range): a window's bytes do not depend on the launch, slab, chunk or shard that computes it.
//
// The write sink (QD_EPI_CF32_BLOCKS, k_cascade_write): the sink's window is a read_at block of B outer outputs (src/lib.rs:178-213),
// whose inter block (B D2 + T2) is far larger than the LDS.  A kernel window is a SUB-BLOCK of K outputs [k0, k0 + K) of block b
// (ChainParams W = K, blk_len = B, blk_sub_mask = B / K - 1): FIR1 forms only the inter samples the sub-block's FIR2 reads,
// [k0 D2 + c2, (k0 + K - 1) D2 + c2 + T2) clipped to the block's n2, each still truncated against the BLOCK's n1; FIR2 truncates
// against the block's n2.  The outputs go straight to global memory (a lane per output, consecutive lanes consecutive float2).
// Without a second lowpass the sub-block's FIR1 outputs are the outputs and nothing is parked.  No FFT: the source sub-tile only.
//
// LDS (dynamic): inter block (n2 plus one pad per D2 when D2 is even: FIR2's lanes stride D2 + 1, odd; the pads are phased so that
// every output's first sample starts a pad period) | source sub-tile (one pad per D1 when D1 is even; the FFT buffer and the bucket
// sums reuse it once FIR1 is done).  An untruncated output's FIR walks its taps in blocks of 8 with
// the pad offsets of the block known per tap (casc_fir_full); the truncated tail outputs take the per-tap form (casc_fir_any).
#pragma once

#include "qd_chain.h"

namespace qd {

constexpr uint32_t kCascadeRow = 512;          // NCO row of every stage: samples [r 512, (r + 1) 512) of that stage's index
constexpr uint32_t kCascadeThreads = 256;
constexpr uint32_t kCascS0 = 1, kCascS1 = 2, kCascL2 = 4, kCascS2 = 8;       // CascadeParams::flags

struct CascadeParams {
    ChainParams c;              // src / src_first / src_count, first_window / n_windows / out_window0 / out, FFT layout, epilogue
    const float *h1, *h2;       // taps of the two lowpass stages (global, read as scalar loads)
    const LaneEntry *jtab;      // 3 x 512 lane entries (qd_nco.h) of the exact products j * ratio_k, one block per NCO
    const RowBase *rows[3];     // row bases of each NCO (k_rowtab, 512-sample rows of its own stage's index) over the launch's range ...
    uint64_t row0[3];           // ... starting at this absolute row
    double ratio0, ratio1, ratio2;
    uint64_t S;                 // stride of the sink, outer samples
    uint32_t D1, T1, D2, T2;    // D2 = 1, T2 = 0 without a second lowpass
    uint32_t n2;                // inter samples per window
    uint32_t M;                 // FIR1 outputs per source sub-tile
    uint32_t inter_elems, src_elems;     // LDS float2 capacities (pads included)
    uint32_t dmagic1, dmagic2;  // floor(2^32 / D) + 1 of an even D (pad index m + (m + phi) / D), else 0: no pad
    uint32_t phi2;              // pad phase of the inter block: (c2 + phi2) % D2 == 0, so FIR2's first sample starts a pad period
    uint32_t flags;             // kCascS0 | kCascS1 | kCascL2 | kCascS2
};

__device__ __forceinline__ uint32_t casc_pad(uint32_t m, uint32_t dmagic, uint32_t phi = 0) { return dmagic ? m + __umulhi(m + phi, dmagic) : m; }

// FIR class of a decimation: how the pads fall inside a block of 8 taps whose first tap starts a pad period (offset j + j / D of tap j
// from the output's first sample): 0 no pad (odd D), 2 / 4 D == 2 / 4 (tap u of a block at u + u / D), 8 D a multiple of 8 (tap u at u),
// -1 any other even D (per-tap pad index)
__device__ __forceinline__ int casc_fir_class(uint32_t D) { return (D & 1) ? 0 : (D == 2 ? 2 : (D == 4 ? 4 : (D % 8 == 0 ? 8 : -1))); }

// One untruncated output: x[0 .. T) of its samples (x = the padded LDS address of the first one, a pad-period start), taps ascending in
// blocks of 8 (one scalar load of 8 taps, 8 LDS reads in flight), each tap a packed multiply then a packed add — two roundings per tap and
// component, the reference's order (src/filter.rs:111-121)
template <int DC>
__device__ __forceinline__ float2 casc_fir_full(const float2 *x, const_f32_p h, uint32_t T, uint32_t D) {
    v2f acc = {0.f, 0.f};
    uint32_t j = 0;
    for (; j + 8 <= T; j += 8) {
        const float2 *xp = x + (DC == 0 ? j : j + j / D);
        float2 xv[8];
        float hv[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) { xv[u] = xp[(DC == 2 || DC == 4) ? u + u / DC : u]; hv[u] = h[j + u]; }
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            const v2f xx = {xv[u].x, xv[u].y}, hh = {hv[u], hv[u]};
            acc = acc + xx * hh;
        }
    }
    for (; j < T; ++j) {
        const float2 xv = x[DC == 0 ? j : j + j / D];
        const v2f xx = {xv.x, xv.y}, hh = {h[j], h[j]};
        acc = acc + xx * hh;
    }
    return make_float2(acc.x, acc.y);
}

// the same sum for any output (truncated ones: jmax < T) and any D: per-tap pad index
__device__ __forceinline__ float2 casc_fir_any(const float2 *base, uint32_t q0, uint32_t jmax, const_f32_p h, uint32_t dmagic, uint32_t phi) {
    float ar = 0.f, ai = 0.f;
    for (uint32_t j = 0; j < jmax; ++j) {
        const float2 x = base[casc_pad(q0 + j, dmagic, phi)];
        const float hj = h[j];
        ar = ar + x.x * hj;
        ai = ai + x.y * hj;
    }
    return make_float2(ar, ai);
}

__device__ __forceinline__ float2 casc_fir(int cls, const float2 *base, uint32_t q0, uint32_t jmax, uint32_t T, uint32_t D, const_f32_p h,
                                           uint32_t dmagic, uint32_t phi) {
    if (jmax == T) {
        const float2 *x = base + casc_pad(q0, dmagic, phi);
        switch (cls) {
        case 0: return casc_fir_full<0>(x, h, T, D);
        case 2: return casc_fir_full<2>(x, h, T, D);
        case 4: return casc_fir_full<4>(x, h, T, D);
        case 8: return casc_fir_full<8>(x, h, T, D);
        default: break;
        }
    }
    return casc_fir_any(base, q0, jmax, h, dmagic, phi);
}

template <int FMT>
__device__ __forceinline__ float2 casc_load(const uint8_t *src, uint64_t i) {
    if constexpr (FMT == 0) return reinterpret_cast<const float2 *>(src)[i];
    else if constexpr (FMT == 1) { const uint16_t w = reinterpret_cast<const uint16_t *>(src)[i]; return make_float2(unpack_cs8(w & 0xff), unpack_cs8(w >> 8)); }
    else if constexpr (FMT == 2) { const uint16_t w = reinterpret_cast<const uint16_t *>(src)[i]; return make_float2(unpack_cu8(w & 0xff), unpack_cu8(w >> 8)); }
    else { const uint32_t w = reinterpret_cast<const uint32_t *>(src)[i]; return make_float2(unpack_cs16(w & 0xffffu), unpack_cs16(w >> 16)); }
}

// multiplier of absolute sample n of one NCO's stream (rb: its row table, whose first row is row0)
__device__ __forceinline__ float2 casc_nco(const RowBase *rb, uint64_t row0, uint64_t n, const LaneEntry *jt, double ratio) {
    const uint32_t j = (uint32_t)(n % kCascadeRow);
    return nco_mul<true>(rb[n / kCascadeRow - row0], nco_lane_rot((double)j, jt[j]), ratio);
}

template <int FMT>
__global__ __launch_bounds__(kCascadeThreads) void k_cascade(const CascadeParams P) {
    extern __shared__ __attribute__((aligned(16))) float2 casc_lds[];
    float2 *inter = casc_lds;
    float2 *tile = casc_lds + P.inter_elems;                                 // source sub-tile, then the FFT buffer
    const uint32_t tid = threadIdx.x;
    const ChainParams &C = P.c;
    const DynGeo geo(C);
    const uint32_t D1 = P.D1, T1 = P.T1, D2 = P.D2, T2 = P.T2, n2 = P.n2, W = C.W;
    const uint32_t c1 = T1 - T1 / 2, c2 = T2 - T2 / 2;
    const uint64_t n1 = (uint64_t)n2 * D1 + T1;
    const bool l2 = (P.flags & kCascL2) != 0;
    const_f32_p h1 = (const_f32_p)P.h1;
    const_f32_p h2 = (const_f32_p)P.h2;
    const uint32_t log_width = 2 * geo.layers;
    const int cls1 = casc_fir_class(D1), cls2 = casc_fir_class(D2);
    for (uint64_t w = C.first_window + blockIdx.x; w < C.first_window + C.n_windows; w += gridDim.x) {
        const uint64_t o = w * P.S;                                          // outer index of the window's first sample
        const uint64_t b2 = l2 ? o * D2 : o;                                 // inter index of inter[0]
        const uint64_t b1 = b2 * D1;                                         // source index of the window's first read
        // ---- 1: FIR1 over source sub-tiles
        for (uint32_t i0 = 0; i0 < n2; i0 += P.M) {
            const uint32_t m = n2 - i0 < P.M ? n2 - i0 : P.M;
            const uint64_t s0 = b1 + (uint64_t)i0 * D1 + c1;                 // first source sample any output of the sub-tile reads
            const uint64_t want = (uint64_t)(m - 1) * D1 + T1, left = n1 - ((uint64_t)i0 * D1 + c1);
            const uint32_t ns = (uint32_t)(want < left ? want : left);
            __syncthreads();                                                 // the previous sub-tile's readers are done
            for (uint32_t q = tid; q < ns; q += kCascadeThreads) {
                const uint64_t s = s0 + q;
                float2 x = make_float2(0.f, 0.f);
                if (s >= C.src_first && s < C.src_first + C.src_count) x = casc_load<FMT>(C.src, s - C.src_first);
                if (P.flags & kCascS0) x = cmul(x, casc_nco(P.rows[0], P.row0[0], s, P.jtab, P.ratio0));
                tile[casc_pad(q, P.dmagic1)] = x;
            }
            __syncthreads();
            for (uint32_t k = tid; k < m; k += kCascadeThreads) {
                const uint32_t i = i0 + k;
                const uint64_t lim = n1 - ((uint64_t)i * D1 + c1);
                const uint32_t jmax = lim < T1 ? (uint32_t)lim : T1;
                float2 v = casc_fir(cls1, tile, k * D1, jmax, T1, D1, h1, P.dmagic1, 0);
                if (P.flags & kCascS1) v = cmul(v, casc_nco(P.rows[1], P.row0[1], b2 + i, P.jtab + kCascadeRow, P.ratio1));
                inter[casc_pad(i, P.dmagic2, P.phi2)] = v;
            }
        }
        __syncthreads();
        // ---- 2: FIR2 (or the inter block itself) into the FFT buffer, digit-reversed
        float2 *fb = tile;
        for (uint32_t k = tid; k < W; k += kCascadeThreads) {
            float2 v;
            if (l2) {
                const uint32_t q0 = k * D2 + c2;
                const uint32_t lim = n2 - q0, jmax = lim < T2 ? lim : T2;
                v = casc_fir(cls2, inter, q0, jmax, T2, D2, h2, P.dmagic2, P.phi2);
                if (P.flags & kCascS2) v = cmul(v, casc_nco(P.rows[2], P.row0[2], o + k, P.jtab + 2 * kCascadeRow, P.ratio2));
            } else {
                v = inter[k];
            }
            if (C.window) { const float wv = C.window[k]; v.x = v.x * wv; v.y = v.y * wv; }   // the plan's window (qd_chain_desc.windowing): Complex<f32> * f32
            const uint32_t xx = k & ((1u << log_width) - 1), yy = k >> log_width;
            fb[yy + (rev4(xx, geo.layers) << geo.log_base)] = v;
        }
        __syncthreads();
        // ---- 3: transform + epilogue on wave 0
        if (tid < 64) {
            wave_fft_epilogue_fn<DynGeo, 0, 3>(C, geo, C.tw, fb, w, 1, tid);
            const uint64_t wrel = w - C.out_window0;
            if (C.epi == QD_EPI_BUCKET2_U8) {
                float *nb = reinterpret_cast<float *>(inter);               // the inter block is dead: norms in natural order
                for (uint32_t b = tid; b < W; b += 64) nb[b] = norm_ref(fb[b]);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (tid == 0) {                                               // src/fft.rs:95-97: two sequential half sums
                    float first = 0.f, second = 0.f;
                    for (uint32_t b = 0; b < W / 2; ++b) first = first + nb[b];
                    for (uint32_t b = W / 2; b < W; ++b) second = second + nb[b];
                    reinterpret_cast<uint8_t *>(C.out)[wrel] = first < second ? 0 : 1;
                }
            } else if (C.epi == QD_EPI_MARK_U8) {
                wave_mark_epilogue_fn<DynGeo>(C, geo, [&](uint32_t b) { return fb[b]; }, reinterpret_cast<uint8_t *>(C.out) + wrel, 1, tid);
            } else if (C.epi == QD_EPI_NORMS_F32) {
                float *outf = reinterpret_cast<float *>(C.out) + wrel * W;
                for (uint32_t b = tid; b < W; b += 64) outf[b] = norm_ref(fb[b ^ (W >> 1)]);
            } else {
                uint8_t *outb = reinterpret_cast<uint8_t *>(C.out) + wrel * W;
                for (uint32_t b = tid; b < W; b += 64) outb[b] = glyph_of<DynGeo>(C, norm_ref(fb[b ^ (W >> 1)]));
            }
        }
        __syncthreads();                                                     // the next window rewrites the row bases, tile and inter block
    }
}

// Write sink behind a cascade: kernel window w = sub-block (w & blk_sub_mask) of read_at block w / (blk_sub_mask + 1), K = W outputs
// each, written as cf32 to out + (w - out_window0) K.  The same arithmetic, truncation and NCO rows as k_cascade (see the top of the file).
template <int FMT>
__global__ __launch_bounds__(kCascadeThreads) void k_cascade_write(const CascadeParams P) {
    extern __shared__ __attribute__((aligned(16))) float2 casc_lds[];
    float2 *inter = casc_lds;                                                // the sub-block's inter samples (second lowpass only)
    float2 *tile = casc_lds + P.inter_elems;                                 // source sub-tile
    const uint32_t tid = threadIdx.x;
    const ChainParams &C = P.c;
    const uint32_t D1 = P.D1, T1 = P.T1, D2 = P.D2, T2 = P.T2, n2 = P.n2, K = C.W;
    const uint32_t c1 = T1 - T1 / 2, c2 = T2 - T2 / 2;
    const uint64_t n1 = (uint64_t)n2 * D1 + T1;
    const bool l2 = (P.flags & kCascL2) != 0;
    const uint32_t log_subs = (uint32_t)__popc(C.blk_sub_mask);            // B / K is a power of two
    const_f32_p h1 = (const_f32_p)P.h1;
    const_f32_p h2 = (const_f32_p)P.h2;
    const int cls1 = casc_fir_class(D1), cls2 = casc_fir_class(D2);
    float2 *out = reinterpret_cast<float2 *>(C.out);
    for (uint64_t w = C.first_window + blockIdx.x; w < C.first_window + C.n_windows; w += gridDim.x) {
        const uint32_t k0 = (uint32_t)(w & C.blk_sub_mask) * K;             // the sub-block's first output within its block
        const uint64_t o = (w >> log_subs) * C.blk_len;                     // outer index of the block's first output
        const uint64_t b2 = l2 ? o * D2 : o;                                 // inter index of the block's inter sample 0
        const uint64_t b1 = b2 * D1;                                         // source index of the block's first read
        const uint32_t i_lo = l2 ? k0 * D2 + c2 : k0;                        // inter samples [i_lo, i_hi) of the block
        const uint32_t i_end = l2 ? (k0 + K - 1) * D2 + c2 + T2 : k0 + K;
        const uint32_t i_hi = i_end < n2 ? i_end : n2;
        float2 *ow = out + (w - C.out_window0) * K;
        // ---- 1: FIR1 over source sub-tiles: inter samples i_lo .. i_hi - 1 (the outputs themselves without a second lowpass)
        for (uint32_t i0 = 0; i0 < i_hi - i_lo; i0 += P.M) {
            const uint32_t m = i_hi - i_lo - i0 < P.M ? i_hi - i_lo - i0 : P.M;
            const uint64_t is = (uint64_t)i_lo + i0;                         // block index of the sub-tile's first output
            const uint64_t s0 = b1 + is * D1 + c1;                           // first source sample any output of the sub-tile reads
            const uint64_t want = (uint64_t)(m - 1) * D1 + T1, left = n1 - (is * D1 + c1);
            const uint32_t ns = (uint32_t)(want < left ? want : left);
            __syncthreads();                                                 // the previous sub-tile's readers are done
            for (uint32_t q = tid; q < ns; q += kCascadeThreads) {
                const uint64_t s = s0 + q;
                float2 x = make_float2(0.f, 0.f);
                if (s >= C.src_first && s < C.src_first + C.src_count) x = casc_load<FMT>(C.src, s - C.src_first);
                if (P.flags & kCascS0) x = cmul(x, casc_nco(P.rows[0], P.row0[0], s, P.jtab, P.ratio0));
                tile[casc_pad(q, P.dmagic1)] = x;
            }
            __syncthreads();
            for (uint32_t k = tid; k < m; k += kCascadeThreads) {
                const uint64_t i = is + k;
                const uint64_t lim = n1 - (i * D1 + c1);
                const uint32_t jmax = lim < T1 ? (uint32_t)lim : T1;
                float2 v = casc_fir(cls1, tile, k * D1, jmax, T1, D1, h1, P.dmagic1, 0);
                if (P.flags & kCascS1) v = cmul(v, casc_nco(P.rows[1], P.row0[1], b2 + i, P.jtab + kCascadeRow, P.ratio1));
                if (l2) inter[casc_pad(i0 + k, P.dmagic2)] = v;            // output k of the sub-block starts at k D2: a pad period
                else ow[i0 + k] = v;
            }
        }
        if (!l2) continue;                                                   // the next window's first barrier orders the tile
        __syncthreads();
        // ---- 2: FIR2 (truncated against the block's n2) + its NCO on the absolute outer index, straight to global memory
        for (uint32_t k = tid; k < K; k += kCascadeThreads) {
            const uint32_t lim = n2 - ((k0 + k) * D2 + c2), jmax = lim < T2 ? lim : T2;
            float2 v = casc_fir(cls2, inter, k * D2, jmax, T2, D2, h2, P.dmagic2, 0);
            if (P.flags & kCascS2) v = cmul(v, casc_nco(P.rows[2], P.row0[2], o + k0 + k, P.jtab + 2 * kCascadeRow, P.ratio2));
            ow[k] = v;
        }
        // the next window writes the inter block only after the barriers of its first sub-tile, which every reader has passed
    }
}

}  // namespace qd
