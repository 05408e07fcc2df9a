// qd_bands.h — band traces of norms rows (qd_plan_bands): k_bands folds each window of a batch of the norms sink's
// windows ACROSS its bins, one result per window and band: the band's exact sum and mean (a qd_mean.h cell), its peak and the peak's bin.
// k_bands_pick names the loudest band of each window.  qd_bands_fold (quadrs_hip.hip) is the CPU twin and uses the same functions.
//
// Every word of a result is an integer sum or an integer max, so neither the lane-group width, nor the split of a band over lanes and
// waves, nor the order the lanes meet in changes a bit.  Windows are independent: there is no accumulator, no seam and no finish kernel.
//
// The first half of the header is the launch geometry as plain integer code: it compiles as C++17 on the host, where a program can walk
// every (workgroup, lane) of a launch (tests/test_bands_cpu.py), and under hipcc, where the kernel takes every index from it.
#ifndef QD_BANDS_H
#define QD_BANDS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define QD_BANDS_HD __host__ __device__
#else
#define QD_BANDS_HD
#endif

namespace qd {

constexpr uint32_t kBandsThreads = 256;
constexpr uint32_t kBandsMax = 255;              // QD_BANDS_MAX
constexpr uint32_t kBandNone = 0xffffffffu;      // QD_BAND_NONE
constexpr uint32_t kBandsReach = 16;             // bins a lane takes before the next wider lane group is chosen
constexpr uint64_t kBandsMaxWorkspace = 1ull << 30;

struct Band { uint32_t lo, hi; };                // qd_band: fftshifted bins [lo, hi)

// Geometry of a launch over one batch: windows [g0, g0 + nw) of the range (g0 counts from the range's first window), W f32 each, K
// bands.
//   item    one (window, band) pair, numbered i = window K + band within the batch, so neighbouring lane groups read the same window's
//           cache lines.  A group of L consecutive lanes (L a power of two, 1 ... 256) owns the item; nobody else touches its outputs.
//   lanes   lane t of the group reads the band's bins lo + t, lo + t + L, ...: consecutive lanes read consecutive words, whatever lo is.
//   width   one L a call, from its longest band: the smallest of 1, 4, 16, 64, 256 with kBandsReach L >= longest, else 256 (the band is
//           then walked in a loop as long as it needs).  A workgroup of 256 lanes holds 256 / L items; the items past the last are
//           masked.  L = 1 is a lane an item: bands of at most kBandsReach bins are rounded by every lane of a wave, not by one in
//           four (measured: DESIGN.md section 3.20).
struct BandsGeometry {
    uint64_t g0, nw, n_items;
    uint32_t W, K, L, log2_L, items_per_group;
};

QD_BANDS_HD inline uint32_t bands_lanes(uint32_t longest) {
    uint32_t L = 1;
    while (L < kBandsThreads && (uint64_t)kBandsReach * L < longest) L *= 4;
    return L;
}

inline void bands_split(uint64_t g0, uint64_t nw, uint32_t W, uint32_t K, uint32_t longest, BandsGeometry *G, uint64_t *grid) {
    G->g0 = g0; G->nw = nw; G->W = W; G->K = K;
    G->L = bands_lanes(longest);
    G->log2_L = 0;
    while ((1u << G->log2_L) < G->L) ++G->log2_L;
    G->items_per_group = kBandsThreads / G->L;
    G->n_items = nw * K;
    *grid = (G->n_items + G->items_per_group - 1) / G->items_per_group;
}

// What lane `tid` of workgroup `block` does: its item's window (within the batch) and band, its place `lane` in the item's lane group,
// and where the item's results go: index `out` of the range's [n, K] rows.  An inactive lane has no item: it reads and stores nothing.
struct BandsLane {
    bool active;
    uint32_t band, lane;
    uint64_t win, out;
};
QD_BANDS_HD inline BandsLane bands_lane(const BandsGeometry &G, uint32_t block, uint32_t tid) {
    BandsLane l;
    const uint64_t item = (uint64_t)block * G.items_per_group + (tid >> G.log2_L);
    l.lane = tid & (G.L - 1);
    l.active = item < G.n_items;
    l.win = 0; l.band = 0;
    if (l.active && (G.n_items >> 32) == 0) {                           // the common case without a 64-bit division
        const uint32_t i = (uint32_t)item;
        l.win = i / G.K; l.band = i % G.K;
    } else if (l.active) {
        l.win = item / G.K; l.band = (uint32_t)(item % G.K);
    }
    l.out = (G.g0 + l.win) * G.K + l.band;
    return l;
}
// the bins of the band [lo, hi) that the lane takes, in rising order: first, and the step to the next
QD_BANDS_HD inline uint32_t bands_first_bin(const BandsLane &l, uint32_t lo) { return lo + l.lane; }
QD_BANDS_HD inline uint32_t bands_step(const BandsGeometry &G) { return G.L; }

// The running peak of a band as one u64 that folds by integer max: the value's bits without the sign above the complement of its bin,
// so that the greatest value wins and among equals the lowest bin.  0 is "no value" (a bin is below 2^32 - 1); NaNs give no key.
QD_BANDS_HD inline uint64_t bands_key(uint32_t bits, uint32_t bin) {
    const uint32_t a = bits & 0x7fffffffu;
    return a > 0x7f800000u ? 0ull : ((uint64_t)a << 32) | (uint64_t)(0xffffffffu - bin);
}
QD_BANDS_HD inline uint32_t bands_key_peak(uint64_t key) { return (uint32_t)(key >> 32); }
QD_BANDS_HD inline uint32_t bands_key_bin(uint64_t key) { return key ? 0xffffffffu - (uint32_t)key : kBandNone; }

// The loudest band of a window from its K levels and counts: the lowest k with the greatest level among bands that hold a value, 255
// when none does.  Levels of such bands are non-negative or +inf, so they order as their bit patterns do: band k's key is its level's
// bits above the complement of k, 0 for a band without a value (k is below 255, so no band's key is 0), and the pick is the greatest.
QD_BANDS_HD inline uint64_t bands_pick_key(uint32_t level_bits, uint32_t count, uint32_t k) {
    return count ? ((uint64_t)level_bits << 32) | (uint64_t)(0xffffffffu - k) : 0ull;
}
QD_BANDS_HD inline uint8_t bands_pick_of(uint64_t key) { return key ? (uint8_t)(0xffffffffu - (uint32_t)key) : (uint8_t)255; }
QD_BANDS_HD inline uint8_t bands_pick(const uint32_t *level_bits, const uint32_t *count, uint32_t K) {
    uint64_t key = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t o = bands_pick_key(level_bits[k], count[k], k);
        key = o > key ? o : key;
    }
    return bands_pick_of(key);
}
// k_bands_pick's lane group: 2^lg lanes a window, the smallest power of two that holds K bands, a wave at most; lane t takes bands
// t, t + 2^lg, ..., so the lanes of a wave read consecutive words of the level and count rows
QD_BANDS_HD inline uint32_t bands_pick_log2_lanes(uint32_t K) {
    uint32_t lg = 0;
    while (lg < 6 && (1u << lg) < K) ++lg;
    return lg;
}

}  // namespace qd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "qd_mean.h"

namespace qd {

struct BandsParams {
    const float *norms;                          // the batch's windows, nw x W
    const Band *bands;                           // K bands, device memory
    BandsGeometry G;
    float *level; double *sum; uint32_t *count;  // n x K each, the whole range's; any may be nullptr
    float *peak; uint32_t *peak_bin;
};

// One item a lane group.  A lane adds its bins into its own ten words (mean_add) and keeps its running key, four loads in flight; the L
// lanes then meet: a butterfly of cross-lane shuffles inside a wave (every lane ends with the group's total; a word that is zero in the
// whole wave is skipped, which for norms leaves two or three limbs, the count and the key), and for L = 256 the four waves' totals
// through u64 LDS adds and one LDS max.  Lane 0 of the group rounds the cell once (mean_finish_cell), decodes the key and stores.
__global__ __launch_bounds__(kBandsThreads) void k_bands(const BandsParams B) {
    __shared__ unsigned long long s_meet[kMeanWords + 1];
    const BandsGeometry &G = B.G;
    const uint32_t tid = threadIdx.x;
    const BandsLane l = bands_lane(G, blockIdx.x, tid);

    uint64_t acc[kMeanWords];
#pragma unroll
    for (int j = 0; j < kMeanWords; ++j) acc[j] = 0;
    uint64_t key = 0;

    if (l.active) {
        const Band b = B.bands[l.band];
        const float *row = B.norms + l.win * G.W;
        const uint32_t step = bands_step(G);
        constexpr int U = 4;                                                // bins in flight per lane
        for (uint32_t bin = bands_first_bin(l, b.lo); bin < b.hi; bin += U * step) {
            uint32_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (bin + u * step < b.hi) v[u] = __float_as_uint(row[bin + u * step]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (bin + u * step < b.hi) {
                    mean_add(acc, v[u]);
                    const uint64_t k = bands_key(v[u], bin + u * step);
                    key = k > key ? k : key;
                }
            }
        }
    }

    // inside a wave: xor offsets below L stay inside the group, whose first lane is a multiple of L
    const uint32_t reach = G.L < 64u ? G.L : 64u;
#pragma unroll
    for (int j = 0; j < kMeanWords; ++j) {
        if (__ballot(acc[j] != 0) == 0) continue;                           // wave-uniform
        for (uint32_t off = reach >> 1; off; off >>= 1) acc[j] += __shfl_xor((unsigned long long)acc[j], (int)off, 64);
    }
    if (__ballot(key != 0) != 0) {
        for (uint32_t off = reach >> 1; off; off >>= 1) {
            const uint64_t o = __shfl_xor((unsigned long long)key, (int)off, 64);
            key = o > key ? o : key;
        }
    }
    if (G.L > 64u) {                                                        // the workgroup is one item: its four waves meet in LDS
        if (tid <= (uint32_t)kMeanWords) s_meet[tid] = 0;
        __syncthreads();
        if ((tid & 63u) == 0) {
#pragma unroll
            for (int j = 0; j < kMeanWords; ++j)
                if (acc[j]) atomicAdd(&s_meet[j], (unsigned long long)acc[j]);
            if (key) atomicMax(&s_meet[kMeanWords], (unsigned long long)key);
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < kMeanWords; ++j) acc[j] = s_meet[j];
            key = s_meet[kMeanWords];
        }
    }
    if (!l.active || l.lane != 0) return;
    uint32_t mb, cnt; double s;
    mean_finish_cell(acc, &mb, &s, &cnt);
    if (B.level) B.level[l.out] = __uint_as_float(mb);
    if (B.sum) B.sum[l.out] = s;
    if (B.count) B.count[l.out] = cnt;
    if (B.peak) B.peak[l.out] = __uint_as_float(bands_key_peak(key));
    if (B.peak_bin) B.peak_bin[l.out] = bands_key_bin(key);
}

// the loudest band of every window of the range from the level and count rows: 2^lg lanes a window (bands_pick_log2_lanes), each over
// its bands' keys, then the integer max across the group
__global__ __launch_bounds__(kBandsThreads) void k_bands_pick(const float *level, const uint32_t *count, uint64_t n, uint32_t K, uint32_t lg, uint8_t *pick) {
    const uint32_t tid = threadIdx.x, lanes = 1u << lg, lane = tid & (lanes - 1);
    const uint64_t i = (uint64_t)blockIdx.x * (kBandsThreads >> lg) + (tid >> lg);
    uint64_t key = 0;
    if (i < n) {
        const uint32_t *lv = reinterpret_cast<const uint32_t *>(level) + i * K;
        const uint32_t *ct = count + i * K;
        for (uint32_t k = lane; k < K; k += lanes) {
            const uint64_t o = bands_pick_key(lv[k], ct[k], k);
            key = o > key ? o : key;
        }
    }
    for (uint32_t off = lanes >> 1; off; off >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)key, (int)off, 64);
        key = o > key ? o : key;
    }
    if (i < n && lane == 0) pick[i] = bands_pick_of(key);
}

}  // namespace qd
#endif  // __HIPCC__
#endif
