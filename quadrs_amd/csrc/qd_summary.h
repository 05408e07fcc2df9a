// qd_summary.h — the level summary of norms rows (qd_plan_summarize): k_summary folds a batch of the norms
// sink's rows into a device accumulator; qd_summary_fold (quadrs_hip.hip) is its CPU twin.
//
// Every field of the summary is a max, a min or an integer sum, so neither the split of the rows over workgroups and launches nor the
// order the atomics arrive in changes a bit of the result.  Norms are hypot(re, im): non-negative or NaN.  Non-negative f32 order as
// their bit patterns do, so the kernel keeps the running max / min as u32; NaNs are taken out with x != x before any integer compare.
#ifndef QD_SUMMARY_H
#define QD_SUMMARY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qd {

constexpr int kSumThreads = 256;
constexpr int kSumBuckets = 2048;                // bits(|x|) >> 20: 8 buckets per octave, +inf in 2040, 2041 ... 2047 NaN patterns only
constexpr uint32_t kSumNanBucket = 2047;         // ... so a workgroup counts its NaNs in LDS bucket 2047 and flushes that one to n_nan
constexpr uint32_t kSumInfBits = 0x7f800000u;
constexpr uint32_t kSumSlabCols = 1024;          // bins one workgroup covers: 256 lanes x 4
constexpr uint64_t kSumMaxPerGroup = 1ull << 30; // values one workgroup may count (its LDS counters are u32)

// the device accumulator: [hist u64 x 2048][n_nan u64][peak u32 x W][floor u32 x W], set to the fold identities before the first launch
struct SumAcc {
    unsigned long long hist[kSumBuckets];
    unsigned long long n_nan;
};
inline size_t sum_acc_bytes(uint64_t W) { return sizeof(SumAcc) + 2 * W * sizeof(uint32_t); }

// Geometry of a launch over rows of W f32 (W a power of two).  A workgroup owns `cols` consecutive bins (a column slab) of a run of
// rows; `lanes_per_row` lanes of V bins each cover the slab, so rows_per_pass = 256 / lanes_per_row rows share a pass.  A lane's bins
// never change: its running max / min stay in registers and are folded across the lanes of the workgroup once, at the end.
//   W < 256   : one slab, 1024 / W rows per pass (V = 4; W < 4: V = 1 and 256 / W rows)
//   W >= 256  : lanes stride over the bins: min(W, 1024) / 4 lanes a row, W / 1024 slabs
struct SumParams {
    const float *norms;
    uint64_t n_rows, rows_per_group;
    uint32_t W, cols, lanes_per_row, rows_per_pass, n_slabs;
    SumAcc *acc;                                 // peak / floor behind it
};

// One value into the wave's histogram.  Noise puts most values into a handful of buckets and an all-zero stream puts every value into
// bucket 0: a wave whose active lanes all hold the same bucket adds their count from one lane (UNIFORM), everything else is one LDS
// atomic per lane.
template <bool UNIFORM>
__device__ __forceinline__ void sum_count(uint32_t *hist, uint32_t bucket) {
    if (UNIFORM) {
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bucket);
        const unsigned long long active = __ballot(1);
        if (__ballot(bucket == first) == active) {
            if ((int)__lane_id() == __ffsll((long long)active) - 1) atomicAdd(&hist[first], (uint32_t)__popcll(active));
            return;
        }
    }
    atomicAdd(&hist[bucket], 1u);
}

// LAYOUT bit 0: one histogram copy for the workgroup instead of one per wave; bit 1: no wave-uniform shortcut.  The library launches
// layout 0; the others exist for scripts/bench_summary.py's comparison (development builds).
template <int V, int LAYOUT>
__global__ __launch_bounds__(kSumThreads) void k_summary(const SumParams P) {
    constexpr int HC = (LAYOUT & 1) ? 1 : kSumThreads / 64;
    constexpr bool UNIFORM = !(LAYOUT & 2);
    __shared__ uint32_t s_hist[HC][kSumBuckets];
    __shared__ uint32_t s_peak[kSumSlabCols], s_floor[kSumSlabCols];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (uint32_t)(HC * kSumBuckets); i += kSumThreads) (&s_hist[0][0])[i] = 0;
    for (uint32_t i = tid; i < kSumSlabCols; i += kSumThreads) { s_peak[i] = 0; s_floor[i] = kSumInfBits; }
    __syncthreads();

    uint32_t *hist = s_hist[HC == 1 ? 0 : tid / 64];
    const uint32_t slab = blockIdx.x % P.n_slabs;
    const uint64_t grp = blockIdx.x / P.n_slabs;
    const uint32_t lcol = (tid % P.lanes_per_row) * V;                  // the lane's first bin inside the slab
    const uint64_t r0 = grp * P.rows_per_group;
    const uint64_t r1 = r0 + P.rows_per_group < P.n_rows ? r0 + P.rows_per_group : P.n_rows;
    const float *base = P.norms + (uint64_t)slab * P.cols + lcol;
    uint32_t mx[V], mn[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { mx[k] = 0; mn[k] = kSumInfBits; }

    constexpr int U = 4;                                                // rows in flight per lane
    for (uint64_t r = r0 + tid / P.lanes_per_row; r < r1; r += (uint64_t)U * P.rows_per_pass) {
        float v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t rr = r + (uint64_t)u * P.rows_per_pass;
            if (rr < r1) {
                if (V == 4) {
                    const float4 q = *reinterpret_cast<const float4 *>(base + rr * P.W);
                    v[u][0] = q.x; v[u][1 % V] = q.y; v[u][2 % V] = q.z; v[u][3 % V] = q.w;
                } else {
                    v[u][0] = base[rr * P.W];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r + (uint64_t)u * P.rows_per_pass < r1) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float x = v[u][k];
                    const bool is_nan = x != x;
                    const uint32_t b = __float_as_uint(x) & 0x7fffffffu;
                    if (!is_nan) {
                        mx[k] = b > mx[k] ? b : mx[k];
                        mn[k] = b < mn[k] ? b : mn[k];
                    }
                    sum_count<UNIFORM>(hist, is_nan ? kSumNanBucket : b >> 20);
                }
            }
        }
    }

    // across the lanes that share a bin, then one flush per workgroup: plain HIP atomics, commutative and exact
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (mx[k] != 0) atomicMax(&s_peak[lcol + k], mx[k]);
        if (mn[k] != kSumInfBits) atomicMin(&s_floor[lcol + k], mn[k]);
    }
    __syncthreads();
    uint32_t *peak = reinterpret_cast<uint32_t *>(P.acc + 1), *floor = peak + P.W;
    for (uint32_t i = tid; i < P.cols; i += kSumThreads) {
        const uint32_t c = slab * P.cols + i;
        if (s_peak[i] != 0) atomicMax(&peak[c], s_peak[i]);
        if (s_floor[i] != kSumInfBits) atomicMin(&floor[c], s_floor[i]);
    }
    for (uint32_t i = tid; i < (uint32_t)kSumBuckets; i += kSumThreads) {
        uint32_t c = 0;
#pragma unroll
        for (int h = 0; h < HC; ++h) c += s_hist[h][i];
        if (c) atomicAdd(i == kSumNanBucket ? &P.acc->n_nan : &P.acc->hist[i], (unsigned long long)c);
    }
}

// the launch geometry for n_rows rows of width W on a device of n_cu compute units
inline void sum_geometry(uint64_t n_rows, uint32_t W, int n_cu, SumParams *P, uint32_t *grid, int *V) {
    *V = W >= 4 ? 4 : 1;
    P->n_rows = n_rows; P->W = W;
    P->cols = W < kSumSlabCols ? W : kSumSlabCols;
    P->lanes_per_row = P->cols / *V;
    P->rows_per_pass = kSumThreads / P->lanes_per_row;
    P->n_slabs = W / P->cols;
    // enough workgroups to fill the device (8 per CU), each with at least a few passes of rows; a workgroup counts fewer than 2^32
    // values into its u32 LDS counters by construction (kSumMaxPerGroup), so it flushes exactly once
    const uint64_t quantum = (uint64_t)P->rows_per_pass * 4;
    uint64_t groups = (uint64_t)n_cu * 8 / P->n_slabs;
    if (groups < 1) groups = 1;
    uint64_t rpg = (n_rows + groups - 1) / groups;
    rpg = (rpg + quantum - 1) / quantum * quantum;
    const uint64_t cap = kSumMaxPerGroup / P->cols;                  // >= 2^20 rows, a multiple of every quantum
    if (rpg > cap) rpg = cap;
    P->rows_per_group = rpg;
    *grid = (uint32_t)((n_rows + rpg - 1) / rpg * P->n_slabs);
}

}  // namespace qd
#endif
