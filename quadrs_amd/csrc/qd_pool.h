// qd_pool.h — peak-hold rows of norms rows (qd_plan_pool): k_pool folds a batch of the norms sink's windows,
// each group of `pool` consecutive windows per bin, into the R x W accumulators; qd_pool_fold (quadrs_hip.hip) is its CPU twin.
//
// A pooled row is a max / min fold, so neither the split of the windows over lanes, workgroups, batches and launches nor the order the
// atomics arrive in changes a bit of it.  Norms are hypot(re, im): non-negative or NaN.  Non-negative f32 order as their bit patterns
// do, so the running max / min are u32 (qd_summary.h); NaNs are taken out with x != x before any integer compare.
#ifndef QD_POOL_H
#define QD_POOL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qd_pieces.h"

namespace qd {

constexpr int kPoolThreads = 256;
constexpr uint32_t kPoolInfBits = 0x7f800000u;
constexpr uint32_t kPoolSlabCols = 1024;         // bins one workgroup covers: 256 lanes x 4
constexpr uint64_t kPoolMinSeg = 16;             // a row is not split into pieces shorter than this many windows
constexpr int kPoolGroupsPerCu = 4;              // workgroups per compute unit a launch aims for before it stops splitting rows

// k_pool's parameters: the launch geometry (qd_pieces.h: pieces, lanes, split and flush) and its own pointers.
struct PoolParams {
    const float *norms;                          // the batch's windows, nw x W
    uint32_t *peak, *floor;                      // R x W words each; either may be nullptr
    PieceGeometry G;
    uint32_t vec_store;                          // both accumulators are 16-byte aligned: a stored row goes out as one uint4 per lane
};

// The window walker of k_pool and k_mean: a lane runs down the windows [l.wa, l.wb) of its piece at the V bins from `lcol` of its slab,
// U = 4 windows in flight, one 16-byte (V = 4) or one 4-byte load per window, and hands each(i, bits) every value's raw bits, i its bin.
template <int V, class F>
__device__ __forceinline__ void walk_piece(const float *ptr, uint64_t wa, uint64_t wb, uint32_t W, F &&each) {
    constexpr int U = 4;                                                // windows in flight per lane
    for (uint64_t w = wa; w < wb; w += U, ptr += (uint64_t)U * W) {
        uint32_t v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (w + u < wb) {
                if (V == 4) {
                    const uint4 f = *reinterpret_cast<const uint4 *>(ptr + (uint64_t)u * W);
                    v[u][0] = f.x; v[u][1 % V] = f.y; v[u][2 % V] = f.z; v[u][3 % V] = f.w;
                } else {
                    v[u][0] = __float_as_uint(ptr[(uint64_t)u * W]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (w + u < wb) {
#pragma unroll
                for (int i = 0; i < V; ++i) each(i, v[u][i]);
            }
        }
    }
}

template <int V>
__global__ __launch_bounds__(kPoolThreads) void k_pool(const PoolParams Q) {
    __shared__ uint32_t s_peak[kPoolSlabCols], s_floor[kPoolSlabCols];
    const PieceGeometry &P = Q.G;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kPoolSlabCols; i += kPoolThreads) { s_peak[i] = 0; s_floor[i] = kPoolInfBits; }
    __syncthreads();

    const uint32_t grp = tid / P.lanes_per_win;
    const uint32_t lcol = (tid % P.lanes_per_win) * V;                                 // the lane's first bin inside the slab
    const PieceLane l = piece_lane(P, blockIdx.x, grp);

    uint32_t mx[V], mn[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = 0; mn[i] = kPoolInfBits; }

    walk_piece<V>(Q.norms + (l.wa - P.g0) * P.W + (uint64_t)l.slab * P.cols + lcol, l.wa, l.wb, P.W, [&](int i, uint32_t bits) {
        const float x = __uint_as_float(bits);
        const uint32_t b = bits & 0x7fffffffu;
        if (!(x != x)) {
            mx[i] = b > mx[i] ? b : mx[i];
            mn[i] = b < mn[i] ? b : mn[i];
        }
    });

    // the pieces of this workgroup that share the row r meet in the LDS slot of the first of them
    if (l.active) {
        const uint32_t slot = l.lead * P.lanes_per_win * V + lcol;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (mx[i] != 0) atomicMax(&s_peak[slot + i], mx[i]);
            if (mn[i] != kPoolInfBits) atomicMin(&s_floor[slot + i], mn[i]);
        }
    }
    __syncthreads();
    if (!l.active || l.lead != grp) return;
    // the leader's slot is tid * V.  Alone on the row within the call: store; else plain HIP atomics, commutative and exact
    const uint64_t o = l.r * P.W + (uint64_t)l.slab * P.cols + lcol;
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = s_peak[tid * V + i]; mn[i] = s_floor[tid * V + i]; }
    if (l.whole(P)) {
        if (V == 4 && Q.vec_store) {
            if (Q.peak) *reinterpret_cast<uint4 *>(Q.peak + o) = make_uint4(mx[0], mx[1 % V], mx[2 % V], mx[3 % V]);
            if (Q.floor) *reinterpret_cast<uint4 *>(Q.floor + o) = make_uint4(mn[0], mn[1 % V], mn[2 % V], mn[3 % V]);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (Q.peak) Q.peak[o + i] = mx[i];
                if (Q.floor) Q.floor[o + i] = mn[i];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (Q.peak && mx[i] != 0) atomicMax(&Q.peak[o + i], mx[i]);
            if (Q.floor && mn[i] != kPoolInfBits) atomicMin(&Q.floor[o + i], mn[i]);
        }
    }
}

// the launch geometry for the batch [g0, g0 + nw) (nw >= 1, 1 <= pool) on a device of n_cu compute units; *grid in workgroups
inline void pool_geometry(uint64_t g0, uint64_t nw, uint64_t n_total, uint64_t pool, uint32_t W, int n_cu, PieceGeometry *P, uint64_t *grid, int *V) {
    *V = W >= 4 ? 4 : 1;
    const uint32_t cols = W < kPoolSlabCols ? W : kPoolSlabCols, lanes_per_win = cols / *V;
    piece_split(g0, nw, n_total, pool, W, cols, lanes_per_win, kPoolThreads / lanes_per_win, kPoolMinSeg, kPoolGroupsPerCu, n_cu, P, grid);
}

}  // namespace qd
#endif
