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

namespace qd {

constexpr int kPoolThreads = 256;
constexpr uint32_t kPoolInfBits = 0x7f800000u;
constexpr uint32_t kPoolSlabCols = 1024;         // bins one workgroup covers: 256 lanes x 4
constexpr uint64_t kPoolMinSeg = 16;             // a row is not split into pieces shorter than this many windows
constexpr int kPoolGroupsPerCu = 4;              // workgroups per compute unit a launch aims for before it stops splitting rows

// Geometry of a launch over one batch: windows [g0, g0 + nw) of a range of n_total windows (g0 counts from the range's first window),
// W f32 each (W a power of two), pooled `pool` windows to a row.
//   piece   `seg` consecutive windows of one output row: row r is cut at r pool, r pool + seg, ... into spr = ceil(pool / seg) pieces,
//           numbered q = r spr + k over the whole range, so a batch holds the pieces q0 ... q0 + n_pieces - 1 (its first and last
//           clipped to the batch).  One lane group runs down one piece.
//   lanes   a lane owns V consecutive bins (V = 4, one 16-byte load a window; W < 4: V = 1); lanes_per_win = min(W, 1024) / V lanes
//           cover a window's bins (W > 1024: n_slabs column slabs of 1024 bins, a workgroup each), so the lanes of a wave read
//           consecutive bins, and for W < 256 a wave spans 256 / W pieces; pieces_per_group = 256 / lanes_per_win pieces share a
//           workgroup and each lane derives its own row from its piece.
//   split   seg = pool (a row is one piece) while the batch's rows alone give kPoolGroupsPerCu workgroups per compute unit: pool = 1
//           is one window per lane group and R large.  With fewer rows a row is cut into as many pieces as reach that number, of at
//           least kPoolMinSeg windows: pool = n is one row with every workgroup on it.
//   flush   the pieces of a workgroup that share a row are combined in LDS (slot of the first of them); that leader stores the row when
//           all of the row's windows lie in this batch and all of its pieces in this workgroup — nobody else contributes to those words
//           within the call — and otherwise uses atomicMax / atomicMin on the accumulator, which holds the fold identities from before
//           the first batch.
struct PoolParams {
    const float *norms;                          // the batch's windows, nw x W
    uint32_t *peak, *floor;                      // R x W words each; either may be nullptr
    uint64_t g0, nw, n_total, pool, seg, spr, q0, n_pieces;
    uint32_t W, cols, lanes_per_win, pieces_per_group, n_slabs;
    uint32_t vec_store;                          // both accumulators are 16-byte aligned: a stored row goes out as one uint4 per lane
};

template <int V>
__global__ __launch_bounds__(kPoolThreads) void k_pool(const PoolParams P) {
    __shared__ uint32_t s_peak[kPoolSlabCols], s_floor[kPoolSlabCols];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kPoolSlabCols; i += kPoolThreads) { s_peak[i] = 0; s_floor[i] = kPoolInfBits; }
    __syncthreads();

    const uint32_t slab = blockIdx.x % P.n_slabs;
    const uint64_t grp0 = (uint64_t)(blockIdx.x / P.n_slabs) * P.pieces_per_group;     // the workgroup's first piece, within the batch
    const uint32_t grp = tid / P.lanes_per_win;
    const uint32_t lcol = (tid % P.lanes_per_win) * V;                                 // the lane's first bin inside the slab
    const bool active = grp0 + grp < P.n_pieces;
    const uint64_t wg_q0 = P.q0 + grp0, q = wg_q0 + grp;
    const uint64_t r = q / P.spr, k = q - r * P.spr;
    const uint64_t row_a = r * P.pool, row_b = row_a + P.pool < P.n_total ? row_a + P.pool : P.n_total;
    const uint64_t end = P.g0 + P.nw;
    uint64_t wa = row_a + k * P.seg, wb = wa + P.seg;
    wa = wa > P.g0 ? wa : P.g0;
    wb = wb < row_b ? wb : row_b;
    wb = wb < end ? wb : end;
    if (!active) wa = wb = P.g0;

    uint32_t mx[V], mn[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = 0; mn[i] = kPoolInfBits; }

    constexpr int U = 4;                                                // windows in flight per lane
    const float *ptr = P.norms + (wa - P.g0) * P.W + (uint64_t)slab * P.cols + lcol;
    for (uint64_t w = wa; w < wb; w += U, ptr += (uint64_t)U * P.W) {
        float v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (w + u < wb) {
                if (V == 4) {
                    const float4 f = *reinterpret_cast<const float4 *>(ptr + (uint64_t)u * P.W);
                    v[u][0] = f.x; v[u][1 % V] = f.y; v[u][2 % V] = f.z; v[u][3 % V] = f.w;
                } else {
                    v[u][0] = ptr[(uint64_t)u * P.W];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (w + u < wb) {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float x = v[u][i];
                    const uint32_t b = __float_as_uint(x) & 0x7fffffffu;
                    if (!(x != x)) {
                        mx[i] = b > mx[i] ? b : mx[i];
                        mn[i] = b < mn[i] ? b : mn[i];
                    }
                }
            }
        }
    }

    // the pieces of this workgroup that share the row r meet in the LDS slot of the first of them
    const uint64_t row_q0 = r * P.spr;
    const uint32_t lead = row_q0 > wg_q0 ? (uint32_t)(row_q0 - wg_q0) : 0u;           // <= grp
    if (active) {
        const uint32_t slot = lead * P.lanes_per_win * V + lcol;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (mx[i] != 0) atomicMax(&s_peak[slot + i], mx[i]);
            if (mn[i] != kPoolInfBits) atomicMin(&s_floor[slot + i], mn[i]);
        }
    }
    __syncthreads();
    if (!active || lead != grp) return;
    // the leader's slot is tid * V.  Alone on the row within the call: store; else plain HIP atomics, commutative and exact
    const bool whole = row_q0 >= wg_q0 && row_q0 + P.spr <= wg_q0 + P.pieces_per_group && row_a >= P.g0 && row_b <= end;
    const uint64_t o = r * P.W + (uint64_t)slab * P.cols + lcol;
#pragma unroll
    for (int i = 0; i < V; ++i) { mx[i] = s_peak[tid * V + i]; mn[i] = s_floor[tid * V + i]; }
    if (whole) {
        if (V == 4 && P.vec_store) {
            if (P.peak) *reinterpret_cast<uint4 *>(P.peak + o) = make_uint4(mx[0], mx[1 % V], mx[2 % V], mx[3 % V]);
            if (P.floor) *reinterpret_cast<uint4 *>(P.floor + o) = make_uint4(mn[0], mn[1 % V], mn[2 % V], mn[3 % V]);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (P.peak) P.peak[o + i] = mx[i];
                if (P.floor) P.floor[o + i] = mn[i];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (P.peak && mx[i] != 0) atomicMax(&P.peak[o + i], mx[i]);
            if (P.floor && mn[i] != kPoolInfBits) atomicMin(&P.floor[o + i], mn[i]);
        }
    }
}

// the launch geometry for the batch [g0, g0 + nw) (nw >= 1, 1 <= pool) on a device of n_cu compute units; *grid in workgroups
inline void pool_geometry(uint64_t g0, uint64_t nw, uint64_t n_total, uint64_t pool, uint32_t W, int n_cu, PoolParams *P, uint64_t *grid, int *V) {
    *V = W >= 4 ? 4 : 1;
    P->g0 = g0; P->nw = nw; P->n_total = n_total; P->pool = pool; P->W = W;
    P->cols = W < kPoolSlabCols ? W : kPoolSlabCols;
    P->lanes_per_win = P->cols / *V;
    P->pieces_per_group = kPoolThreads / P->lanes_per_win;
    P->n_slabs = W / P->cols;
    uint64_t want = (uint64_t)n_cu * kPoolGroupsPerCu * P->pieces_per_group / P->n_slabs;
    if (want < 1) want = 1;
    const uint64_t rows = nw / pool + 1;
    uint64_t seg = pool;
    if (rows < want) {
        const uint64_t cuts = (want + rows - 1) / rows;
        seg = (pool + cuts - 1) / cuts;
        const uint64_t least = pool < kPoolMinSeg ? pool : kPoolMinSeg;
        if (seg < least) seg = least;
    }
    P->seg = seg;
    P->spr = (pool + seg - 1) / seg;
    const uint64_t wl = g0 + nw - 1;
    P->q0 = g0 / pool * P->spr + g0 % pool / seg;
    P->n_pieces = wl / pool * P->spr + wl % pool / seg - P->q0 + 1;
    *grid = (P->n_pieces + P->pieces_per_group - 1) / P->pieces_per_group * P->n_slabs;
}

}  // namespace qd
#endif
