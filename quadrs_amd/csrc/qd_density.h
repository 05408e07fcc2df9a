// qd_density.h — per-bin level counts of norms rows (qd_plan_density): k_density folds a batch of the norms sink's
// windows, each group of `pool` consecutive windows per bin, into counts over a window of the summary's bucket scale; density_quantile_level
// reads a percentile off a cell.  qd_density_fold / qd_density_quantile (quadrs_hip.hip) are the CPU twins and use the same functions.
//
// Every cell is an integer count, so neither the split of the windows over lanes, workgroups, batches and launches nor the order the
// atomics arrive in changes a bit of it.
#ifndef QD_DENSITY_H
#define QD_DENSITY_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QD_DENSITY_HD __host__ __device__
#else
#define QD_DENSITY_HD
#endif

#include "qd_pieces.h"

namespace qd {

constexpr uint32_t kDensityMaxLevels = 256;      // L
constexpr uint32_t kDensityBuckets = 2041;       // buckets 0 ... 2040 of bits >> 20; +inf is 2040
constexpr uint64_t kDensityMaxCount = 1ull << 31;            // windows a group may hold
constexpr uint32_t kDensityNanBits = 0x7fc00000u;            // both bounds of a cell without values
constexpr int kDensityMaxQ = 8;
constexpr uint64_t kDensityMaxWorkspace = 1ull << 30;        // QD_DENSITY_MAX_WORKSPACE

// the level of a value on the grid [level0, level0 + L), or L for a NaN
QD_DENSITY_HD inline uint32_t density_level(uint32_t bits, uint32_t level0, uint32_t L) {
    bits &= 0x7fffffffu;
    if (bits > 0x7f800000u) return L;
    uint32_t k = bits >> 20;
    k = k > level0 ? k : level0;
    k -= level0;
    return k < L - 1 ? k : L - 1;
}

// the level j of a cell's q-quantile (qd_summary_quantile's rule): N = sum of the L counts (> 0), r = max(1, ceil(q N)) in f64, j the first
// level whose cumulative count reaches r.  `stride` words lie between a cell's consecutive levels.
QD_DENSITY_HD inline uint32_t density_quantile_level(const uint32_t *c, uint64_t stride, uint32_t L, uint64_t N, double q) {
    const double want = ceil(q * (double)N);
    const uint64_t r = want < 1.0 ? 1 : (want >= (double)N ? N : (uint64_t)want);
    uint64_t cum = 0;
    uint32_t j = 0;
    for (; j + 1 < L; ++j) { cum += c[j * stride]; if (cum >= r) break; }
    return j;
}
QD_DENSITY_HD inline uint32_t density_lo_bits(uint32_t level0, uint32_t j) { return j ? (level0 + j) << 20 : 0u; }
QD_DENSITY_HD inline uint32_t density_hi_bits(uint32_t level0, uint32_t L, uint32_t j) { return j + 1 < L ? (level0 + j + 1) << 20 : 0x7f800000u; }

constexpr int kDensityThreads = 256;
constexpr uint32_t kDensityLdsWords = 16384;     // the workgroup histogram: 64 KiB of static LDS
constexpr uint64_t kDensityMinSeg = 128;         // a row is not split into pieces shorter than this many windows
constexpr int kDensityGroupsPerCu = 4;           // workgroups per compute unit a launch aims for before it stops splitting rows
constexpr int kDensityInFlight = 8;              // windows in flight per lane

// Geometry of a launch over one batch: the pooled folds' pieces (qd_pieces.h), with a column layout that L decides:
//   columns  a workgroup's histogram is hist[level][column], level-major, ncol columns wide: ncol is the largest power of two with
//            ncol L <= 16384 words, at most 256 and at least 64 (L = 256: 64; L <= 64: 256).  Column c = slot cols + bin is bin `bin` of
//            the slab for the workgroup's piece number `slot`: cols = min(W, ncol) bins a slab (n_slabs = W / cols slabs, a workgroup
//            each — k_pool's 1024-bin slab would need 1024 L words) and pieces_per_group = ncol / cols pieces a workgroup, each with its
//            own run of columns, so pieces of different rows never meet.
//   banks    lane t adds to column t mod ncol: the lanes of a wave hold 64 consecutive columns, ncol is a multiple of 64 and a level
//            moves the address by a multiple of ncol words, so lane i of a wave is on bank i mod 64 (i mod 32 within its half, where the
//            LDS serves a half at a time) WHATEVER levels the wave's values have: no add of one instruction shares a bank with another.
//            W < 64: a wave spans 64 / W pieces, whose column runs are consecutive, so the rule holds unchanged.  This rests on the
//            bank rule, not on a counter reading.
//   lanes    a lane owns one bin (one 4-byte load a window; the lanes of a wave read 64 consecutive f32).  ncol < 256 (L > 64): the
//            nsub = 256 / ncol lanes t, t + ncol, ... share a column and take its piece's windows in turn (window wa + sub, step nsub);
//            they are in different waves, so they meet only in the LDS adder.
//   split    piece_split with this kernel's figures: kDensityGroupsPerCu workgroups per compute unit and pieces of at least
//            kDensityMinSeg windows — a piece pays up to L words of flush per column, so it is 8 times k_pool's shortest.
//   flush    the lanes of the first piece of a row in the workgroup add up the row's pieces here, level by level (lane sub takes levels
//            sub, sub + nsub, ...).  Whole row (all windows in this batch, all pieces in this workgroup: PieceLane::whole): the
//            non-zero counts are stored; cut row: they are added with u32 atomicAdd.  The accumulator is zero from before the first
//            batch, so zero counts are never written.
struct DensityParams {
    const float *norms;                          // the batch's windows, nw x W
    PieceGeometry G;
    uint32_t *counts;                            // R x W x L words
    uint32_t level0, L, ncol, nsub;
};

// One lane's two halves of k_density, as functions of the lane's piece (PieceLane of its slot) and its own place over a memory policy M,
// so that a host program can walk every lane of a launch with a policy that checks bounds and counts the reads and the stores.
struct DensityLane { uint32_t col, sub, slot, bin; };
QD_DENSITY_HD inline DensityLane density_lane(const DensityParams &D, uint32_t tid) {
    DensityLane d;
    d.col = tid % D.ncol; d.sub = tid / D.ncol;
    d.slot = d.col / D.G.cols; d.bin = d.col % D.G.cols;
    return d;
}

template <class M>
QD_DENSITY_HD inline void density_lane_fold(const DensityParams &D, const PieceLane &l, const DensityLane &d, uint32_t *hist, M &mem) {
    const PieceGeometry &P = D.G;
    constexpr int U = kDensityInFlight;
    const uint64_t step = (uint64_t)D.nsub * P.W;
    const float *ptr = D.norms + (l.wa - P.g0 + d.sub) * P.W + (uint64_t)l.slab * P.cols + d.bin;
    uint32_t *mine = hist + d.col;
    for (uint64_t w = l.wa + d.sub; w < l.wb; w += (uint64_t)U * D.nsub, ptr += (uint64_t)U * step) {
        uint32_t v[U];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int u = 0; u < U; ++u)
            if (w + (uint64_t)u * D.nsub < l.wb) v[u] = mem.load(ptr + (uint64_t)u * step);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int u = 0; u < U; ++u) {
            if (w + (uint64_t)u * D.nsub < l.wb) {
                const uint32_t lv = density_level(v[u], D.level0, D.L);
                if (lv < D.L) mem.lds_add(mine + lv * D.ncol);
            }
        }
    }
}

template <class M>
QD_DENSITY_HD inline void density_lane_flush(const DensityParams &D, const PieceLane &l, const DensityLane &d, const uint32_t *hist, M &mem) {
    const PieceGeometry &P = D.G;
    if (!l.active || l.lead != d.slot) return;
    uint32_t *out = D.counts + (l.r * P.W + (uint64_t)l.slab * P.cols + d.bin) * D.L;
    const uint32_t n_same = l.n_same(P);
    const bool whole = l.whole(P);
    for (uint32_t lv = d.sub; lv < D.L; lv += D.nsub) {
        const uint32_t *h = hist + lv * D.ncol + d.col;
        uint32_t c = 0;
        for (uint32_t s = 0; s < n_same; ++s) c += h[s * P.cols];
        if (c == 0) continue;
        if (whole) mem.store(out + lv, c); else mem.add(out + lv, c);
    }
}

// the launch geometry for the batch [g0, g0 + nw) (nw >= 1, 1 <= pool, 1 <= L <= 256) on a device of n_cu compute units; *grid in workgroups
inline void density_geometry(uint64_t g0, uint64_t nw, uint64_t n_total, uint64_t pool, uint32_t W, uint32_t L, int n_cu, DensityParams *D, uint64_t *grid) {
    uint32_t ncol = 64;
    while (ncol * 2 * L <= kDensityLdsWords && ncol * 2 <= (uint32_t)kDensityThreads) ncol *= 2;
    D->ncol = ncol; D->nsub = kDensityThreads / ncol; D->L = L;
    const uint32_t cols = W < ncol ? W : ncol;
    piece_split(g0, nw, n_total, pool, W, cols, cols, ncol / cols, kDensityMinSeg, kDensityGroupsPerCu, n_cu, &D->G, grid);
}

}  // namespace qd

#if defined(__HIPCC__)
namespace qd {

struct DensityDeviceMem {
    __device__ uint32_t load(const float *p) const { return __float_as_uint(*p); }
    __device__ void lds_add(uint32_t *p) const { atomicAdd(p, 1u); }                   // result unused: an add without return
    __device__ void store(uint32_t *p, uint32_t v) const { *p = v; }
    __device__ void add(uint32_t *p, uint32_t v) const { atomicAdd(p, v); }
};

__global__ __launch_bounds__(kDensityThreads) void k_density(const DensityParams D) {
    __shared__ uint32_t s_hist[kDensityLdsWords];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < D.ncol * D.L; i += kDensityThreads) s_hist[i] = 0;
    __syncthreads();
    DensityDeviceMem mem;
    const DensityLane d = density_lane(D, tid);
    const PieceLane l = piece_lane(D.G, blockIdx.x, d.slot);
    density_lane_fold(D, l, d, s_hist, mem);
    __syncthreads();
    density_lane_flush(D, l, d, s_hist, mem);
}

struct DensityQ { double q[kDensityMaxQ]; };

// one lane per cell: the lo bound of the level of each of the n_q quantiles, trace i at i cells; a cell without values: the quiet NaN
__global__ __launch_bounds__(kDensityThreads) void k_density_quantile(const uint32_t *counts, uint64_t cells, uint32_t level0, uint32_t L, const DensityQ Q,
                                                                      uint32_t n_q, uint32_t *trace) {
    const uint64_t c = (uint64_t)blockIdx.x * kDensityThreads + threadIdx.x;
    if (c >= cells) return;
    const uint32_t *cell = counts + c * L;
    uint64_t N = 0;
    for (uint32_t l = 0; l < L; ++l) N += cell[l];
    for (uint32_t i = 0; i < n_q; ++i)
        trace[(uint64_t)i * cells + c] = N ? density_lo_bits(level0, density_quantile_level(cell, 1, L, N, Q.q[i])) : kDensityNanBits;
}

}  // namespace qd
#endif  // __HIPCC__
#endif
