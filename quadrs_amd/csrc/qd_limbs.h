// qd_limbs.h — the one fold and the one finish of the exact-sum row sinks.  A sink is a cell policy (MeanCell
// in qd_mean.h, PowerCell in qd_power.h, SpreadCell in qd_spread.h):
//   kWords                 u64 words a cell; the last one is the count word
//   add(acc, bits)         acc[0..kWords) += one value
//   Out                    the output pointers, R x W each, any may be nullptr (and what else the rounding needs)
//   round_to(acc, out, at) a cell's words rounded once into the outputs that are not nullptr, at element `at`
// k_mean<V>, k_power<V> and their *_finish kernels are one-line entry points over limb_fold and limb_finish.  k_spread and
// k_spread_finish (qd_spread.h) are the same program in their own text, for the reason given there; SpreadCell has no round_to.
#ifndef QD_LIMBS_H
#define QD_LIMBS_H

#include "qd_pool.h"

namespace qd {

// limb_fold runs on k_pool's piece geometry (PieceGeometry; the rule is qd_pieces.h, the layouts pool_geometry and power_geometry) with
// k_pool's window walker (walk_piece) and reads the carrier once.  A lane owns V bins down a piece and adds each value into its own
// cell, in registers.  Pieces of a workgroup that share a row meet in LDS, word by word (one u64 per bin: MEET = 256 V slots), with u64
// LDS adds into the slot of the first of them.  A row then ends in one of two ways:
//   whole   all of the row's windows lie in this batch and all of its pieces in this workgroup (PieceLane::whole): the leader rounds
//           the cells and stores the outputs; no global accumulator is touched.
//   cut     every other row (cut by a batch seam, or split over workgroups because the rows are few): the leader adds its non-zero
//           words with 64-bit global atomicAdd — one per word per workgroup — into the limb accumulator and raises the row's flag;
//           limb_finish, one lane per cell, rounds the flagged rows once all of their batches are through.
// The limb accumulator is planar (word k of cell c at k cells + c, cells = acc_rows W, so the lanes of a wave touch consecutive words)
// and holds rows [r_base, r_base + acc_rows) of the range.
// Workspace rule (walk_limbs, quadrs_hip.hip): the accumulator is at most max(2 chunk_bytes, one row of cells), whatever R is.  Batches
// end on multiples of pool whenever pool <= chunk windows, so rows of small pools are whole and need no accumulator; a batch that can cut
// rows is clipped to the rows the accumulator holds, and when its rows pass the accumulator's end the span is finished, the accumulator
// zeroed and moved.
template <class Cell>
struct LimbParams {
    const float *norms;                          // the batch's windows, nw x W
    PieceGeometry G;
    typename Cell::Out out;
    unsigned long long *acc;                     // planar limbs, Cell::kWords x cells
    uint32_t *flags;                             // acc_rows: the row went through the accumulator
    uint64_t r_base, acc_rows, cells;            // acc_rows 0: the host found that this launch cuts no row
};

// M by value: through a reference the kernel's arguments are memory that the atomics might change, and are loaded again behind them
// (ROCm 7.2: 60 more scalar instructions in k_power<1>)
template <class Cell, int V, int MEET>
__device__ __forceinline__ void limb_fold(const LimbParams<Cell> M) {
    static_assert(MEET >= kPoolThreads * V, "one LDS slot per bin of the workgroup");
    constexpr int kWords = Cell::kWords;
    __shared__ unsigned long long s_meet[MEET];
    const PieceGeometry &P = M.G;
    const uint32_t tid = threadIdx.x;
    const uint32_t grp = tid / P.lanes_per_win;
    const uint32_t lcol = (tid % P.lanes_per_win) * V;                                 // the lane's first bin inside the slab
    const PieceLane l = piece_lane(P, blockIdx.x, grp);

    uint64_t acc[V][kWords];
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
        for (int j = 0; j < kWords; ++j) acc[i][j] = 0;

    walk_piece<V>(M.norms + (l.wa - P.g0) * P.W + (uint64_t)l.slab * P.cols + lcol, l.wa, l.wb, P.W, [&](int i, uint32_t bits) { Cell::add(acc[i], bits); });

    // the pieces of this workgroup that share the row r meet in the LDS slot of the first of them, one word at a time; with one piece
    // a row (spr == 1) or one piece a workgroup every lane group leads its own row and nothing meets
    if (P.spr > 1 && P.pieces_per_group > 1) {
        const uint32_t slot = l.lead * P.lanes_per_win * V + lcol;
#pragma unroll
        for (int i = 0; i < V; ++i) s_meet[tid * V + i] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kWords; ++j) {
            if (l.active) {
#pragma unroll
                for (int i = 0; i < V; ++i)
                    if (acc[i][j]) atomicAdd(&s_meet[slot + i], (unsigned long long)acc[i][j]);
            }
            __syncthreads();
            // slot tid V + i is read and cleared by lane tid alone
#pragma unroll
            for (int i = 0; i < V; ++i) { acc[i][j] = s_meet[tid * V + i]; s_meet[tid * V + i] = 0; }
            __syncthreads();
        }
    }
    if (!l.active || l.lead != grp) return;
    const uint64_t col = (uint64_t)l.slab * P.cols + lcol;
    if (l.whole(P)) {
        const uint64_t o = l.r * P.W + col;
        // a cell is rounded from a copy of its own words.  Measured, not reasoned (one MI355X, ROCm 7.2, October 2026; DESIGN.md section
        // 3.24): rounded from its row of acc, k_power<1>'s pool 1 legs lay 1 % above the parent commit's in two sittings, with the copy
        // at or below them.  Whether a later compiler still needs it is a build and scripts/bench_power.py away.
#pragma unroll
        for (int i = 0; i < V; ++i) {
            uint64_t w[kWords];
#pragma unroll
            for (int j = 0; j < kWords; ++j) w[j] = acc[i][j];
            Cell::round_to(w, M.out, o + i);
        }
    } else {
        const uint64_t ra = l.r - M.r_base, cell = ra * P.W + col;
        if (ra >= M.acc_rows) return;                                    // never past the accumulator
        if (lcol == 0) M.flags[ra] = 1u;
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int j = 0; j < kWords; ++j)
                if (acc[i][j]) atomicAdd(&M.acc[(uint64_t)j * M.cells + cell + i], (unsigned long long)acc[i][j]);
    }
}

// the flagged rows of the accumulator, rows [r_base, r_base + n_rows) of the range, into the outputs: one lane per cell
template <class Cell>
__device__ __forceinline__ void limb_finish(const unsigned long long *accg, const uint32_t *flags, uint64_t cells, uint64_t r_base, uint64_t n_rows,
                                            uint32_t W, const typename Cell::Out out) {
    const uint64_t c = (uint64_t)blockIdx.x * kPoolThreads + threadIdx.x;
    if (c >= n_rows * W) return;
    if (!flags[c / W]) return;
    uint64_t acc[Cell::kWords];
#pragma unroll
    for (int j = 0; j < Cell::kWords; ++j) acc[j] = accg[(uint64_t)j * cells + c];
    Cell::round_to(acc, out, r_base * W + c);
}

}  // namespace qd
#endif
