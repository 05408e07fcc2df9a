// qd_pieces.h — how the pooled folds (k_pool, k_mean, k_density) cut a batch of windows into pieces, and what a
// lane group of a launch does with its piece: plain-integer rules, stated once.
//
// The kernels take every index from piece_lane; the host (quadrs_hip.hip, through pool_geometry and density_geometry) fills the geometry
// with piece_split.  Nothing here is HIP-specific: the header compiles as plain C++17 on the host, where a program can walk every
// (workgroup, slot) of a launch (tests/test_pieces_cpu.py), and under hipcc.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define QD_PIECES_HD __host__ __device__
#else
#define QD_PIECES_HD
#endif

namespace qd {

// Geometry of a launch over one batch: windows [g0, g0 + nw) of a range of n_total windows (g0 counts from the range's first window),
// W f32 each (W a power of two), pooled `pool` windows to a row.
//   piece   `seg` consecutive windows of one output row: row r is cut at r pool, r pool + seg, ... into spr = ceil(pool / seg) pieces,
//           numbered q = r spr + k over the whole range, so a batch holds the pieces q0 ... q0 + n_pieces - 1 (its first and last
//           clipped to the batch).  One lane group runs down one piece.
//   lanes   the kernel's column layout: lanes_per_win lanes cover the `cols` bins of a window that a workgroup takes (W > cols: n_slabs
//           = W / cols column slabs, a workgroup each), so the lanes of a wave read consecutive bins; pieces_per_group pieces share a
//           workgroup, piece number `slot` of them on its own lane group, and each lane group derives its own row from its piece.
//           k_pool and k_mean: a lane owns V consecutive bins (V = 4, one 16-byte load a window; W < 4: V = 1), cols = min(W, 1024),
//           lanes_per_win = cols / V, pieces_per_group = 256 / lanes_per_win: for W < 256 a wave spans 256 / W pieces.  k_density:
//           qd_density.h, where the number of levels decides.
//   split   seg = pool (a row is one piece) while the batch's rows alone give the kernel's workgroups per compute unit: pool = 1 is one
//           window per lane group and R large.  With fewer rows a row is cut into as many pieces as reach that number, of at least the
//           kernel's shortest piece: pool = n is one row with every workgroup on it.
//   flush   the pieces of a workgroup that share a row are combined in LDS (slot of the first of them, `lead`); that leader stores the
//           row when all of the row's windows lie in this batch and all of its pieces in this workgroup (`whole`) — nobody else
//           contributes to those words within the call — and otherwise uses atomics on the accumulator, which holds the fold
//           identities from before the first batch.
struct PieceGeometry {
    uint64_t g0, nw, n_total, pool, seg, spr, q0, n_pieces;
    uint32_t W, cols, lanes_per_win, pieces_per_group, n_slabs;
};

// The split rule: the geometry of the batch [g0, g0 + nw) (nw >= 1, 1 <= pool) for a kernel of the given column layout that aims at
// groups_per_cu workgroups on each of n_cu compute units and cuts no row into pieces shorter than min_seg windows; *grid in workgroups.
inline void piece_split(uint64_t g0, uint64_t nw, uint64_t n_total, uint64_t pool, uint32_t W, uint32_t cols, uint32_t lanes_per_win,
                        uint32_t pieces_per_group, uint64_t min_seg, int groups_per_cu, int n_cu, PieceGeometry *G, uint64_t *grid) {
    G->g0 = g0; G->nw = nw; G->n_total = n_total; G->pool = pool; G->W = W;
    G->cols = cols; G->lanes_per_win = lanes_per_win; G->pieces_per_group = pieces_per_group;
    G->n_slabs = W / cols;
    uint64_t want = (uint64_t)n_cu * groups_per_cu * pieces_per_group / G->n_slabs;
    if (want < 1) want = 1;
    const uint64_t rows = nw / pool + 1;
    uint64_t seg = pool;
    if (rows < want) {
        const uint64_t cuts = (want + rows - 1) / rows;
        seg = (pool + cuts - 1) / cuts;
        const uint64_t least = pool < min_seg ? pool : min_seg;
        if (seg < least) seg = least;
    }
    G->seg = seg;
    G->spr = (pool + seg - 1) / seg;
    const uint64_t wl = g0 + nw - 1;
    G->q0 = g0 / pool * G->spr + g0 % pool / seg;
    G->n_pieces = wl / pool * G->spr + wl % pool / seg - G->q0 + 1;
    *grid = (G->n_pieces + pieces_per_group - 1) / pieces_per_group * G->n_slabs;
}

// What the lane group `slot` (0 ... pieces_per_group - 1) of workgroup `block` does: its column slab, its piece's row r = windows
// [row_a, row_b) of the range = pieces from row_q0, the windows [wa, wb) of the piece that lie in the batch (which ends at `end`; an
// inactive slot has none), and the slot through which the row leaves the workgroup: `lead` (<= slot), the first of the row's pieces
// here (the workgroup's pieces start at wg_q0).  Of that leader, asked once a lane knows that it is one, so that only leaders work them
// out: n_same, the count of the row's pieces here (slots lead ... lead + n_same - 1), and whole, whether the row is stored.
struct PieceLane {
    uint32_t slab, lead;
    bool active;
    uint64_t wg_q0, r, row_q0, row_a, row_b, end, wa, wb;
    QD_PIECES_HD uint32_t n_same(const PieceGeometry &P) const {
        uint64_t last = row_q0 + P.spr;
        last = last < wg_q0 + P.pieces_per_group ? last : wg_q0 + P.pieces_per_group;
        last = last < P.q0 + P.n_pieces ? last : P.q0 + P.n_pieces;
        return (uint32_t)(last - (wg_q0 + lead));
    }
    QD_PIECES_HD bool whole(const PieceGeometry &P) const {
        return row_q0 >= wg_q0 && row_q0 + P.spr <= wg_q0 + P.pieces_per_group && row_a >= P.g0 && row_b <= end;
    }
};
QD_PIECES_HD inline PieceLane piece_lane(const PieceGeometry &P, uint32_t block, uint32_t slot) {
    PieceLane l;
    l.slab = block % P.n_slabs;
    const uint64_t grp0 = (uint64_t)(block / P.n_slabs) * P.pieces_per_group;          // the workgroup's first piece, within the batch
    l.active = grp0 + slot < P.n_pieces;
    l.wg_q0 = P.q0 + grp0;
    const uint64_t q = l.wg_q0 + slot;
    l.r = q / P.spr;
    l.row_q0 = l.r * P.spr;
    const uint64_t k = q - l.row_q0;
    l.row_a = l.r * P.pool; l.row_b = l.row_a + P.pool < P.n_total ? l.row_a + P.pool : P.n_total;
    l.end = P.g0 + P.nw;
    uint64_t wa = l.row_a + k * P.seg, wb = wa + P.seg;
    wa = wa > P.g0 ? wa : P.g0;
    wb = wb < l.row_b ? wb : l.row_b;
    wb = wb < l.end ? wb : l.end;
    if (!l.active) wa = wb = P.g0;
    l.wa = wa; l.wb = wb;
    l.lead = l.row_q0 > l.wg_q0 ? (uint32_t)(l.row_q0 - l.wg_q0) : 0u;
    return l;
}

}  // namespace qd
