// qd_emissions.h — the emission list of norms rows (qd_plan_emissions): the per-bin thresholds of the burst list
// (qd_bursts.h) turn every cell of the norms sink's windows on or off, and an emission is a maximal 4-connected set of on cells in the
// (window, bin) plane.  The kernels here label the on cells of a span of windows, join the labels across tiles and onto the emissions
// the previous span left open, fold the cells into one record per emission, count the emissions that ended and store the first `cap` of
// them in the order of an event log: by last window, then by the lowest bin that is on in that window.  qd_emissions_fold /
// qd_emissions_finish (quadrs_hip.hip) are the CPU twin: emissions_twin_* below, row by row.
//
// Every output is an integer count, an integer extreme or an index, so no batch, span, tile or launch order changes a byte.
//
// The first half of the header is plain integer code: the record and its join, the twin, and the launch geometry.  It compiles as C++17
// on the host, where a program can walk every (workgroup, lane) of a launch (tests/test_emissions_cpu.py, scripts/emissions_host_check.cpp),
// and under hipcc, where the kernels take every index from it.
#ifndef QD_EMISSIONS_H
#define QD_EMISSIONS_H

#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "qd_bursts.h"

#if defined(__HIPCC__)
#define QD_EMISSIONS_HD __host__ __device__
#else
#define QD_EMISSIONS_HD
#endif

namespace qd {

constexpr uint32_t kEmissionsThreads = 256;
constexpr uint32_t kEmissionsWaves = kEmissionsThreads / 64;
static_assert(kEmissionsThreads == kListThreads, "k_emissions_scan, _emit and _close are rounds of qd_lists.h");
constexpr uint32_t kEmissionsWords = 8;                      // QD_EMISSIONS_WORDS: per bin one slot word and one 7-word record of the open table
constexpr uint64_t kEmissionsNone = ~0ull;
constexpr uint32_t kEmissionsOff = 0xffffffffu;              // the label of an off cell
constexpr uint32_t kEmissionsMaxWidth = 4096;                // W above this is QD_ERR_UNSUPPORTED
constexpr uint32_t kEmissionsTileCols = 256;                 // a tile is at most this many bins wide; even, so a pair of bins never straddles tiles
constexpr uint32_t kEmissionsTileCells = 2048;               // and holds at most this many cells ...
constexpr uint32_t kEmissionsTileSlots = 1024;               // ... and this many record slots (one per pair of bins of a row)
constexpr uint32_t kEmissionsLdsWords = kEmissionsTileCells + 7 * kEmissionsTileSlots;    // the LDS budget of k_emissions_tile: 36 KiB of u32
constexpr uint64_t kEmissionsSpanCells = 1ull << 20;         // a span holds at most this many cells (and at least one window)
constexpr uint32_t kEmissionsPieceCells = 2048;              // k_emissions_emit: consecutive cells of one workgroup
constexpr uint32_t kEmissionsRecWords = 8;                   // u64 planes of the record table
constexpr uint64_t kEmissionsMaxWorkspace = 1ull << 30;      // the list's workspace when the list is not device memory; the span's slots stay below it too
constexpr uint32_t kEmissionsCutFirst = 1u, kEmissionsCutLast = 2u;

struct Emission {                                            // qd_emission, 56 bytes
    uint64_t first, last, cells, peak_at;
    uint32_t lo, hi, end_bin, peak_bin, peak_bits, flags;
};

// ---- the record rule, shared with the CPU twin
// the partial record of one on cell
QD_EMISSIONS_HD inline Emission emissions_cell(uint64_t w, uint32_t bin, uint32_t mag) {
    return Emission{w, w, 1, w, bin, bin, bin, bin, mag, w == 0 ? kEmissionsCutFirst : 0u};
}
// b into a: associative and commutative.  The peak goes to the lexicographically smallest (window, bin) that attains it; end_bin is the
// lowest bin of the later last window.
QD_EMISSIONS_HD inline void emissions_join(Emission &a, const Emission &b) {
    if (b.last > a.last || (b.last == a.last && b.end_bin < a.end_bin)) a.end_bin = b.end_bin;
    if (b.peak_bits > a.peak_bits || (b.peak_bits == a.peak_bits && (b.peak_at < a.peak_at || (b.peak_at == a.peak_at && b.peak_bin < a.peak_bin)))) {
        a.peak_bits = b.peak_bits; a.peak_at = b.peak_at; a.peak_bin = b.peak_bin;
    }
    if (b.first < a.first) a.first = b.first;
    if (b.last > a.last) a.last = b.last;
    a.cells += b.cells;
    if (b.lo < a.lo) a.lo = b.lo;
    if (b.hi > a.hi) a.hi = b.hi;
    a.flags |= b.flags;
}
QD_EMISSIONS_HD inline bool emissions_kept(uint64_t first, uint64_t last, uint64_t cells, uint64_t min_len, uint64_t min_cells) {
    return last - first + 1 >= min_len && cells >= min_cells;
}

// ---- the CPU twin.  state: [W slot words: the open emission of the bin in the previous row, or kEmissionsNone][W records of 7 words:
// the open table][next window][open records].  A row has at most ceil(W / 2) open emissions.
struct EmissionsSink { Emission *list; uint64_t cap; uint64_t *found; uint64_t min_len, min_cells; };
inline void emissions_twin_emit(const EmissionsSink &k, const Emission &e) {
    if (!emissions_kept(e.first, e.last, e.cells, k.min_len, k.min_cells)) return;
    if (*k.found < k.cap) k.list[*k.found] = e;
    *k.found += 1;
}
inline Emission *emissions_twin_table(uint64_t *state, uint32_t W) { return reinterpret_cast<Emission *>(state + W); }
inline void emissions_twin_init(uint64_t *state, uint32_t W) {
    for (uint32_t b = 0; b < W; ++b) state[b] = kEmissionsNone;
    for (size_t i = W; i < (size_t)kEmissionsWords * W + 2; ++i) state[i] = 0;
}
// one row, window w: `thr` are the W threshold words.  Nodes 0 ... W-1 are the open slots, W + a the run of on cells that starts at bin a.
inline void emissions_twin_row(uint64_t *state, uint32_t W, const uint32_t *thr, uint64_t w, const uint32_t *row_bits, const EmissionsSink &k) {
    Emission *table = emissions_twin_table(state, W);
    std::vector<uint32_t> parent(2 * (size_t)W), run_of(W, kEmissionsOff);
    std::vector<Emission> run(W);
    for (uint32_t i = 0; i < 2 * W; ++i) parent[i] = i;
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (uint32_t b = 0; b < W; ++b) {
        const uint32_t a = bursts_mag(row_bits[b]);
        if (!bursts_on(a, thr[b])) continue;
        const Emission c = emissions_cell(w, b, a);
        if (b && run_of[b - 1] != kEmissionsOff) { run_of[b] = run_of[b - 1]; emissions_join(run[run_of[b]], c); }
        else { run_of[b] = b; run[b] = c; }
        if (state[b] != kEmissionsNone) {                                  // the larger root wins, so a class with a run is rooted at a run
            const uint32_t x = find((uint32_t)state[b]), y = find(W + run_of[b]);
            if (x != y) parent[x < y ? x : y] = x < y ? y : x;
        }
    }
    // the open emissions without an on neighbour in this row have ended: by their lowest bin in the previous row
    std::vector<uint8_t> seen(W, 0);
    for (uint32_t b = 0; b < W; ++b) {
        if (state[b] == kEmissionsNone || seen[state[b]]) continue;
        seen[state[b]] = 1;
        if (find((uint32_t)state[b]) < W) emissions_twin_emit(k, table[state[b]]);
    }
    // the others join their class's runs; the new table is numbered by the class's lowest bin in this row
    std::vector<Emission> next;
    std::vector<uint32_t> slot_of(2 * (size_t)W, kEmissionsOff);
    for (uint32_t b = 0; b < W; ++b) {
        if (run_of[b] != b) continue;
        const uint32_t root = find(W + b);
        if (slot_of[root] == kEmissionsOff) { slot_of[root] = (uint32_t)next.size(); next.push_back(run[b]); }
        else emissions_join(next[slot_of[root]], run[b]);
    }
    for (uint32_t s = 0; s < W; ++s) {
        if (!seen[s]) continue;
        const uint32_t root = find(s);
        if (root >= W) emissions_join(next[slot_of[root]], table[s]);
    }
    for (uint32_t b = 0; b < W; ++b) state[b] = run_of[b] == kEmissionsOff ? kEmissionsNone : slot_of[find(W + run_of[b])];
    for (size_t s = 0; s < next.size(); ++s) table[s] = next[s];
    state[(size_t)kEmissionsWords * W + 1] = next.size();
}
// what is open closes at the last window folded, cut there, in the same order
inline void emissions_twin_finish(uint64_t *state, uint32_t W, const EmissionsSink &k) {
    Emission *table = emissions_twin_table(state, W);
    std::vector<uint8_t> seen(W, 0);
    for (uint32_t b = 0; b < W; ++b) {
        if (state[b] == kEmissionsNone || seen[state[b]]) continue;
        seen[state[b]] = 1;
        Emission e = table[state[b]];
        e.flags |= kEmissionsCutLast;
        emissions_twin_emit(k, e);
    }
    emissions_twin_init(state, W);
}

// ---- the geometry of the launches over one span: S >= 1 windows [w0, w0 + S) of the range, W bins each.
//   plane   (S + 1) rows of W u32 labels.  Row 0 is the virtual row: the last row of the previous span (of this or the previous batch),
//           whose on cells carry the emissions still open; rows 1 ... S are the span's windows.  Cell (r, b) has the index
//           r W + (W - 1 - b): row ascending, bin reversed, so the greatest index of a component is the cell (last, end_bin) of the
//           definition.  A label is a cell index of the same component that is not smaller (max-root); a cell is a root iff its label is
//           its own index, iff its component ends there.
//   slot    a pair of bins (2h, 2h + 1) of one row: r H + h, H = ceil(W / 2).  Two on cells of a pair are neighbours, so at most one cell
//           of a pair is a root, of its tile or of the plane, and the slot holds its record without a compaction: kEmissionsRecWords
//           planes of `ns` u64 (the slots of the longest span), 0 first, 1 last, 2 cells, 3 lo | hi << 32, 4 peak | flags << 32,
//           5 the peak's position window W + bin, 6 the slot's own root cell << 32 | own peak (~0: no tile-local root here), 7 the own
//           peak's position.  Planes 0 ... 5 of a root take its whole emission; 6 and 7 stay what the tile left.
//   tile    tr rows x at most 256 bins, tr = 2048 / (2 ceil(min(W, 256) / 2)): at most 2048 cells and 1024 slots.  Workgroup
//           t_row n_tcols + t_col of k_emissions_tile; lane tid takes cells tid, tid + 256, ... of the tile in row-major order.
//   link    one lane per cell of a border: the row above every tile row (n_trows W lanes; tile row 0 borders the virtual row), then the
//           column left of every tile column but the first (S lanes each).
//   slots   k_emissions_fold, k_emissions_peak: one lane per slot of rows 0 ... S.  k_emissions_carry: one lane per bin.
//   pieces  k_emissions_emit: rows 0 ... S - 1 (the roots there have ended; those of row S are open) as S W cells in the list's order,
//           row-major with the bin ascending, cut into pieces of 2048 cells, one workgroup each.
struct EmissionsGeometry {
    uint64_t w0, ns;
    uint32_t S, W, H, tr, n_trows, n_tcols, n_pieces;
};
QD_EMISSIONS_HD inline uint64_t emissions_span(uint32_t W) { const uint64_t s = kEmissionsSpanCells / W; return s ? s : 1; }
QD_EMISSIONS_HD inline uint32_t emissions_half(uint32_t W) { return (W + 1) / 2; }
QD_EMISSIONS_HD inline uint32_t emissions_tile_rows(uint32_t W) {
    const uint32_t tc = W < kEmissionsTileCols ? W : kEmissionsTileCols;
    return kEmissionsTileCells / (2 * emissions_half(tc));
}
// the workspace of the longest span of a call whose batches hold at most nw_max windows: the plane, the record table, the pieces
inline uint64_t emissions_span_max(uint32_t W, uint64_t nw_max) { const uint64_t s = emissions_span(W); return nw_max < s ? (nw_max ? nw_max : 1) : s; }
inline uint64_t emissions_plane_bytes(uint32_t W, uint64_t span_max) { return (span_max + 1) * W * 4; }
inline uint64_t emissions_slots(uint32_t W, uint64_t span_max) { return (span_max + 1) * emissions_half(W); }
inline uint64_t emissions_pieces_bound(uint32_t W, uint64_t span_max) { return (span_max * W + kEmissionsPieceCells - 1) / kEmissionsPieceCells; }
inline uint64_t emissions_workspace(uint32_t W, uint64_t span_max) {
    return emissions_plane_bytes(W, span_max) + emissions_slots(W, span_max) * kEmissionsRecWords * 8 + emissions_pieces_bound(W, span_max) * 16;
}
inline void emissions_split(uint64_t w0, uint64_t S, uint32_t W, uint64_t span_max, EmissionsGeometry *G) {
    G->w0 = w0; G->S = (uint32_t)S; G->W = W; G->H = emissions_half(W);
    G->ns = emissions_slots(W, span_max);
    G->tr = emissions_tile_rows(W);
    G->n_trows = (uint32_t)((S + G->tr - 1) / G->tr);
    G->n_tcols = (W + kEmissionsTileCols - 1) / kEmissionsTileCols;
    G->n_pieces = (uint32_t)((S * W + kEmissionsPieceCells - 1) / kEmissionsPieceCells);
}
QD_EMISSIONS_HD inline uint32_t emissions_index(const EmissionsGeometry &G, uint32_t r, uint32_t b) { return r * G.W + (G.W - 1 - b); }
QD_EMISSIONS_HD inline uint32_t emissions_row(const EmissionsGeometry &G, uint32_t cell) { return cell / G.W; }
QD_EMISSIONS_HD inline uint32_t emissions_bin(const EmissionsGeometry &G, uint32_t cell) { return G.W - 1 - cell % G.W; }
QD_EMISSIONS_HD inline uint64_t emissions_slot(const EmissionsGeometry &G, uint32_t r, uint32_t b) { return (uint64_t)r * G.H + b / 2; }
QD_EMISSIONS_HD inline uint64_t emissions_slot_of(const EmissionsGeometry &G, uint32_t cell) { return emissions_slot(G, emissions_row(G, cell), emissions_bin(G, cell)); }
QD_EMISSIONS_HD inline uint64_t emissions_window(const EmissionsGeometry &G, uint32_t r) { return G.w0 + r - 1; }       // r >= 1

struct EmissionsTile { uint32_t r0, nr, b0, nc, hc; };       // plane rows [r0, r0 + nr), bins [b0, b0 + nc), hc slots per row
QD_EMISSIONS_HD inline EmissionsTile emissions_tile(const EmissionsGeometry &G, uint32_t block) {
    EmissionsTile T;
    const uint32_t trow = block / G.n_tcols, tcol = block % G.n_tcols;
    T.r0 = 1 + trow * G.tr;
    T.nr = G.S - trow * G.tr < G.tr ? G.S - trow * G.tr : G.tr;
    T.b0 = tcol * kEmissionsTileCols;
    T.nc = G.W - T.b0 < kEmissionsTileCols ? G.W - T.b0 : kEmissionsTileCols;
    T.hc = emissions_half(T.nc);
    return T;
}
// The cells of a lane, one function for every cell phase.  k_emissions_tile: cell number k (0 ... 7) of lane tid of a tile, (lr, lb) within
// the tile, li its index in the tile's LDS labels, ordered like the plane's: row ascending, bin reversed.
struct EmissionsCell { bool valid; uint32_t lr, lb, li; };
QD_EMISSIONS_HD inline EmissionsCell emissions_tile_cell(const EmissionsTile &T, uint32_t tid, uint32_t k) {
    EmissionsCell c;
    const uint32_t i = tid + k * kEmissionsThreads;
    c.valid = i < T.nr * T.nc;
    c.lr = i / T.nc; c.lb = i % T.nc;
    c.li = c.lr * T.nc + (T.nc - 1 - c.lb);
    return c;
}
QD_EMISSIONS_HD inline uint32_t emissions_tile_slot(const EmissionsTile &T, uint32_t li) { return (li / T.nc) * T.hc + (T.nc - 1 - li % T.nc) / 2; }
// k_emissions_link: lane i joins cells (ra, ba) and (rb, bb) when both are on; (rp, bp_a, bp_b) is the pair before it along the border
// within the same tiles, or has_prev is false: when all four are on, the earlier pair has made the same join.
struct EmissionsLink { bool valid, has_prev; uint32_t ra, ba, rb, bb, pra, pba, prb, pbb; };
QD_EMISSIONS_HD inline uint64_t emissions_link_lanes(const EmissionsGeometry &G) { return (uint64_t)G.n_trows * G.W + (uint64_t)(G.n_tcols - 1) * G.S; }
QD_EMISSIONS_HD inline EmissionsLink emissions_link(const EmissionsGeometry &G, uint64_t i) {
    EmissionsLink l{};
    const uint64_t n_h = (uint64_t)G.n_trows * G.W;
    l.valid = i < emissions_link_lanes(G);
    if (!l.valid) return l;
    if (i < n_h) {
        const uint32_t t = (uint32_t)(i / G.W), b = (uint32_t)(i % G.W);
        l.ra = t * G.tr; l.rb = l.ra + 1; l.ba = l.bb = b;
        l.has_prev = b % kEmissionsTileCols != 0;
        l.pra = l.ra; l.prb = l.rb; l.pba = l.pbb = b - 1;
    } else {
        const uint64_t j = i - n_h;
        const uint32_t v = (uint32_t)(j / G.S), r = 1 + (uint32_t)(j % G.S);
        l.ra = l.rb = r; l.bb = (v + 1) * kEmissionsTileCols; l.ba = l.bb - 1;
        l.has_prev = (r - 1) % G.tr != 0;
        l.pra = l.prb = r - 1; l.pba = l.ba; l.pbb = l.bb;
    }
    return l;
}
// k_emissions_emit: cell number `it` of lane tid of piece q, in the list's order
QD_EMISSIONS_HD inline bool emissions_piece_cell(const EmissionsGeometry &G, uint32_t q, uint32_t it, uint32_t tid, uint32_t *r, uint32_t *b) {
    const uint64_t n = (uint64_t)q * kEmissionsPieceCells + it * kEmissionsThreads + tid;
    if (n >= (uint64_t)G.S * G.W) return false;
    *r = (uint32_t)(n / G.W); *b = (uint32_t)(n % G.W);
    return true;
}

}  // namespace qd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace qd {

struct EmissionsParams {
    const float *norms;                      // the span's windows, S x W
    const uint32_t *thr;                     // W threshold words (bursts_threshold)
    EmissionsGeometry G;
    uint64_t min_len, min_cells;
    uint32_t *plane;                         // (span_max + 1) W labels
    unsigned long long *rec;                 // kEmissionsRecWords planes of G.ns
    ListCursor<Emission> L;                  // per piece: the emissions that end in it; the running count; the list (qd_lists.h)
};
enum { kEmFirst = 0, kEmLast, kEmCells, kEmLoHi, kEmPeakFlags, kEmPos, kEmOwn, kEmOwnPos };

__device__ inline unsigned long long *emissions_rec(const EmissionsParams &E, uint32_t plane, uint64_t slot) { return E.rec + (uint64_t)plane * E.G.ns + slot; }

// Labels move one way only: a label is replaced by a greater one of the same component, by atomicMax or by a store of an ancestor, so
// every walk ends at the plane's greatest index at the latest, and nobody waits for anybody.
template <typename T>
__device__ inline uint32_t emissions_find(T *L, uint32_t x) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}
template <typename T>
__device__ inline void emissions_union(T *L, uint32_t a, uint32_t b) {
    for (;;) {
        a = emissions_find(L, a); b = emissions_find(L, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMax(&L[a], b);             // a < b: a root a now hangs under b
        if (old == a) return;
        a = old;                                              // a had a parent already, greater than a: go on from there
    }
}

// Phase 1: a tile's labels and tile-local records, in LDS.
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_tile(const EmissionsParams E) {
    __shared__ uint32_t s_lab[kEmissionsTileCells];
    __shared__ uint32_t s_first[kEmissionsTileSlots], s_last[kEmissionsTileSlots], s_cells[kEmissionsTileSlots], s_lo[kEmissionsTileSlots],
        s_hi[kEmissionsTileSlots], s_peak[kEmissionsTileSlots], s_pos[kEmissionsTileSlots];
    const EmissionsGeometry &G = E.G;
    const uint32_t tid = threadIdx.x;
    const EmissionsTile T = emissions_tile(G, blockIdx.x);
    constexpr uint32_t K = kEmissionsTileCells / kEmissionsThreads;
    for (uint32_t k = 0; k < K; ++k) {
        const EmissionsCell c = emissions_tile_cell(T, tid, k);
        if (!c.valid) break;
        const uint32_t b = T.b0 + c.lb;
        const uint32_t a = bursts_mag(__float_as_uint(E.norms[(uint64_t)(T.r0 + c.lr - 1) * G.W + b]));
        s_lab[c.li] = bursts_on(a, E.thr[b]) ? c.li : kEmissionsOff;
    }
    for (uint32_t s = tid; s < T.nr * T.hc; s += kEmissionsThreads) {
        s_first[s] = 0xffffffffu; s_last[s] = 0; s_cells[s] = 0; s_lo[s] = 0xffffffffu; s_hi[s] = 0; s_peak[s] = 0; s_pos[s] = 0xffffffffu;
    }
    __syncthreads();
    // local union along rows and columns: the next bin is the index below, the next row nc above
    for (uint32_t k = 0; k < K; ++k) {
        const EmissionsCell c = emissions_tile_cell(T, tid, k);
        if (!c.valid) break;
        if (s_lab[c.li] == kEmissionsOff) continue;
        if (c.lb + 1 < T.nc && s_lab[c.li - 1] != kEmissionsOff) emissions_union(s_lab, c.li, c.li - 1);
        if (c.lr + 1 < T.nr && s_lab[c.li + T.nc] != kEmissionsOff) emissions_union(s_lab, c.li, c.li + T.nc);
    }
    __syncthreads();
    for (uint32_t k = 0; k < K; ++k) {
        const EmissionsCell c = emissions_tile_cell(T, tid, k);
        if (!c.valid) break;
        if (s_lab[c.li] != kEmissionsOff) s_lab[c.li] = emissions_find(s_lab, c.li);
    }
    __syncthreads();
    // the cells into their root's slot: integer LDS atomics
    for (uint32_t k = 0; k < K; ++k) {
        const EmissionsCell c = emissions_tile_cell(T, tid, k);
        if (!c.valid) break;
        const uint32_t root = s_lab[c.li];
        if (root == kEmissionsOff) continue;
        const uint32_t s = emissions_tile_slot(T, root);
        const uint32_t a = bursts_mag(__float_as_uint(E.norms[(uint64_t)(T.r0 + c.lr - 1) * G.W + T.b0 + c.lb]));
        atomicMin(&s_first[s], c.lr); atomicMax(&s_last[s], c.lr); atomicAdd(&s_cells[s], 1u);
        atomicMin(&s_lo[s], c.lb); atomicMax(&s_hi[s], c.lb); atomicMax(&s_peak[s], a);
    }
    __syncthreads();
    for (uint32_t k = 0; k < K; ++k) {
        const EmissionsCell c = emissions_tile_cell(T, tid, k);
        if (!c.valid) break;
        const uint32_t root = s_lab[c.li];
        if (root == kEmissionsOff) continue;
        const uint32_t s = emissions_tile_slot(T, root);
        const uint32_t a = bursts_mag(__float_as_uint(E.norms[(uint64_t)(T.r0 + c.lr - 1) * G.W + T.b0 + c.lb]));
        if (a == s_peak[s]) atomicMin(&s_pos[s], c.lr * T.nc + c.lb);
    }
    __syncthreads();
    // the label plane: the plane's index of the local root
    for (uint32_t k = 0; k < K; ++k) {
        const EmissionsCell c = emissions_tile_cell(T, tid, k);
        if (!c.valid) break;
        const uint32_t root = s_lab[c.li];
        E.plane[emissions_index(G, T.r0 + c.lr, T.b0 + c.lb)] =
            root == kEmissionsOff ? kEmissionsOff : emissions_index(G, T.r0 + root / T.nc, T.b0 + (T.nc - 1 - root % T.nc));
    }
    // the tile's records: every slot's own word, and the rest where a local root stands
    for (uint32_t s = tid; s < T.nr * T.hc; s += kEmissionsThreads) {
        const uint32_t lr = s / T.hc, lb0 = 2 * (s % T.hc);
        const uint32_t li0 = lr * T.nc + (T.nc - 1 - lb0);
        uint32_t lb = 0xffffffffu;
        if (s_lab[li0] == li0) lb = lb0;
        else if (lb0 + 1 < T.nc && s_lab[li0 - 1] == li0 - 1) lb = lb0 + 1;
        const uint64_t slot = emissions_slot(G, T.r0 + lr, T.b0 + lb0);
        if (lb == 0xffffffffu) { *emissions_rec(E, kEmOwn, slot) = kEmissionsNone; continue; }
        const uint64_t first = emissions_window(G, T.r0 + s_first[s]);
        *emissions_rec(E, kEmFirst, slot) = first;
        *emissions_rec(E, kEmLast, slot) = emissions_window(G, T.r0 + s_last[s]);
        *emissions_rec(E, kEmCells, slot) = s_cells[s];
        *emissions_rec(E, kEmLoHi, slot) = (unsigned long long)(T.b0 + s_lo[s]) | (unsigned long long)(T.b0 + s_hi[s]) << 32;
        *emissions_rec(E, kEmPeakFlags, slot) = (unsigned long long)s_peak[s] | (unsigned long long)(first == 0 ? kEmissionsCutFirst : 0u) << 32;
        *emissions_rec(E, kEmPos, slot) = kEmissionsNone;
        *emissions_rec(E, kEmOwn, slot) = (unsigned long long)emissions_index(G, T.r0 + lr, T.b0 + lb) << 32 | s_peak[s];
        *emissions_rec(E, kEmOwnPos, slot) = emissions_window(G, T.r0 + s_pos[s] / T.nc) * G.W + T.b0 + s_pos[s] % T.nc;
    }
}

// Phase 2: union across the tile borders and with the virtual row, on the plane.
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_link(const EmissionsParams E) {
    const EmissionsGeometry &G = E.G;
    const EmissionsLink l = emissions_link(G, (uint64_t)blockIdx.x * kEmissionsThreads + threadIdx.x);
    if (!l.valid) return;
    const uint32_t a = emissions_index(G, l.ra, l.ba), b = emissions_index(G, l.rb, l.bb);
    // whether a cell is on never changes, so these reads need no order
    if (E.plane[a] == kEmissionsOff || E.plane[b] == kEmissionsOff) return;
    if (l.has_prev && E.plane[emissions_index(G, l.pra, l.pba)] != kEmissionsOff && E.plane[emissions_index(G, l.prb, l.pbb)] != kEmissionsOff) return;
    emissions_union(E.plane, a, b);
}

// Phase 3a: every tile-local record (and every carried one, in row 0) that is not its emission's root joins the root's record: one set
// of integer atomics per tile-local component, none per cell.  The record's cell is pointed at the root.
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_fold(const EmissionsParams E) {
    const EmissionsGeometry &G = E.G;
    const uint64_t s = (uint64_t)blockIdx.x * kEmissionsThreads + threadIdx.x;
    if (s >= (uint64_t)(G.S + 1) * G.H) return;
    const unsigned long long own = *emissions_rec(E, kEmOwn, s);
    if (own == kEmissionsNone) return;
    const uint32_t cell = (uint32_t)(own >> 32);
    const uint32_t root = emissions_find(E.plane, cell);
    if (root == cell) return;
    E.plane[cell] = root;
    const uint64_t t = emissions_slot_of(G, root);
    atomicMin(emissions_rec(E, kEmFirst, t), *emissions_rec(E, kEmFirst, s));
    atomicMax(emissions_rec(E, kEmLast, t), *emissions_rec(E, kEmLast, s));
    atomicAdd(emissions_rec(E, kEmCells, t), *emissions_rec(E, kEmCells, s));
    const unsigned long long lohi = *emissions_rec(E, kEmLoHi, s), pf = *emissions_rec(E, kEmPeakFlags, s);
    uint32_t *lh = reinterpret_cast<uint32_t *>(emissions_rec(E, kEmLoHi, t)), *pk = reinterpret_cast<uint32_t *>(emissions_rec(E, kEmPeakFlags, t));
    atomicMin(lh, (uint32_t)lohi); atomicMax(lh + 1, (uint32_t)(lohi >> 32));
    atomicMax(pk, (uint32_t)pf);
    if (pf >> 32) atomicOr(pk + 1, (uint32_t)(pf >> 32));
}
// Phase 3b: the peak's place, among the records that attain the emission's peak
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_peak(const EmissionsParams E) {
    const EmissionsGeometry &G = E.G;
    const uint64_t s = (uint64_t)blockIdx.x * kEmissionsThreads + threadIdx.x;
    if (s >= (uint64_t)(G.S + 1) * G.H) return;
    const unsigned long long own = *emissions_rec(E, kEmOwn, s);
    if (own == kEmissionsNone) return;
    const uint64_t t = emissions_slot_of(G, E.plane[(uint32_t)(own >> 32)]);
    if ((uint32_t)own == (uint32_t)*emissions_rec(E, kEmPeakFlags, t)) atomicMin(emissions_rec(E, kEmPos, t), *emissions_rec(E, kEmOwnPos, s));
}

__device__ inline void emissions_store(const EmissionsParams &E, uint64_t rank, uint64_t slot, uint32_t end_bin, uint32_t more_flags) {
    unsigned long long *d = reinterpret_cast<unsigned long long *>(E.L.list + rank);
    const unsigned long long lohi = *emissions_rec(E, kEmLoHi, slot), pf = *emissions_rec(E, kEmPeakFlags, slot), pos = *emissions_rec(E, kEmPos, slot);
    d[0] = *emissions_rec(E, kEmFirst, slot);
    d[1] = *emissions_rec(E, kEmLast, slot);
    d[2] = *emissions_rec(E, kEmCells, slot);
    d[3] = pos / E.G.W;
    d[4] = lohi;
    d[5] = (unsigned long long)end_bin | (unsigned long long)(uint32_t)(pos % E.G.W) << 32;
    d[6] = pf | (unsigned long long)more_flags << 32;
}
__device__ inline bool emissions_slot_kept(const EmissionsParams &E, uint64_t slot) {
    return emissions_kept(*emissions_rec(E, kEmFirst, slot), *emissions_rec(E, kEmLast, slot), *emissions_rec(E, kEmCells, slot), E.min_len, E.min_cells);
}

// Phase 4: the roots above the span's last row have ended.  COUNT leaves the piece's number of kept ones; EMIT ranks them by ballot and
// popcount from the piece's base, in the list's order, and stores those whose rank is below cap.
enum { kEmissionsCount = 0, kEmissionsEmit = 1 };
template <int MODE>
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_emit(const EmissionsParams E) {
    __shared__ unsigned long long s_bal[2][kEmissionsWaves];
    __shared__ uint32_t s_tot;
    const EmissionsGeometry &G = E.G;
    const uint32_t tid = threadIdx.x, q = blockIdx.x;
    uint64_t rank0 = 0;
    if (MODE == kEmissionsEmit) {
        if (!list_piece_stores(E.L, q, &rank0)) return;                     // workgroup-uniform
    } else {
        if (tid == 0) s_tot = 0;
        __syncthreads();
    }
    uint32_t cnt = 0;
#pragma unroll(MODE == kEmissionsEmit ? kEmissionsPieceCells / kEmissionsThreads : 2)      // the forms the compiler chose for the parent's text (section 3.26)
    for (uint32_t it = 0; it < kEmissionsPieceCells / kEmissionsThreads; ++it) {
        uint32_t r = 0, b = 0;
        bool keep = false;
        uint64_t slot = 0;
        if (emissions_piece_cell(G, q, it, tid, &r, &b)) {
            const uint32_t c = emissions_index(G, r, b);
            if (E.plane[c] == c) { slot = emissions_slot(G, r, b); keep = emissions_slot_kept(E, slot); }
        }
        if (MODE == kEmissionsCount) { cnt += keep; continue; }
        const uint64_t rank = list_round_rank(keep, s_bal[it & 1], rank0);  // two sets of words: the next round writes the other one
        if (keep && rank < E.L.cap) emissions_store(E, rank, slot, b, 0);
    }
    if (MODE == kEmissionsCount) {
        if (cnt) atomicAdd(&s_tot, cnt);
        __syncthreads();
        if (tid == 0) E.L.totals[q] = s_tot;
    }
}

// between COUNT and EMIT: the pieces' totals into their bases, and the span's emissions onto the running count (list_scan, qd_lists.h)
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_scan(const EmissionsParams E) { list_scan(E.L, E.G.n_pieces); }

// The seam, of spans and of batches alike: the span's last row becomes the next span's virtual row.  A cell of the last row has its
// root there; a root's record moves to row 0 with its emission's peak as its own.
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_carry(const EmissionsParams E) {
    const EmissionsGeometry &G = E.G;
    const uint32_t i = blockIdx.x * kEmissionsThreads + threadIdx.x;
    const uint32_t down = G.S * G.W;
    if (i < G.W) {
        const uint32_t c = emissions_index(G, G.S, i);
        E.plane[emissions_index(G, 0, i)] = E.plane[c] == kEmissionsOff ? kEmissionsOff : emissions_find(E.plane, c) - down;
    }
    if (i < G.H) {
        const uint64_t s = (uint64_t)G.S * G.H + i;
        const unsigned long long own = *emissions_rec(E, kEmOwn, s);
        const uint32_t cell = (uint32_t)(own >> 32);
        if (own == kEmissionsNone || E.plane[cell] != cell) { *emissions_rec(E, kEmOwn, i) = kEmissionsNone; return; }
        for (uint32_t k = kEmFirst; k <= kEmPeakFlags; ++k) *emissions_rec(E, k, i) = *emissions_rec(E, k, s);
        *emissions_rec(E, kEmPos, i) = kEmissionsNone;
        *emissions_rec(E, kEmOwn, i) = (unsigned long long)(cell - down) << 32 | (uint32_t)*emissions_rec(E, kEmPeakFlags, s);
        *emissions_rec(E, kEmOwnPos, i) = *emissions_rec(E, kEmPos, s);
    }
}

// Phase 5, after the last batch: what the virtual row holds closes at the range's last folded window, cut there, by bin.  One workgroup
// walks the bins in slabs of 256.
__global__ __launch_bounds__(kEmissionsThreads) void k_emissions_close(const EmissionsParams E) {
    __shared__ unsigned long long s_bal[kEmissionsWaves];
    const EmissionsGeometry &G = E.G;
    const uint32_t tid = threadIdx.x;
    uint64_t rank0 = *E.L.found;
    __syncthreads();                                                        // everybody has read the count before anybody replaces it
    for (uint32_t c0 = 0; c0 < G.W; c0 += kEmissionsThreads) {
        const uint32_t b = c0 + tid;
        bool keep = false;
        if (b < G.W && E.plane[emissions_index(G, 0, b)] == emissions_index(G, 0, b)) keep = emissions_slot_kept(E, emissions_slot(G, 0, b));
        const uint64_t rank = list_round_rank(keep, s_bal, rank0);
        if (keep && rank < E.L.cap) {
            // the carried record holds its emission's peak as its own: nothing has joined it since
            *emissions_rec(E, kEmPos, emissions_slot(G, 0, b)) = *emissions_rec(E, kEmOwnPos, emissions_slot(G, 0, b));
            emissions_store(E, rank, emissions_slot(G, 0, b), b, kEmissionsCutLast);
        }
        __syncthreads();                                                    // the next round replaces the words
    }
    if (tid == 0) *E.L.found = rank0;
}

}  // namespace qd
#endif  // __HIPCC__
#endif
