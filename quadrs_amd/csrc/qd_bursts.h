// qd_bursts.h — the burst list of norms rows (qd_plan_bursts): a threshold per bin turns every cell of the norms
// sink's windows on or off, and a burst is a maximal run of on cells in one bin.  The kernels here find the runs of a batch of windows,
// carry the open ones from batch to batch, count the bursts that end and store the first `cap` of them in the order of an event log:
// by last window, then bin.  qd_bursts_fold / qd_bursts_finish (quadrs_hip.hip) are the CPU twin and use the same functions.
//
// Every output is an integer count, an integer max or an index, so no batch, piece or launch order changes a byte.
//
// The first half of the header is the launch geometry as plain integer code: it compiles as C++17 on the host, where a program can walk
// every (workgroup, lane) of a launch (tests/test_bursts_cpu.py), and under hipcc, where the kernels take every index from it.
#ifndef QD_BURSTS_H
#define QD_BURSTS_H

#include <stdint.h>

#include "qd_lists.h"

#if defined(__HIPCC__)
#define QD_BURSTS_HD __host__ __device__
#else
#define QD_BURSTS_HD
#endif

namespace qd {

constexpr uint32_t kBurstsThreads = 256;
constexpr uint32_t kBurstsWaves = kBurstsThreads / 64;
static_assert(kBurstsThreads == kListThreads, "k_bursts_scan and k_bursts_close are rounds of qd_lists.h");
constexpr uint32_t kBurstsWords = 3;                     // QD_BURSTS_WORDS: first window of the open run or kBurstsNone, its peak_at, its peak bits
constexpr uint64_t kBurstsNone = ~0ull;
constexpr uint32_t kBurstsMasked = 0xffffffffu;          // the threshold word of a masked bin: above every |value|, so never on
constexpr uint32_t kBurstsInfBits = 0x7f800000u;
constexpr uint32_t kBurstsLdsWords = 2048;               // the LDS budget of k_bursts_emit: u64 ballot words, 16 KiB
constexpr uint64_t kBurstsMinSeg = 16;                   // a batch is not cut into pieces shorter than this
constexpr uint32_t kBurstsGroupsPerCu = 2;
constexpr uint64_t kBurstsMaxPieces = 8192;              // the stitch walks a batch's pieces in kBurstsStitchGroups sequential spans
constexpr uint64_t kBurstsMaxWorkspace = 1ull << 30;     // the list's workspace when the list is not device memory

struct Burst { uint64_t first, length, peak_at; uint32_t bin; uint32_t peak_bits; };      // qd_burst, 32 bytes

// ---- the cell rule, shared with the CPU twin
// the threshold word of a bin from the bits of its f32 threshold: false when the threshold is not admissible
QD_BURSTS_HD inline bool bursts_threshold(uint32_t bits, uint32_t *word) {
    if ((bits & 0x7fffffffu) > kBurstsInfBits) { *word = kBurstsMasked; return true; }       // a NaN of either sign masks the bin
    if (bits > kBurstsInfBits) return false;                                                 // the sign bit is set
    *word = bits;
    return true;
}
QD_BURSTS_HD inline uint32_t bursts_mag(uint32_t bits) { return bits & 0x7fffffffu; }
QD_BURSTS_HD inline bool bursts_on(uint32_t mag, uint32_t word) { return mag <= kBurstsInfBits && mag >= word; }

// the open run of a bin: first == kBurstsNone when none is open
struct BurstsRun { uint64_t first, peak_at; uint32_t peak; };
// one cell at window w into the run: on extends or opens it (the first window that attains the peak keeps it); off closes it.  Returns
// true when the cell ends a run, which *ended then holds.
QD_BURSTS_HD inline bool bursts_step(BurstsRun &r, uint64_t w, uint32_t mag, bool on, BurstsRun *ended) {
    if (on) {
        if (r.first == kBurstsNone) { r.first = w; r.peak_at = w; r.peak = mag; }
        else if (mag > r.peak) { r.peak = mag; r.peak_at = w; }
        return false;
    }
    if (r.first == kBurstsNone) return false;
    *ended = r;
    r.first = kBurstsNone;
    return true;
}

// Geometry of the launches over one batch: windows [g0, g0 + nw) of the range (g0 counts from the range's first window), W f32 each.
//   piece   `seg` consecutive windows of the batch: piece q covers [g0 + q seg, g0 + (q + 1) seg), the last one clipped to the batch.
//           Pieces belong to their batch alone; nothing depends on the range's length.
//   lanes   a lane owns a bin, so consecutive lanes read consecutive words of a row.  P lanes hold a piece: the smallest power of two
//           that holds min(W, 256) bins; ppg = 256 / P pieces share a workgroup, piece number `slot` of them on lanes slot P ... For
//           W < 64 several pieces share a wave, and a ballot word holds several pieces' lanes.  W > 256: the workgroup is one piece and
//           walks its columns in n_slabs slabs of 256 bins, one after the other (correct, not tuned).
//   split   seg = ceil(nw / want), want = min(n_cu kBurstsGroupsPerCu ppg, kBurstsMaxPieces) pieces, at least kBurstsMinSeg and at
//           most seg_max = kBurstsLdsWords / (4 n_slabs) windows: k_bursts_emit keeps one ballot word per (row, slab, wave) in LDS,
//           seg n_slabs 4 u64 words <= kBurstsLdsWords.
//   k_bursts_edge, k_bursts_emit<COUNT>, k_bursts_emit<EMIT>: grid = ceil(n_pieces / ppg) workgroups, every index from bursts_lane.
//   k_bursts_stitch: a workgroup takes kBurstsStitchBins bins and cuts the batch's pieces into kBurstsStitchGroups groups of consecutive
//           pieces, a lane for each (group, bin): ceil(W / kBurstsStitchBins) workgroups, every index from bursts_stitch_lane.
//   k_bursts_scan, k_bursts_close: one workgroup.
struct BurstsGeometry {
    uint64_t g0, nw, seg, n_pieces;
    uint32_t W, P, log2_P, ppg, n_slabs;
};

QD_BURSTS_HD inline uint32_t bursts_slabs(uint32_t W) { return W > kBurstsThreads ? (W + kBurstsThreads - 1) / kBurstsThreads : 1u; }
QD_BURSTS_HD inline uint64_t bursts_seg_max(uint32_t W) { return kBurstsLdsWords / (kBurstsWaves * bursts_slabs(W)); }      // 0: W is too wide
inline uint32_t bursts_lanes(uint32_t W) {
    uint32_t P = 1;
    while (P < kBurstsThreads && P < W) P *= 2;
    return P;
}
inline uint64_t bursts_want(uint32_t W, int n_cu) {
    const uint64_t want = (uint64_t)(n_cu > 0 ? n_cu : 1) * kBurstsGroupsPerCu * (kBurstsThreads / bursts_lanes(W));
    return want < kBurstsMaxPieces ? want : kBurstsMaxPieces;
}
// the most pieces a batch of at most nw_max windows is cut into: what the per-piece workspace is sized by
inline uint64_t bursts_pieces_bound(uint64_t nw_max, uint32_t W, int n_cu) {
    const uint64_t a = bursts_want(W, n_cu), sm = bursts_seg_max(W), b = (nw_max + sm - 1) / sm;
    return a > b ? a : b;
}
inline void bursts_split(uint64_t g0, uint64_t nw, uint32_t W, int n_cu, BurstsGeometry *G, uint64_t *grid) {
    G->g0 = g0; G->nw = nw; G->W = W;
    G->P = bursts_lanes(W);
    G->log2_P = 0;
    while ((1u << G->log2_P) < G->P) ++G->log2_P;
    G->ppg = kBurstsThreads / G->P;
    G->n_slabs = bursts_slabs(W);
    const uint64_t want = bursts_want(W, n_cu), seg_max = bursts_seg_max(W);
    uint64_t seg = (nw + want - 1) / want;
    if (seg < kBurstsMinSeg) seg = kBurstsMinSeg;
    if (seg > seg_max) seg = seg_max;
    G->seg = seg;
    G->n_pieces = (nw + seg - 1) / seg;
    *grid = (G->n_pieces + G->ppg - 1) / G->ppg;
}

// What lane `tid` of workgroup `block` does in k_bursts_edge and k_bursts_emit: its piece (within the batch) and the windows [wa, wb) of
// the range that the piece covers, its slot in the workgroup, and its bin in slab s: col0 + 256 s, which it owns when that is below W.
// An inactive lane has no piece: it reads and stores nothing, but walks the same seg rows so that a wave's ballots stay whole.
struct BurstsLane {
    bool active;
    uint32_t slot, col0;
    uint64_t piece, wa, wb;
};
QD_BURSTS_HD inline BurstsLane bursts_lane(const BurstsGeometry &G, uint32_t block, uint32_t tid) {
    BurstsLane l;
    l.slot = tid >> G.log2_P;
    l.col0 = tid & (G.P - 1);
    l.piece = (uint64_t)block * G.ppg + l.slot;
    l.active = l.piece < G.n_pieces;
    l.wa = G.g0 + l.piece * G.seg;
    l.wb = l.wa + G.seg < G.g0 + G.nw ? l.wa + G.seg : G.g0 + G.nw;
    if (!l.active) l.wa = l.wb = G.g0;
    return l;
}
QD_BURSTS_HD inline uint32_t bursts_col(const BurstsLane &l, uint32_t slab) { return l.col0 + slab * kBurstsThreads; }
// the ballot words of k_bursts_emit: where wave `wave` keeps row j of slab s, and which words and bits of a row are a lane's piece's
QD_BURSTS_HD inline uint32_t bursts_word(const BurstsGeometry &G, uint32_t j, uint32_t slab, uint32_t wave) { return (j * G.n_slabs + slab) * kBurstsWaves + wave; }
QD_BURSTS_HD inline uint32_t bursts_piece_waves(const BurstsGeometry &G) { return G.P > 64u ? G.P / 64u : 1u; }
QD_BURSTS_HD inline uint32_t bursts_piece_wave0(const BurstsGeometry &G, uint32_t tid) { return G.P > 64u ? (tid >> G.log2_P) * (G.P / 64u) : tid >> 6; }
QD_BURSTS_HD inline uint64_t bursts_piece_mask(const BurstsGeometry &G, uint32_t tid) {
    if (G.P >= 64u) return ~0ull;
    return ((1ull << G.P) - 1ull) << (((tid & 63u) >> G.log2_P) << G.log2_P);
}
// a piece's summary into the run that reaches the piece: a piece that is on throughout continues an open run (its peak wins only when
// greater: the earlier window keeps a tie), any other piece leaves its own tail.  A span of consecutive pieces summarises the same way
// (on throughout iff all of them are), so the rule also joins spans; (no run, on throughout) is the empty span.
QD_BURSTS_HD inline void bursts_join(BurstsRun &r, uint64_t first, uint64_t peak_at, uint32_t peak, bool all) {
    if (all && r.first != kBurstsNone) {
        if (peak > r.peak) { r.peak = peak; r.peak_at = peak_at; }
    } else {
        r.first = first; r.peak_at = peak_at; r.peak = peak;
    }
}
constexpr uint32_t kBurstsStitchGroups = 16, kBurstsStitchBins = 16;
struct BurstsStitchLane { bool active; uint32_t group, col; uint64_t q0, q1; };       // the lane's bin and its pieces [q0, q1) of the batch
QD_BURSTS_HD inline BurstsStitchLane bursts_stitch_lane(const BurstsGeometry &G, uint32_t block, uint32_t tid) {
    BurstsStitchLane l;
    l.group = tid / kBurstsStitchBins;
    l.col = block * kBurstsStitchBins + tid % kBurstsStitchBins;
    l.active = l.col < G.W;
    const uint64_t per = (G.n_pieces + kBurstsStitchGroups - 1) / kBurstsStitchGroups;
    l.q0 = l.group * per < G.n_pieces ? l.group * per : G.n_pieces;
    l.q1 = l.q0 + per < G.n_pieces ? l.q0 + per : G.n_pieces;
    return l;
}
// the per-piece words in the workspace: plane k (0 ... kBurstsWords - 1) of piece q, W words each, so lanes write consecutive words
QD_BURSTS_HD inline uint64_t bursts_slot_word(uint32_t W, uint64_t piece, uint32_t k, uint32_t col) { return (piece * kBurstsWords + k) * W + col; }

}  // namespace qd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace qd {

struct BurstsParams {
    const float *norms;                      // the batch's windows, nw x W
    const uint32_t *thr;                     // W threshold words (bursts_threshold)
    BurstsGeometry G;
    uint64_t min_len;
    unsigned long long *state;               // kBurstsWords planes of W: the open runs after the last batch
    unsigned long long *edge;                // per piece: the run that touches the piece's end, and bit 32 of word 2: every window is on
    unsigned long long *inc;                 // per piece: the open run that comes in
    ListCursor<Burst> L;                     // per piece: the bursts that end in it; the running count; the list (qd_lists.h)
    unsigned long long *on_counts;           // W words, or nullptr
    int vec_store;                           // the list is 16-byte aligned
};

__device__ inline void bursts_store(const BurstsParams &B, uint64_t rank, const BurstsRun &r, uint64_t end, uint32_t bin) {
    Burst *d = B.L.list + rank;
    const uint64_t len = end - r.first;
    if (B.vec_store) {
        uint4 *q = reinterpret_cast<uint4 *>(d);
        q[0] = make_uint4((uint32_t)r.first, (uint32_t)(r.first >> 32), (uint32_t)len, (uint32_t)(len >> 32));
        q[1] = make_uint4((uint32_t)r.peak_at, (uint32_t)(r.peak_at >> 32), bin, r.peak);
    } else {
        d->first = r.first; d->length = len; d->peak_at = r.peak_at; d->bin = bin; d->peak_bits = r.peak;
    }
}

// Phase 1: a lane walks its bin down its piece and leaves the piece's summary: the run that touches the piece's end and whether every
// window is on.  The piece's on cells go to on_counts by an integer atomic.
__global__ __launch_bounds__(kBurstsThreads) void k_bursts_edge(const BurstsParams B) {
    const BurstsGeometry &G = B.G;
    const BurstsLane l = bursts_lane(G, blockIdx.x, threadIdx.x);
    if (!l.active) return;
    for (uint32_t s = 0; s < G.n_slabs; ++s) {
        const uint32_t col = bursts_col(l, s);
        if (col >= G.W) break;
        const uint32_t t = B.thr[col];
        const float *p = B.norms + (l.wa - G.g0) * G.W + col;
        BurstsRun r{kBurstsNone, 0, 0}, e;
        uint64_t n_on = 0;
        bool all = true;
        for (uint64_t w = l.wa; w < l.wb; ++w, p += G.W) {
            const uint32_t a = bursts_mag(__float_as_uint(*p));
            const bool on = bursts_on(a, t);
            (void)bursts_step(r, w, a, on, &e);
            n_on += on; all = all && on;
        }
        B.edge[bursts_slot_word(G.W, l.piece, 0, col)] = r.first;
        B.edge[bursts_slot_word(G.W, l.piece, 1, col)] = r.peak_at;
        B.edge[bursts_slot_word(G.W, l.piece, 2, col)] = (unsigned long long)r.peak | (all ? 1ull << 32 : 0ull);
        if (B.on_counts && n_on) atomicAdd(&B.on_counts[col], (unsigned long long)n_on);
    }
}

// Phase 2: the carry.  The pieces' summaries join associatively (bursts_join), so the batch's pieces are cut into groups: a lane
// walks its bin down its group once for the group's summary, the groups meet in LDS, the lane joins the groups before its own onto
// the state the previous batch left (read by every lane before the barrier), and walks its group again, writing each piece's incoming
// run.  The last group's lane leaves the state after the batch's last window, behind the barrier: nobody reads what it writes.  The only sequential step: 2 n_pieces / kBurstsStitchGroups long, over small data.
__device__ inline void bursts_stitch_walk(const BurstsParams &B, const BurstsStitchLane &l, BurstsRun &r, bool *all, bool write) {
    const BurstsGeometry &G = B.G;
    const unsigned long long *__restrict__ edge = B.edge;
    unsigned long long *__restrict__ inc = B.inc;
    constexpr int U = 4;                                                    // pieces whose summaries are in flight
    for (uint64_t q0 = l.q0; q0 < l.q1; q0 += U) {
        unsigned long long f[U], at[U], pk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q0 + u < l.q1) {
                f[u] = edge[bursts_slot_word(G.W, q0 + u, 0, l.col)];
                at[u] = edge[bursts_slot_word(G.W, q0 + u, 1, l.col)];
                pk[u] = edge[bursts_slot_word(G.W, q0 + u, 2, l.col)];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q0 + u < l.q1) {
                if (write) {
                    inc[bursts_slot_word(G.W, q0 + u, 0, l.col)] = r.first;
                    inc[bursts_slot_word(G.W, q0 + u, 1, l.col)] = r.peak_at;
                    inc[bursts_slot_word(G.W, q0 + u, 2, l.col)] = r.peak;
                }
                const bool on = (pk[u] >> 32) != 0;
                bursts_join(r, f[u], at[u], (uint32_t)pk[u], on);
                *all = *all && on;
            }
        }
    }
}
__global__ __launch_bounds__(kBurstsThreads) void k_bursts_stitch(const BurstsParams B) {
    __shared__ unsigned long long s_first[kBurstsThreads], s_at[kBurstsThreads];
    __shared__ uint32_t s_peak[kBurstsThreads], s_all[kBurstsThreads];
    const BurstsGeometry &G = B.G;
    const uint32_t tid = threadIdx.x;
    const BurstsStitchLane l = bursts_stitch_lane(G, blockIdx.x, tid);
    BurstsRun r{kBurstsNone, 0, 0}, carried{kBurstsNone, 0, 0};
    bool all = true;
    if (l.active) {
        // every group's lane reads the carried state BEFORE the barrier; the last group's lane replaces it after the barrier
        carried = BurstsRun{B.state[l.col], B.state[G.W + l.col], (uint32_t)B.state[2ull * G.W + l.col]};
        bursts_stitch_walk(B, l, r, &all, false);
    }
    s_first[tid] = r.first; s_at[tid] = r.peak_at; s_peak[tid] = r.peak; s_all[tid] = all;
    __syncthreads();
    if (!l.active) return;
    r = carried;
    for (uint32_t g = 0; g < l.group; ++g) {
        const uint32_t o = g * kBurstsStitchBins + tid % kBurstsStitchBins;
        bursts_join(r, s_first[o], s_at[o], s_peak[o], s_all[o] != 0);
    }
    bursts_stitch_walk(B, l, r, &all, true);
    if (l.group == kBurstsStitchGroups - 1) { B.state[l.col] = r.first; B.state[G.W + l.col] = r.peak_at; B.state[2ull * G.W + l.col] = r.peak; }
}

// Phase 3: the same walker twice.  With its incoming run a lane sees a burst end at cell (w, bin) when the run is open and the cell is
// off; the burst's last window is w - 1.  COUNT leaves the piece's number of kept bursts.  EMIT first lays every row's ballot words into
// LDS (one barrier after the walk, none inside it), then walks again: a burst's rank is the piece's base, plus the ends in the earlier
// rows of the piece, plus the ends at lower bins of its row, both popcounts of those words.  A record is stored iff its rank < cap.
enum { kBurstsCount = 0, kBurstsEmit = 1 };
template <int MODE>
__global__ __launch_bounds__(kBurstsThreads) void k_bursts_emit(const BurstsParams B) {
    __shared__ unsigned long long s_bal[MODE == kBurstsEmit ? kBurstsLdsWords : 1];
    __shared__ uint32_t s_tot[kBurstsThreads];
    __shared__ uint32_t s_any;
    const BurstsGeometry &G = B.G;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const BurstsLane l = bursts_lane(G, blockIdx.x, tid);
    const uint32_t seg = (uint32_t)G.seg;
    bool work = l.active;
    uint64_t base = 0;
    if (MODE == kBurstsEmit) {
        if (tid == 0) s_any = 0;
        __syncthreads();
        if (work) work = list_piece_stores(B.L, l.piece, &base);
        if (work) s_any = 1;
        __syncthreads();
        if (!s_any) return;                                                 // workgroup-uniform
    } else {
        s_tot[tid] = 0;
        __syncthreads();
    }

    // the walk that finds the ends: all lanes run the same seg rows
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < G.n_slabs; ++s) {
        const uint32_t col = bursts_col(l, s);
        const bool ok = work && col < G.W;
        const uint32_t t = ok ? B.thr[col] : kBurstsMasked;
        uint64_t first = ok ? B.inc[bursts_slot_word(G.W, l.piece, 0, col)] : kBurstsNone;
        const float *p = B.norms + (ok ? (l.wa - G.g0) * G.W + col : 0);
        for (uint32_t j = 0; j < seg; ++j) {
            const uint64_t w = l.wa + j;
            bool end = false;
            if (ok && w < l.wb) {
                const uint32_t a = bursts_mag(__float_as_uint(*p));
                p += G.W;
                if (bursts_on(a, t)) {
                    if (first == kBurstsNone) first = w;
                } else if (first != kBurstsNone) {
                    end = w - first >= B.min_len;
                    first = kBurstsNone;
                }
            }
            if (MODE == kBurstsEmit) {
                const unsigned long long bal = __ballot(end);
                if ((tid & 63u) == 0) s_bal[bursts_word(G, j, s, wave)] = bal;
            } else {
                cnt += end;
            }
        }
    }
    if (MODE == kBurstsCount) {
        if (cnt) atomicAdd(&s_tot[l.slot], cnt);
        __syncthreads();
        if (tid < G.ppg && (uint64_t)blockIdx.x * G.ppg + tid < G.n_pieces) B.L.totals[(uint64_t)blockIdx.x * G.ppg + tid] = s_tot[tid];
        return;
    }
    __syncthreads();
    if (!work) return;

    // the walk that stores: the running rank of the row's first end, from the ballot words
    const uint32_t pw0 = bursts_piece_wave0(G, tid), pwn = bursts_piece_waves(G);
    const uint64_t pmask = bursts_piece_mask(G, tid);
    const uint64_t below_me = (1ull << (tid & 63u)) - 1ull;
    for (uint32_t s = 0; s < G.n_slabs; ++s) {
        const uint32_t col = bursts_col(l, s);
        if (col >= G.W) break;
        const uint32_t t = B.thr[col];
        BurstsRun r{B.inc[bursts_slot_word(G.W, l.piece, 0, col)], B.inc[bursts_slot_word(G.W, l.piece, 1, col)],
                    (uint32_t)B.inc[bursts_slot_word(G.W, l.piece, 2, col)]}, e;
        const float *p = B.norms + (l.wa - G.g0) * G.W + col;
        uint64_t rank0 = base;                                              // of the first end of row j
        for (uint32_t j = 0; l.wa + j < l.wb && rank0 < B.L.cap; ++j, p += G.W) {
            const uint64_t w = l.wa + j;
            const uint32_t a = bursts_mag(__float_as_uint(*p));
            if (bursts_step(r, w, a, bursts_on(a, t), &e) && w - e.first >= B.min_len) {
                uint64_t rank = rank0;
                for (uint32_t s2 = 0; s2 < s; ++s2)
                    for (uint32_t v = 0; v < pwn; ++v) rank += __popcll(s_bal[bursts_word(G, j, s2, pw0 + v)] & pmask);
                for (uint32_t v = pw0; v < wave; ++v) rank += __popcll(s_bal[bursts_word(G, j, s, v)] & pmask);
                rank += __popcll(s_bal[bursts_word(G, j, s, wave)] & pmask & below_me);
                if (rank < B.L.cap) bursts_store(B, rank, e, w, col);
            }
            for (uint32_t s2 = 0; s2 < G.n_slabs; ++s2)
                for (uint32_t v = 0; v < pwn; ++v) rank0 += __popcll(s_bal[bursts_word(G, j, s2, pw0 + v)] & pmask);
        }
    }
}

// between COUNT and EMIT: the pieces' totals into their bases, and the batch's bursts onto the running count (list_scan, qd_lists.h)
__global__ __launch_bounds__(kBurstsThreads) void k_bursts_scan(const BurstsParams B) { list_scan(B.L, B.G.n_pieces); }

// Phase 4, after the last batch: the runs still open close at the range's last folded window, by bin; `end` is the number of windows
// folded.  One workgroup walks the bins in slabs of 256; the state is left as before the first batch.
__global__ __launch_bounds__(kBurstsThreads) void k_bursts_close(const BurstsParams B, uint64_t end) {
    __shared__ unsigned long long s_bal[kBurstsWaves];
    const uint32_t tid = threadIdx.x, W = B.G.W;
    uint64_t rank0 = *B.L.found;
    __syncthreads();                                                        // everybody has read the count before anybody replaces it
    for (uint32_t c0 = 0; c0 < W; c0 += kBurstsThreads) {
        const uint32_t col = c0 + tid;
        BurstsRun r{kBurstsNone, 0, 0};
        if (col < W) {
            r.first = B.state[col]; r.peak_at = B.state[W + col]; r.peak = (uint32_t)B.state[2ull * W + col];
            B.state[col] = kBurstsNone; B.state[W + col] = 0; B.state[2ull * W + col] = 0;
        }
        const bool keep = r.first != kBurstsNone && end - r.first >= B.min_len;
        const uint64_t rank = list_round_rank(keep, s_bal, rank0);
        if (keep && rank < B.L.cap) bursts_store(B, rank, r, end, col);
        __syncthreads();                                                    // the next round replaces the words
    }
    if (tid == 0) *B.L.found = rank0;
}

}  // namespace qd
#endif  // __HIPCC__
#endif
