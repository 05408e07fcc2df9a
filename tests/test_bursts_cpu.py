"""The burst list's host half (include/quadrs_hip.h, "burst list"): qd_bursts_init / _fold / _finish against a referee written here with
Python integers from the definition (column by column, itertools.groupby on `on`), partition independence, planted columns, cap, the
error codes, and the launch geometry of the k_bursts_* kernels (quadrs_amd/csrc/qd_bursts.h) walked by a stand-alone host program.
No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_bands_cpu import patterns

F32 = np.float32
INF_BITS = 0x7F800000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrs_amd", "csrc")
BURST = np.dtype([("first", "<u8"), ("length", "<u8"), ("peak_at", "<u8"), ("bin", "<u4"), ("peak", "<f4")])
# 0, the smallest subnormal, 1.0, 1.5, +inf, NaN, -NaN
THRESHOLD_BITS = np.array([0, 1, 0x3F800000, 0x3FC00000, INF_BITS, 0x7FC00000, 0xFFC00001], dtype=np.uint32)


def cycled_thresholds(W, shift=0):
    return THRESHOLD_BITS[(np.arange(W) + shift) % THRESHOLD_BITS.size].view(F32)


def ref_on(bits, thresholds):
    """on[n, W] of u32 bit patterns [n, W] and f32 thresholds [W], with Python integers"""
    n, W = bits.shape
    on = np.zeros((n, W), dtype=bool)
    for b in range(W):
        t = int(np.asarray(thresholds, F32).view(np.uint32)[b])
        masked = (t & 0x7FFFFFFF) > INF_BITS
        assert masked or t <= INF_BITS, "the referee is asked only admissible thresholds"
        for i in range(n):
            a = int(bits[i, b]) & 0x7FFFFFFF
            on[i, b] = (not masked) and a <= INF_BITS and a >= t
    return on


def ref_bursts(bits, thresholds, min_len):
    """(list BURST in order, found, on_counts u64[W]) of u32 bit patterns [n, W], by the definition"""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    n, W = bits.shape
    on = ref_on(bits, thresholds)
    recs = []
    for b in range(W):
        mags = [int(x) & 0x7FFFFFFF for x in bits[:, b]]
        i = 0
        for key, grp in itertools.groupby(on[:, b].tolist()):
            length = len(list(grp))
            if key and length >= min_len:
                run = mags[i:i + length]
                peak = max(run)
                recs.append((i + length - 1, b, i, length, i + run.index(peak), peak))
            i += length
    recs.sort()
    assert len({r[:2] for r in recs}) == len(recs)                         # no two bursts share (last window, bin)
    out = np.zeros(len(recs), dtype=BURST)
    for k, (_, b, first, length, at, peak) in enumerate(recs):
        out[k] = (first, length, at, b, np.uint32(peak).view(F32))
    out["peak"].view(np.uint32)[:] = [r[5] for r in recs]
    return out, len(recs), on.sum(axis=0).astype(np.uint64)


def same(got, ref):
    assert got[1] == ref[1], (got[1], ref[1])
    assert got[0].dtype == BURST and got[0].tobytes() == ref[0].tobytes()
    assert got[2].dtype == np.uint64 and got[2].tobytes() == ref[2].tobytes()
    return True


def test_record_layout(engine):
    assert BURST.itemsize == 32 and engine.BURST_DTYPE == BURST
    assert [BURST.fields[k][1] for k in ("first", "length", "peak_at", "bin", "peak")] == [0, 8, 16, 24, 28]


@pytest.mark.parametrize("W", [1, 2, 4, 64, 256])
def test_twin_matches_the_integer_referee(engine, W):
    n = 200
    bits = patterns(n, W, 900 + W)
    lengths = set()
    for shift in ((0, 2, 3) if W < 4 else (0,)):
        thr = cycled_thresholds(W, shift)
        for min_len in (1, 2, 5, n, n + 1):
            ref = ref_bursts(bits, thr, min_len)
            assert same(engine.bursts_of(bits.view(F32), thr, min_len, cap=n * W), ref)
            lengths.update(ref[0]["length"].tolist())
    # a column of the one binade alone, so that thresholds 1.0 and 1.5 bite, and one that is on throughout
    col = np.full((n, 1), 0x3F800000, np.uint32)
    assert same(engine.bursts_of(col.view(F32), np.array([1.0], F32), n, cap=4), ref_bursts(col, np.array([1.0], F32), n))
    assert engine.bursts_of(col.view(F32), np.array([1.0], F32), n + 1, cap=4)[1] == 0
    if W >= 4:
        assert min(lengths) == 1 and max(lengths) >= 5                     # teeth: short and long runs in this very input


SEAMS = {"whole": [37], "1+36": [1, 36], "7+7+23": [7, 7, 23], "rows": [1] * 37, "with empties": [0, 7, 0, 0, 7, 23, 0]}


def test_partition_independence(engine):
    n, W = 37, 8
    bits = patterns(n, W, 41)
    bits[:, 0] = 0x3F800000                                                # bin 0 (threshold 0) is on throughout: a run crosses every seam
    bits[5:9, 2] = 0x3FC00000                                              # bin 2 (threshold 1.0): a run over the seam at 7
    thr = cycled_thresholds(W)
    on = ref_on(bits, thr)
    ref = ref_bursts(bits, thr, 2)
    results = {}
    for name, parts in SEAMS.items():
        assert sum(parts) == n
        state, counts = engine.bursts_init(W)
        into = np.zeros(n * W, dtype=BURST)
        found, at = 0, 0
        for k in parts:
            if 0 < at < n and k:
                assert (on[at - 1] & on[at]).any(), "no run crosses the seam at %d" % at
            found = engine.bursts_fold(state, bits[at:at + k].view(F32), thr, 2, at, into, found, counts)
            at += k
        assert int(state[-1]) == n
        found = engine.bursts_finish(state, 2, into, found)
        fresh, _ = engine.bursts_init(W)
        assert state.tobytes() == fresh.tobytes()                          # _finish leaves the state as _init does
        results[name] = (into[:found], found, counts)
        assert same(results[name], ref), name
    assert (on[6, 2] and on[7, 2]) and ref[1] > W


def planted(engine, column, threshold, min_len=1):
    a = np.asarray(column, dtype=F32).reshape(-1, 1)
    got = engine.bursts_of(a, np.array([threshold], F32), min_len)
    assert same(got, ref_bursts(a.view(np.uint32), np.array([threshold], F32), min_len))
    return [(int(r["first"]), int(r["length"]), int(r["peak_at"]), float(r["peak"])) for r in got[0]], got


def test_planted_columns(engine):
    n = 11
    nan, inf = np.uint32(0x7FC00000).view(F32), F32(np.inf)
    recs, got = planted(engine, [2.0] * n, 1.0)
    assert recs == [(0, n, 0, 2.0)] and got[2].tolist() == [n]             # a run over the whole range
    recs, got = planted(engine, [2.0, 0.5] * 5 + [2.0], 1.0)
    assert len(recs) == (n + 1) // 2 and all(r[1] == 1 for r in recs) and got[2].tolist() == [6]      # alternating: ceil(n / 2) bursts
    recs, _ = planted(engine, [1, 3, 2, 3, 3, 0, 5, 5], 1.0)
    assert recs == [(0, 5, 1, 3.0), (6, 2, 6, 5.0)]                        # equal peaks: the first window wins
    recs, _ = planted(engine, [0, 2, inf, 2, 0], 1.0)
    assert recs == [(1, 3, 2, np.inf)]
    recs, got = planted(engine, [0, 2, inf, 2, 0], inf)
    assert recs == [(2, 1, 2, np.inf)] and got[2].tolist() == [1]          # +inf turns on only +inf
    recs, _ = planted(engine, [2, 2, nan, 2, 2], 0.0)
    assert recs == [(0, 2, 0, 2.0), (3, 2, 3, 2.0)]                        # a NaN splits a run, even at threshold 0
    recs, _ = planted(engine, [2, -3, 2, 0.5], 1.0)
    assert recs == [(0, 3, 1, 3.0)]                                        # a negative value counts by magnitude; the peak has no sign
    # a masked bin beside a threshold-0 bin
    a = np.array([[5, 5], [nan, 5], [5, 5]], dtype=F32)
    thr = np.array([0.0, nan], F32)
    got = engine.bursts_of(a, thr)
    assert same(got, ref_bursts(a.view(np.uint32), thr, 1))
    assert got[0]["bin"].tolist() == [0, 0] and got[2].tolist() == [2, 0]
    # the order is by last window, then bin: bin 1's burst ends first
    a = np.array([[2, 2], [2, 0], [0, 0]], dtype=F32)
    got = engine.bursts_of(a, 1.0)
    assert got[0]["bin"].tolist() == [1, 0] and got[0]["length"].tolist() == [1, 2]
    # min_len filters the list, not the occupancy
    got = engine.bursts_of(a, 1.0, min_len=2)
    assert got[0]["bin"].tolist() == [0] and got[2].tolist() == [2, 1]


def test_cap_keeps_the_prefix_and_the_full_count(engine):
    n, W = 40, 16
    bits = patterns(n, W, 7)
    bits[n - 1, :4] = 0x3F800000                                           # runs that are open at the end: _finish has bursts to close
    thr = cycled_thresholds(W)
    full, found, counts = ref_bursts(bits, thr, 1)
    assert found > 4
    closes = 0
    for cap in (0, 1, found - 1, found, found + 1):
        buf = np.full((cap + 2) * 32, 0xA5, dtype=np.uint8)                # sentinel records past cap, too
        into = buf[:cap * 32].view(BURST)
        state, on_counts = engine.bursts_init(W)
        f = engine.bursts_fold(state, bits[:n - 3].view(F32), thr, 1, 0, into if cap else None, 0, on_counts)
        f = engine.bursts_fold(state, bits[n - 3:].view(F32), thr, 1, n - 3, into if cap else None, f, on_counts)
        before = f
        f = engine.bursts_finish(state, 1, into if cap else None, f)
        closes = f - before
        assert f == found and on_counts.tobytes() == counts.tobytes()
        k = min(found, cap)
        assert buf[:k * 32].tobytes() == full[:k].tobytes()
        assert (buf[k * 32:] == 0xA5).all()
    assert closes > 0                                                       # _finish itself ran into the cap
    lst, f, _ = engine.bursts_of(bits.view(F32), thr, 1, cap=3)
    assert f == found and lst.tobytes() == full[:3].tobytes()


def test_refusals(engine):
    from quadrs_amd import _ffi
    L, INVALID = _ffi.lib(), _ffi.ERR_INVALID
    W = 4
    a = np.ones((2, W), F32)
    norms = a.ctypes.data_as(C.c_void_p)
    state, counts = engine.bursts_init(W)
    clean = state.copy()
    sp, cp = state.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)
    lst = np.full(8 * 32, 0x5A, np.uint8)
    lp = lst.ctypes.data_as(C.c_void_p)
    found = C.c_uint64(0)
    ok = np.array([0, 1, np.inf, np.nan], F32)

    def fold(state=sp, width=W, thr=ok, min_len=1, at=0, norms=norms, n=2, lst=lp, cap=8, found=C.byref(found), counts=cp):
        t = None if thr is None else np.ascontiguousarray(thr, F32)
        return L.qd_bursts_fold(state, width, None if t is None else t.ctypes.data_as(C.c_void_p), min_len, at, norms, n, lst, cap, found, counts)
    assert fold(width=0) == INVALID
    assert fold(state=None) == INVALID
    assert fold(thr=None) == INVALID
    assert fold(found=None) == INVALID
    assert fold(min_len=0) == INVALID
    assert fold(lst=None) == INVALID                                       # list NULL with cap > 0
    assert fold(norms=None) == INVALID                                     # norms NULL with n > 0
    assert fold(at=1) == INVALID                                           # not the state's next window
    for bad in (-1.0, -0.0, -np.inf, -1e-45):
        assert fold(thr=np.array([0, bad, 1, 1], F32)) == INVALID, bad
    assert state.tobytes() == clean.tobytes() and (lst == 0x5A).all() and found.value == 0 and not counts.any()
    assert L.qd_bursts_init(None, None, W) == INVALID and L.qd_bursts_init(sp, None, 0) == INVALID
    assert L.qd_bursts_finish(None, W, 1, lp, 8, C.byref(found)) == INVALID
    assert L.qd_bursts_finish(sp, 0, 1, lp, 8, C.byref(found)) == INVALID
    assert L.qd_bursts_finish(sp, W, 0, lp, 8, C.byref(found)) == INVALID
    assert L.qd_bursts_finish(sp, W, 1, None, 8, C.byref(found)) == INVALID
    assert L.qd_bursts_finish(sp, W, 1, lp, 8, None) == INVALID
    # what is fine: nothing to fold, no list with cap 0, no on_counts
    assert fold(norms=None, n=0) == 0 and fold(lst=None, cap=0, counts=None) == 0 and found.value == 0 and int(state[-1]) == 2
    assert fold(at=0) == INVALID and fold(at=2) == 0 and int(state[-1]) == 4
    assert L.qd_bursts_finish(sp, W, 1, lp, 8, C.byref(found)) == 0 and found.value == 2 and state.tobytes() == clean.tobytes()
    assert lst[:64].view(BURST)["length"].tolist() == [4, 4] and (lst[64:] == 0x5A).all()
    with pytest.raises(ValueError):
        engine.bursts_of(a, np.zeros(W + 1, F32))
    # qd_plan_bursts without a plan is refused before anything else is looked at, as every plan call is
    t = ok.ctypes.data_as(C.c_void_p)
    assert L.qd_plan_bursts(None, None, _ffi.MEM_HOST, 0, 0, 0, 1, t, 1, lp, 8, C.byref(found), cp, _ffi.MEM_HOST, None) == INVALID
    assert _ffi.BURSTS_WORDS == 3


def test_burst_rules_live_in_one_host_clean_header(tmp_path):
    tu = tmp_path / "only_bursts.cpp"
    tu.write_text('#include "qd_bursts.h"\nint main() { qd::BurstsGeometry G; uint64_t grid; qd::bursts_split(0, 1, 4, 1, &G, &grid);\n'
                  '    uint32_t w; return qd::bursts_lane(G, 0, 0).active && qd::bursts_threshold(0, &w) && qd::bursts_on(1, w) ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the host source takes the rules from the header: it carries no copy of the piece arithmetic or of the comparison
    text = open(os.path.join(CSRC, "quadrs_hip.hip"), encoding="utf-8").read()
    for phrase in ("log2_P", "G.ppg", "kBurstsMinSeg", "kBurstsLdsWords"):
        assert phrase not in text, phrase


WALKER = r"""
#include "qd_bursts.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace qd;

static unsigned long long g_ctx[8];
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s\n  W %llu n %llu batch %llu cu %llu g0 %llu block %llu tid %llu\n", #c, \
    g_ctx[0], g_ctx[1], g_ctx[2], g_ctx[3], g_ctx[4], g_ctx[5], g_ctx[6]); std::exit(1); } } while (0)

static unsigned long long g_launches = 0, g_cells = 0;

// every (workgroup, lane) of the piece launches (k_bursts_edge, k_bursts_emit<COUNT>, k_bursts_emit<EMIT>: all three take their indices
// from bursts_lane) and of k_bursts_stitch and k_bursts_close, for a range of n windows cut into the given batches
static void walk(uint32_t W, uint64_t n, const std::vector<uint64_t> &cuts, int n_cu) {
    g_ctx[0] = W; g_ctx[1] = n; g_ctx[2] = cuts[0]; g_ctx[3] = (unsigned long long)n_cu;
    std::vector<uint8_t> seen(n * W, 0);
    uint64_t longest = 0;
    for (uint64_t c : cuts) longest = c > longest ? c : longest;
    uint64_t g0 = 0;
    for (size_t ci = 0; g0 < n; ++ci) {
        const uint64_t bw = cuts[ci % cuts.size()], nw = n - g0 < bw ? n - g0 : bw;
        g_ctx[4] = g0; g_ctx[5] = g_ctx[6] = ~0ull;
        BurstsGeometry G;
        uint64_t grid = 0;
        bursts_split(g0, nw, W, n_cu, &G, &grid);
        ++g_launches;
        // the rules of the header
        CHECK(G.P >= 1 && G.P <= kBurstsThreads && (G.P & (G.P - 1)) == 0 && (1u << G.log2_P) == G.P && G.ppg * G.P == kBurstsThreads);
        CHECK(W > kBurstsThreads ? (G.P == kBurstsThreads && G.n_slabs == (W + 255) / 256) : (G.P >= W && (G.P == 1 || G.P / 2 < W) && G.n_slabs == 1));
        CHECK(G.seg >= 1 && G.seg <= bursts_seg_max(W) && (G.seg >= kBurstsMinSeg || G.seg == bursts_seg_max(W)));
        CHECK(G.seg * G.n_slabs * kBurstsWaves <= kBurstsLdsWords);                      // the LDS budget
        CHECK(G.n_pieces == (nw + G.seg - 1) / G.seg && G.n_pieces <= bursts_pieces_bound(longest, W, n_cu));
        CHECK(grid > 0 && grid <= 0x7fffffffull && (grid - 1) * G.ppg < G.n_pieces && grid * G.ppg >= G.n_pieces);
        std::vector<uint8_t> summary(G.n_pieces * W, 0), word_taken(kBurstsLdsWords, 0);
        uint64_t next_wa = g0;                                                            // pieces tile the batch in order
        for (uint64_t block = 0; block < grid; ++block) {
            g_ctx[5] = block;
            for (uint32_t i = 0; i < kBurstsLdsWords; ++i) word_taken[i] = 0;
            for (uint32_t tid = 0; tid < kBurstsThreads; ++tid) {
                g_ctx[6] = tid;
                const BurstsLane l = bursts_lane(G, (uint32_t)block, tid);
                const uint32_t wave = tid / 64;
                CHECK(l.slot == tid / G.P && l.col0 == tid % G.P && l.piece == block * G.ppg + l.slot && l.active == (l.piece < G.n_pieces));
                // the ballot words: one per (row, slab, wave), inside the budget; a lane's piece is the mask's lanes of the words' waves
                const uint32_t pw0 = bursts_piece_wave0(G, tid), pwn = bursts_piece_waves(G);
                const uint64_t mask = bursts_piece_mask(G, tid);
                CHECK(wave >= pw0 && wave < pw0 + pwn && pw0 + pwn <= kBurstsWaves && ((mask >> (tid % 64)) & 1));
                for (uint32_t t2 = 0; t2 < kBurstsThreads; ++t2) {
                    const bool same_piece = t2 / G.P == l.slot;
                    const bool covered = t2 / 64 >= pw0 && t2 / 64 < pw0 + pwn && ((mask >> (t2 % 64)) & 1);
                    CHECK(G.P < 64 ? (t2 / 64 != wave || same_piece == covered) : same_piece == covered);
                }
                if (tid % 64 == 0)
                    for (uint32_t j = 0; j < G.seg; ++j)
                        for (uint32_t s = 0; s < G.n_slabs; ++s) {
                            const uint32_t at = bursts_word(G, j, s, wave);
                            CHECK(at < kBurstsLdsWords && at < G.seg * G.n_slabs * kBurstsWaves && word_taken[at] == 0);
                            word_taken[at] = 1;
                        }
                if (!l.active) { CHECK(l.wa == l.wb); continue; }
                CHECK(l.wa == g0 + l.piece * G.seg && l.wb > l.wa && l.wb <= g0 + nw && l.wb - l.wa <= G.seg && (l.wb - l.wa == G.seg || l.wb == g0 + nw));
                if (l.col0 == 0) { CHECK(l.wa == next_wa); next_wa = l.wb; }
                for (uint32_t s = 0; s < G.n_slabs; ++s) {
                    const uint32_t col = bursts_col(l, s);
                    CHECK(col == l.col0 + s * kBurstsThreads);                            // consecutive lanes, consecutive words
                    if (col >= W) continue;
                    for (uint64_t w = l.wa; w < l.wb; ++w) {
                        uint8_t &c = seen[w * W + col];
                        CHECK(c == 0);
                        c = 1; ++g_cells;
                    }
                    // the piece's words in the workspace: the three planes of a piece, one word a bin, nobody else's
                    CHECK(bursts_slot_word(W, l.piece, 0, col) == (l.piece * 3) * W + col && bursts_slot_word(W, l.piece, 2, col) == (l.piece * 3 + 2) * W + col);
                    CHECK(summary[l.piece * W + col] == 0);
                    summary[l.piece * W + col] = 1;
                }
            }
        }
        g_ctx[5] = g_ctx[6] = ~0ull;
        CHECK(next_wa == g0 + nw);
        for (uint8_t c : summary) CHECK(c == 1);
        // k_bursts_stitch: a lane a (group of consecutive pieces, bin); every (piece, bin) has one lane, the groups in order
        std::vector<uint8_t> stitched(G.n_pieces * W, 0);
        static_assert(kBurstsStitchGroups * kBurstsStitchBins == kBurstsThreads, "a lane for each (group, bin) of a workgroup");
        for (uint32_t block = 0; block < (W + kBurstsStitchBins - 1) / kBurstsStitchBins; ++block)
            for (uint32_t tid = 0; tid < kBurstsThreads; ++tid) {
                const BurstsStitchLane l = bursts_stitch_lane(G, block, tid);
                CHECK(l.group == tid / kBurstsStitchBins && l.col == block * kBurstsStitchBins + tid % kBurstsStitchBins && l.active == (l.col < W));
                CHECK(l.q0 <= l.q1 && l.q1 <= G.n_pieces && (l.group != 0 || l.q0 == 0) && (l.group != kBurstsStitchGroups - 1 || l.q1 == G.n_pieces));
                if (l.group) CHECK(l.q0 == bursts_stitch_lane(G, block, tid - kBurstsStitchBins).q1);
                if (!l.active) continue;
                for (uint64_t q = l.q0; q < l.q1; ++q) { CHECK(stitched[q * W + l.col] == 0); stitched[q * W + l.col] = 1; }
            }
        for (uint8_t c : stitched) CHECK(c == 1);
        // k_bursts_close: a lane a bin in slabs of 256, every bin once
        std::vector<uint8_t> bin(W, 0);
        for (uint32_t c0 = 0; c0 < W; c0 += kBurstsThreads)
            for (uint32_t tid = 0; tid < kBurstsThreads; ++tid)
                if (c0 + tid < W) { CHECK(bin[c0 + tid] == 0); bin[c0 + tid] = 1; }
        for (uint8_t c : bin) CHECK(c == 1);
        g0 += nw;
    }
    for (uint8_t c : seen) CHECK(c == 1);
}

int main() {
    CHECK(bursts_lanes(1) == 1 && bursts_lanes(2) == 2 && bursts_lanes(3) == 4 && bursts_lanes(64) == 64 && bursts_lanes(96) == 128 && bursts_lanes(2048) == 256);
    CHECK(bursts_seg_max(1) == 512 && bursts_seg_max(256) == 512 && bursts_seg_max(257) == 256 && bursts_seg_max(2048) == 64 && bursts_seg_max(131072) == 1);
    CHECK(bursts_seg_max(131073) == 0);
    uint32_t w = 7;
    CHECK(bursts_threshold(0, &w) && w == 0 && bursts_threshold(0x7f800000u, &w) && w == 0x7f800000u);
    CHECK(bursts_threshold(0x7fc00000u, &w) && w == kBurstsMasked && bursts_threshold(0xffc00001u, &w) && w == kBurstsMasked);
    CHECK(!bursts_threshold(0x80000000u, &w) && !bursts_threshold(0xff800000u, &w) && !bursts_threshold(0xbf800000u, &w));
    CHECK(bursts_on(0, 0) && !bursts_on(0x7f800001u, 0) && bursts_on(0x7f800000u, 0x7f800000u) && !bursts_on(0x7f7fffffu, 0x7f800000u) && !bursts_on(0x7f800000u, kBurstsMasked));
    const uint32_t Ws[] = {1, 2, 4, 64, 96, 128, 1024, 2048};
    const int cus[] = {1, 8, 256};
    for (uint32_t W : Ws)
        for (int cu : cus) {
            const uint64_t big = W >= 1024 ? 700 : 5000;
            walk(W, 1, {1}, cu);
            walk(W, 37, {37}, cu);
            walk(W, 37, {1}, cu);                                  // one-window batches
            walk(W, 333, {100, 7, 1, 64}, cu);                     // ragged
            walk(W, big, {big}, cu);
            walk(W, big, {big / 3 + 1}, cu);
            walk(W, big, {513, 16, 17}, cu);
        }
    walk(4, 600000, {600000}, 256);                                // the piece count's cap: seg above the minimum
    walk(1, 5000000, {4200000}, 256);                              // ... and seg at its LDS limit
    std::printf("ok: %llu launches, %llu cells\n", g_launches, g_cells);
    return 0;
}
"""


def test_every_lane_of_every_launch(tmp_path):
    """Over W in {1, 2, 4, 64, 96, 128, 1024, 2048}, 1, 8 and 256 compute units, ranges in one batch, in one-window batches and in ragged
    ones: the geometry obeys the header's rules; pieces tile each batch in order; in the piece launches every cell of every batch is
    walked by exactly one lane, consecutive lanes on consecutive words, and every (piece, bin) summary is written once; in the stitch
    every (piece, bin) has one lane and the groups tile the pieces in order, in the close every bin has one lane; the ballot words of a workgroup are distinct and stay within the stated LDS budget, and a lane's
    piece mask and waves are exactly its piece's lanes."""
    src = tmp_path / "walk_bursts.cpp"
    src.write_text(WALKER)
    exe = tmp_path / "walk_bursts"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
