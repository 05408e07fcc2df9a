"""The emission list's host half (include/quadrs_hip.h, "emission list"): qd_emissions_init / _fold / _finish against a referee written
here from the definition (a flood fill over the on matrix in plain Python, records, filter and sort), over seeded partitions of the
range into folds, with the teeth asserted on the referee's own output; cap, the error codes, and the launch geometry of the
k_emissions_* kernels (quadrs_amd/csrc/qd_emissions.h) walked by a stand-alone host program.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

F32 = np.float32
INF_BITS = 0x7F800000
NAN_BITS = 0x7FC00000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrs_amd", "csrc")
EMISSION = np.dtype([("first", "<u8"), ("last", "<u8"), ("cells", "<u8"), ("peak_at", "<u8"), ("lo", "<u4"), ("hi", "<u4"), ("end_bin", "<u4"),
                     ("peak_bin", "<u4"), ("peak", "<f4"), ("flags", "<u4")])


def ref_on(bits, thresholds):
    """(on[n, W], mag[n, W]) of u32 bit patterns [n, W] and f32 thresholds [W], from the definition's integers"""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    t = np.ascontiguousarray(thresholds, dtype=F32).view(np.uint32).astype(np.int64)
    masked = (t & 0x7FFFFFFF) > INF_BITS
    assert (masked | (t <= INF_BITS)).all(), "the referee is asked only admissible thresholds"
    mag = bits.astype(np.int64) & 0x7FFFFFFF
    return (~masked)[None, :] & (mag <= INF_BITS) & (mag >= t[None, :]), mag


def ref_emissions(bits, thresholds, min_len=1, min_cells=1):
    """(list EMISSION in order, found, components before the filter) of u32 bit patterns [n, W]: a flood fill, by the definition"""
    on, mag = ref_on(bits, thresholds)
    n, W = on.shape
    on_l, mag_l = on.tolist(), mag.tolist()
    seen = [[False] * W for _ in range(n)]
    recs = []
    for i0 in range(n):
        for b0 in range(W):
            if not on_l[i0][b0] or seen[i0][b0]:
                continue
            seen[i0][b0] = True
            stack, cells = [(i0, b0)], []
            while stack:
                i, b = stack.pop()
                cells.append((i, b))
                for j, c in ((i - 1, b), (i + 1, b), (i, b - 1), (i, b + 1)):      # 4 neighbours; a row does not wrap
                    if 0 <= j < n and 0 <= c < W and on_l[j][c] and not seen[j][c]:
                        seen[j][c] = True
                        stack.append((j, c))
            first, last = min(i for i, _ in cells), max(i for i, _ in cells)
            peak = max(mag_l[i][b] for i, b in cells)
            peak_at, peak_bin = min((i, b) for i, b in cells if mag_l[i][b] == peak)
            recs.append(dict(first=first, last=last, cells=len(cells), peak_at=peak_at, lo=min(b for _, b in cells), hi=max(b for _, b in cells),
                             end_bin=min(b for i, b in cells if i == last), peak_bin=peak_bin, peak=peak,
                             flags=(1 if first == 0 else 0) | (2 if last == n - 1 else 0)))
    kept = [r for r in recs if r["last"] - r["first"] + 1 >= min_len and r["cells"] >= min_cells]
    kept.sort(key=lambda r: (r["last"], r["end_bin"]))
    assert len({(r["last"], r["end_bin"]) for r in recs}) == len(recs)       # no two emissions share (last, end_bin)
    out = np.zeros(len(kept), dtype=EMISSION)
    for k, r in enumerate(kept):
        for name in EMISSION.names:
            if name != "peak":
                out[k][name] = r[name]
    out["peak"].view(np.uint32)[:] = [r["peak"] for r in kept]
    return out, len(kept), len(recs)


def same(got, ref):
    assert got[1] == ref[1], (got[1], ref[1])
    assert got[0].dtype == EMISSION
    if got[0].tobytes() != ref[0].tobytes():
        k = next(i for i in range(len(ref[0])) if got[0][i:i + 1].tobytes() != ref[0][i:i + 1].tobytes())
        raise AssertionError("record %d: got %s, referee %s" % (k, got[0][k], ref[0][k]))
    return True


def matrix(n, W, occupancy, seed):
    """u32 patterns [n, W] of which about `occupancy` are at or above 1.0: a few magnitudes only (so peaks tie), both signs, NaN and
    +-inf cells; occupancy 1.0 leaves no cell off"""
    rng = np.random.default_rng(seed)
    loud = np.array([1.0, 1.5, 1.5, 2.0, 3.0, 3.0], F32).view(np.uint32)
    quiet = np.array([0.0, 0.25, 0.5], F32).view(np.uint32)
    bits = np.where(rng.random((n, W)) < occupancy, loud[rng.integers(0, loud.size, (n, W))], quiet[rng.integers(0, quiet.size, (n, W))]).astype(np.uint32)
    bits ^= (rng.random((n, W)) < 0.3).astype(np.uint32) << 31              # the sign is dropped
    if occupancy < 1.0:
        bits[rng.random((n, W)) < 0.02] = NAN_BITS
        bits[rng.random((n, W)) < 0.01] = 0xFFC00001
    bits[rng.random((n, W)) < 0.01] = INF_BITS
    bits[rng.random((n, W)) < 0.01] = 0xFF800000
    return bits


def partitions(n, seed):
    """a seeded set of cuts of [0, n) into folds: whole, one-row folds, folds with n == 0 among them, ragged ones"""
    rng = np.random.default_rng(seed)
    out = [[n], [1] * n, [0, n, 0]]
    if n >= 2:
        out.append([1, n - 1])
        out.append([n - 1, 0, 1])
    for _ in range(3):
        parts, left = [], n
        while left:
            k = int(min(left, rng.integers(0, max(2, n // 3))))
            parts.append(k)
            left -= k
        out.append(parts)
    return out


def twin(engine, bits, thr, min_len, min_cells, parts, cap=None):
    n, W = bits.shape
    state = engine.emissions_init(W)
    into = np.zeros(n * W if cap is None else cap, dtype=EMISSION)
    found, at = 0, 0
    for k in parts:
        found = engine.emissions_fold(state, bits[at:at + k].view(F32), thr, min_len, min_cells, at, into if into.size else None, found)
        at += k
    assert at == n and int(state[-2]) == n
    found = engine.emissions_finish(state, min_len, min_cells, into if into.size else None, found)
    assert state.tobytes() == engine.emissions_init(W).tobytes()            # _finish leaves the state as _init does
    return into[:min(found, into.size)], found


def test_record_layout(engine):
    from quadrs_amd import _ffi
    assert EMISSION.itemsize == 56 and engine.EMISSION_DTYPE == EMISSION and _ffi.EMISSIONS_WORDS == 8
    assert [EMISSION.fields[k][1] for k in EMISSION.names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    assert engine.emissions_init(5).size == 8 * 5 + 2


def thresholds_for(W, kind):
    if kind == "one":
        return np.full(W, 1.0, F32)
    if kind == "zero":
        return np.zeros(W, F32)
    if kind == "inf":
        return np.full(W, np.inf, F32)
    t = np.array([1.0, 1.5, 1.0, 2.0, 0.0, 1.0, np.nan, 1.0], F32)[np.arange(W) % 8]        # mixed, with a masked bin and a threshold-0 bin
    return np.ascontiguousarray(t)


@pytest.mark.parametrize("W", [1, 2, 3, 64, 96])
def test_twin_matches_the_flood_fill_referee(engine, W):
    n = 400 if W <= 3 else 120
    components = 0
    for occupancy in (0.1, 0.5, 0.7, 1.0):
        bits = matrix(n, W, occupancy, 1000 * W + int(occupancy * 10))
        for kind in ("one", "mixed", "zero", "inf"):
            thr = thresholds_for(W, kind)
            for min_len, min_cells in ((1, 1), (3, 1), (1, 4), (n, 1), (n + 1, 1)):
                if (min_len, min_cells) != (1, 1) and kind != "one":
                    continue
                ref = ref_emissions(bits, thr, min_len, min_cells)
                components += ref[2]
                for parts in (partitions(n, W) if (min_len, min_cells) == (1, 1) and kind in ("one", "mixed") else [[n], [n // 2, n - n // 2]]):
                    assert same(twin(engine, bits, thr, min_len, min_cells, parts), ref), (occupancy, kind, min_len, min_cells, parts[:6])
                assert same(engine.emissions_of(bits.view(F32), thr, min_len, min_cells, cap=n * W), ref)
        if occupancy == 1.0:                                               # threshold 0 over a matrix without NaN: one emission holds everything
            ref = ref_emissions(bits, np.zeros(W, F32))
            assert ref[1] == 1 and int(ref[0]["cells"][0]) == n * W and int(ref[0]["flags"][0]) == 3
    assert components > 0


def test_component_count_agrees_with_scipy_where_it_is_installed():
    ndimage = pytest.importorskip("scipy.ndimage")
    bits = matrix(60, 40, 0.5, 5)
    thr = thresholds_for(40, "mixed")
    on, _ = ref_on(bits, thr)
    assert ndimage.label(on)[1] == ref_emissions(bits, thr)[2]


def planted_ring():
    """12 windows x 12 bins at threshold 1.0: a ring with one cell inside it, two emissions that end in one window, all four flag values"""
    a = np.zeros((12, 12), F32)
    a[2, 2:7] = a[6, 2:7] = 2.0
    a[2:7, 2] = a[2:7, 6] = 2.0                                            # the ring: windows 2 ... 6, bins 2 ... 6
    a[4, 4] = 5.0                                                           # the cell inside, not connected to the ring
    a[5:9, 9] = 3.0                                                         # ends in window 8 ...
    a[8, 0:2] = 3.0                                                         # ... and so does this one
    a[0, 11] = 1.0                                                          # cut at the first window
    a[11, 4:6] = 1.0                                                        # cut at the last window
    return a


def test_teeth_of_the_referee_and_the_twin_on_them(engine):
    a = planted_ring()
    ref = ref_emissions(a.view(np.uint32), np.full(12, 1.0, F32))
    assert same(engine.emissions_of(a, 1.0), ref)
    L = ref[0]
    assert any(r["hi"] > r["lo"] and r["last"] > r["first"] for r in L)    # an emission that spans bins and windows
    ring = L[(L["cells"] == 16)][0]
    inside = L[(L["first"] == 4) & (L["last"] == 4) & (L["lo"] == 4)][0]
    assert ring["lo"] < inside["lo"] and inside["hi"] < ring["hi"] and ring["first"] < inside["first"] and inside["last"] < ring["last"]
    assert ring["end_bin"] == 2 and ring["hi"] == 6
    # the enclosed cell ends first, so it is reported before the ring that holds it
    order = [(int(r["last"]), int(r["end_bin"])) for r in L]
    assert order == sorted(order) and order.index((4, 4)) < order.index((6, 2))
    # a hook that ends at its lowest bin beside a cell under it: by (last, end_bin) the hook comes first, by (last, hi) it would not
    b = np.zeros((5, 9), F32)
    b[1, 1:8] = 2.0
    b[1:4, 1] = 2.0                                                         # ends in window 3 at end_bin 1, hi 7
    b[3, 3] = 2.0                                                           # ends in window 3 at bin 3, enclosed by the hook's bins
    ref2 = ref_emissions(b.view(np.uint32), np.full(9, 1.0, F32))
    assert same(engine.emissions_of(b, 1.0), ref2)
    assert [(int(r["end_bin"]), int(r["hi"])) for r in ref2[0]] == [(1, 7), (3, 3)]
    # the mirrored hook: its end_bin is not its lowest bin
    c = np.zeros((5, 9), F32)
    c[1, 1:8] = 2.0
    c[1:4, 7] = 2.0                                                         # an L: ends in window 3 at end_bin 7, lo 1, hi 7
    c[3, 3] = 2.0                                                           # ends in window 3 at bin 3
    ref3 = ref_emissions(c.view(np.uint32), np.full(9, 1.0, F32))
    assert same(engine.emissions_of(c, 1.0), ref3)
    assert [(int(r["end_bin"]), int(r["lo"])) for r in ref3[0]] == [(3, 3), (7, 1)]      # by end_bin: by lo or hi alone the L would not sort so
    assert sorted(L["flags"].tolist())[0] == 0 and {1, 2} <= set(L["flags"].tolist())
    whole = ref_emissions(np.full((3, 2), 2.0, F32).view(np.uint32), np.full(2, 1.0, F32))[0]
    assert whole["flags"].tolist() == [3]
    assert sum(1 for r in L if r["last"] == 8) == 2                         # two emissions end in the same window
    # min_len and min_cells each drop something the other keeps: a row of 2 cells in one window, a column of 2 windows
    d = np.zeros((6, 6), F32)
    d[1, 0:3] = 2.0                                                         # 3 cells, 1 window
    d[3:5, 5] = 2.0                                                         # 2 cells, 2 windows
    thr = np.full(6, 1.0, F32)
    by_len, by_cells = ref_emissions(d.view(np.uint32), thr, 2, 1), ref_emissions(d.view(np.uint32), thr, 1, 3)
    assert by_len[0]["lo"].tolist() == [5] and by_cells[0]["lo"].tolist() == [0]
    assert same(engine.emissions_of(d, 1.0, 2, 1), by_len) and same(engine.emissions_of(d, 1.0, 1, 3), by_cells)
    # tied peaks: the lexicographically smallest (window, bin) wins, across a merge of two branches
    e = np.zeros((4, 5), F32)
    e[0:3, 0] = [2, 7, 2]
    e[0:3, 4] = [7, 2, 2]
    e[2, 0:5] = 2.0
    e[2, 2] = 7.0
    ref5 = ref_emissions(e.view(np.uint32), np.full(5, 1.0, F32))
    assert same(engine.emissions_of(e, 1.0), ref5)
    assert (int(ref5[0]["peak_at"][0]), int(ref5[0]["peak_bin"][0])) == (0, 4)


def test_cap_keeps_the_prefix_and_the_full_count(engine):
    n, W = 40, 16
    bits = matrix(n, W, 0.4, 7)
    bits[n - 1, :4] = 0x3F800000                                           # open at the end: _finish has emissions to close
    thr = thresholds_for(W, "one")
    full, found, _ = ref_emissions(bits, thr)
    assert found > 4
    closes = 0
    for cap in (0, 1, found - 1, found, found + 1):
        buf = np.full((cap + 2) * 56, 0xA5, dtype=np.uint8)                # sentinel records past cap, too
        into = buf[:cap * 56].view(EMISSION)
        state = engine.emissions_init(W)
        f = engine.emissions_fold(state, bits[:n - 3].view(F32), thr, 1, 1, 0, into if cap else None, 0)
        f = engine.emissions_fold(state, bits[n - 3:].view(F32), thr, 1, 1, n - 3, into if cap else None, f)
        before = f
        f = engine.emissions_finish(state, 1, 1, into if cap else None, f)
        closes = f - before
        assert f == found
        k = min(found, cap)
        assert buf[:k * 56].tobytes() == full[:k].tobytes()
        assert (buf[k * 56:] == 0xA5).all()
    assert closes > 0                                                       # _finish itself ran into the cap
    lst, f = engine.emissions_of(bits.view(F32), thr, 1, 1, cap=3)
    assert f == found and lst.tobytes() == full[:3].tobytes()


def test_refusals(engine):
    from quadrs_amd import _ffi
    L, INVALID = _ffi.lib(), _ffi.ERR_INVALID
    W = 4
    a = np.ones((2, W), F32)
    norms = a.ctypes.data_as(C.c_void_p)
    state = engine.emissions_init(W)
    clean = state.copy()
    sp = state.ctypes.data_as(C.c_void_p)
    lst = np.full(8 * 56, 0x5A, np.uint8)
    lp = lst.ctypes.data_as(C.c_void_p)
    found = C.c_uint64(0)
    ok = np.array([0, 1, np.inf, np.nan], F32)

    def fold(state=sp, width=W, thr=ok, min_len=1, min_cells=1, at=0, norms=norms, n=2, lst=lp, cap=8, found=C.byref(found)):
        t = None if thr is None else np.ascontiguousarray(thr, F32)
        return L.qd_emissions_fold(state, width, None if t is None else t.ctypes.data_as(C.c_void_p), min_len, min_cells, at, norms, n, lst, cap, found)
    assert fold(width=0) == INVALID
    assert fold(state=None) == INVALID
    assert fold(thr=None) == INVALID
    assert fold(found=None) == INVALID
    assert fold(min_len=0) == INVALID
    assert fold(min_cells=0) == INVALID
    assert fold(lst=None) == INVALID                                       # list NULL with cap > 0
    assert fold(norms=None) == INVALID                                     # norms NULL with n > 0
    assert fold(at=1) == INVALID                                           # not the state's next window
    for bad in (-1.0, -0.0, -np.inf, -1e-45):
        assert fold(thr=np.array([0, bad, 1, 1], F32)) == INVALID, bad
    assert state.tobytes() == clean.tobytes() and (lst == 0x5A).all() and found.value == 0
    assert L.qd_emissions_init(None, W) == INVALID and L.qd_emissions_init(sp, 0) == INVALID
    assert L.qd_emissions_finish(None, W, 1, 1, lp, 8, C.byref(found)) == INVALID
    assert L.qd_emissions_finish(sp, 0, 1, 1, lp, 8, C.byref(found)) == INVALID
    assert L.qd_emissions_finish(sp, W, 0, 1, lp, 8, C.byref(found)) == INVALID
    assert L.qd_emissions_finish(sp, W, 1, 0, lp, 8, C.byref(found)) == INVALID
    assert L.qd_emissions_finish(sp, W, 1, 1, None, 8, C.byref(found)) == INVALID
    assert L.qd_emissions_finish(sp, W, 1, 1, lp, 8, None) == INVALID
    # what is fine: nothing to fold, no list with cap 0
    assert fold(norms=None, n=0) == 0 and fold(lst=None, cap=0) == 0 and found.value == 0 and int(state[-2]) == 2
    assert fold(at=0) == INVALID and fold(at=2) == 0 and int(state[-2]) == 4
    assert L.qd_emissions_finish(sp, W, 1, 1, lp, 8, C.byref(found)) == 0 and found.value == 1 and state.tobytes() == clean.tobytes()
    rec = lst[:56].view(EMISSION)[0]                                        # bins 0 and 1 are on (thresholds 0 and 1), bins 2 and 3 are not
    assert (int(rec["first"]), int(rec["last"]), int(rec["cells"]), int(rec["lo"]), int(rec["hi"]), int(rec["flags"])) == (0, 3, 8, 0, 1, 3)
    assert (lst[56:] == 0x5A).all()
    with pytest.raises(ValueError):
        engine.emissions_of(a, np.zeros(W + 1, F32))
    # qd_plan_emissions without a plan is refused before anything else is looked at, as every plan call is
    t = ok.ctypes.data_as(C.c_void_p)
    assert L.qd_plan_emissions(None, None, _ffi.MEM_HOST, 0, 0, 0, 1, t, 1, 1, lp, 8, C.byref(found), _ffi.MEM_HOST, None) == INVALID


def test_emission_rules_live_in_one_host_clean_header(tmp_path):
    tu = tmp_path / "only_emissions.cpp"
    tu.write_text('#include "qd_emissions.h"\nint main() { qd::EmissionsGeometry G; qd::emissions_split(0, 1, 4, 1, &G);\n'
                  '    qd::Emission a = qd::emissions_cell(0, 1, 2); qd::emissions_join(a, qd::emissions_cell(1, 0, 2));\n'
                  '    return qd::emissions_tile_cell(qd::emissions_tile(G, 0), 0, 0).valid && a.cells == 2 && a.end_bin == 0 && a.peak_bin == 1 ? 0 : 1; }\n')
    exe = tmp_path / "only_emissions"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
    # the host source takes the rules from the header: it carries no copy of the tile arithmetic
    text = open(os.path.join(CSRC, "quadrs_hip.hip"), encoding="utf-8").read()
    for phrase in ("kEmissionsTileCells", "kEmissionsSpanCells", "G.tr", "n_tcols *"):
        assert phrase not in text.replace("Q.G.n_trows * Q.G.n_tcols", ""), phrase


WALKER = r"""
#include "qd_emissions.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace qd;

static unsigned long long g_ctx[8];
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s\n  W %llu n %llu batch %llu span %llu w0 %llu block %llu tid %llu\n", #c, \
    g_ctx[0], g_ctx[1], g_ctx[2], g_ctx[3], g_ctx[4], g_ctx[5], g_ctx[6]); std::exit(1); } } while (0)

static unsigned long long g_spans = 0, g_cells = 0;

// every (workgroup, lane) of the launches over one span: k_emissions_tile (emissions_tile_cell), k_emissions_link (emissions_link),
// the slot launches, k_emissions_emit (emissions_piece_cell), k_emissions_carry and k_emissions_close
static void span(uint64_t w0, uint64_t S, uint32_t W, uint64_t span_max) {
    g_ctx[3] = S; g_ctx[4] = w0; g_ctx[5] = g_ctx[6] = ~0ull;
    EmissionsGeometry G;
    emissions_split(w0, S, W, span_max, &G);
    ++g_spans;
    CHECK(S >= 1 && S <= span_max && span_max <= emissions_span(W) && G.H == (W + 1) / 2 && G.ns == (span_max + 1) * G.H);
    CHECK((uint64_t)(S + 1) * W <= 0xffffffffull);                                         // a u32 label holds every index, and kEmissionsOff is none
    const uint32_t tc = W < kEmissionsTileCols ? W : kEmissionsTileCols;
    CHECK(G.tr >= 1 && G.tr * tc <= kEmissionsTileCells && G.tr * ((tc + 1) / 2) <= kEmissionsTileSlots && (G.tr + 1) * 2 * ((tc + 1) / 2) > kEmissionsTileCells);
    CHECK(kEmissionsTileCells + 7 * kEmissionsTileSlots == kEmissionsLdsWords && kEmissionsLdsWords * 4 <= 64 * 1024);      // the LDS budget
    CHECK(G.n_trows == (S + G.tr - 1) / G.tr && G.n_tcols == (W + 255) / 256 && kEmissionsTileCols % 2 == 0);
    // tiles tile the span; every cell of rows 1 ... S has one lane; every slot of those rows belongs to one tile
    std::vector<uint8_t> cell((size_t)(S + 1) * W, 0), slot((size_t)(S + 1) * G.H, 0), index_taken((size_t)(S + 1) * W, 0);
    for (uint32_t block = 0; block < G.n_trows * G.n_tcols; ++block) {
        g_ctx[5] = block;
        const EmissionsTile T = emissions_tile(G, block);
        CHECK(T.nr >= 1 && T.nr <= G.tr && T.nc >= 1 && T.nc <= kEmissionsTileCols && T.r0 >= 1 && T.r0 + T.nr <= S + 1 && T.b0 + T.nc <= W && T.b0 % kEmissionsTileCols == 0);
        CHECK(T.hc == (T.nc + 1) / 2 && T.nr * T.nc <= kEmissionsTileCells && T.nr * T.hc <= kEmissionsTileSlots);
        std::vector<uint8_t> li_taken(T.nr * T.nc, 0);
        bool ended = false;
        for (uint32_t k = 0; k < kEmissionsTileCells / kEmissionsThreads; ++k)
            for (uint32_t tid = 0; tid < kEmissionsThreads; ++tid) {
                g_ctx[6] = tid;
                const EmissionsCell c = emissions_tile_cell(T, tid, k);
                if (!c.valid) { ended = true; continue; }
                CHECK(!ended || tid > 0);                                                  // a lane's cells are valid for k = 0 ... and then never
                CHECK(c.lr < T.nr && c.lb < T.nc && c.lr * T.nc + c.lb == tid + k * kEmissionsThreads);       // consecutive lanes, consecutive words
                CHECK(c.li < T.nr * T.nc && li_taken[c.li] == 0);
                li_taken[c.li] = 1;
                // the local order is the plane's order, and the local slot is the plane's slot
                CHECK(c.li / T.nc == c.lr && T.nc - 1 - c.li % T.nc == c.lb && emissions_tile_slot(T, c.li) == c.lr * T.hc + c.lb / 2);
                const uint32_t r = T.r0 + c.lr, b = T.b0 + c.lb, at = emissions_index(G, r, b);
                CHECK(at < (S + 1) * W && emissions_row(G, at) == r && emissions_bin(G, at) == b && emissions_slot_of(G, at) == emissions_slot(G, r, b));
                CHECK(emissions_slot(G, r, b) == (uint64_t)r * G.H + T.b0 / 2 + c.lb / 2 && emissions_slot(G, r, b) < G.ns);
                CHECK(cell[(size_t)r * W + b] == 0 && index_taken[at] == 0);
                cell[(size_t)r * W + b] = 1; index_taken[at] = 1; ++g_cells;
                if (c.lb % 2 == 0) { CHECK(slot[emissions_slot(G, r, b)] == 0); slot[emissions_slot(G, r, b)] = 1; }
            }
        for (uint8_t x : li_taken) CHECK(x == 1);
    }
    g_ctx[5] = g_ctx[6] = ~0ull;
    for (size_t i = W; i < cell.size(); ++i) CHECK(cell[i] == 1);
    for (size_t i = G.H; i < slot.size(); ++i) CHECK(slot[i] == 1);
    for (uint32_t b = 0; b < W; ++b) { CHECK(emissions_index(G, 0, b) == W - 1 - b); }      // the virtual row lies below every cell of the span
    // the index order: row ascending, bin descending, so the greatest index of a set of cells is its (last row, lowest bin)
    if (S >= 2 && W >= 2) CHECK(emissions_index(G, 2, 0) > emissions_index(G, 2, 1) && emissions_index(G, 2, W - 1) > emissions_index(G, 1, 0));
    // the link: every border between two tiles, and between the virtual row and the first tile row, is visited once, cell by cell
    std::vector<uint8_t> below((size_t)(S + 1) * W, 0), right((size_t)(S + 1) * W, 0);
    const uint64_t lanes = emissions_link_lanes(G), grid = (lanes + kEmissionsThreads - 1) / kEmissionsThreads;
    for (uint64_t i = 0; i < grid * kEmissionsThreads; ++i) {
        const EmissionsLink l = emissions_link(G, i);
        CHECK(l.valid == (i < lanes));
        if (!l.valid) continue;
        CHECK(l.rb <= S && l.bb < W);
        if (l.ra != l.rb) {
            CHECK(l.rb == l.ra + 1 && l.ba == l.bb && l.ra % G.tr == 0 && below[(size_t)l.ra * W + l.ba] == 0);
            below[(size_t)l.ra * W + l.ba] = 1;
            CHECK(l.has_prev == (l.ba % kEmissionsTileCols != 0));
            if (l.has_prev) CHECK(l.pra == l.ra && l.prb == l.rb && l.pba == l.ba - 1 && l.pbb == l.pba);
        } else {
            CHECK(l.ra >= 1 && l.bb == l.ba + 1 && l.bb % kEmissionsTileCols == 0 && right[(size_t)l.ra * W + l.ba] == 0);
            right[(size_t)l.ra * W + l.ba] = 1;
            CHECK(l.has_prev == ((l.ra - 1) % G.tr != 0));                                 // the row above lies in the same two tiles
            if (l.has_prev) CHECK(l.pra == l.ra - 1 && l.prb == l.pra && l.pba == l.ba && l.pbb == l.bb && l.pra >= 1);
        }
    }
    for (uint32_t r = 0; r <= S; ++r)
        for (uint32_t b = 0; b < W; ++b) {
            CHECK(below[(size_t)r * W + b] == (r < S && r % G.tr == 0 ? 1 : 0));           // row r and r + 1 lie in two tiles (or r is the virtual row)
            CHECK(right[(size_t)r * W + b] == (r >= 1 && b + 1 < W && (b + 1) % kEmissionsTileCols == 0 ? 1 : 0));
        }
    // the emit pieces: every cell of rows 0 ... S - 1 once, in the list's order
    CHECK(G.n_pieces == (S * W + kEmissionsPieceCells - 1) / kEmissionsPieceCells && G.n_pieces <= emissions_pieces_bound(W, span_max));
    uint64_t next = 0;
    for (uint32_t q = 0; q < G.n_pieces; ++q)
        for (uint32_t it = 0; it < kEmissionsPieceCells / kEmissionsThreads; ++it)
            for (uint32_t tid = 0; tid < kEmissionsThreads; ++tid) {
                uint32_t r = 0, b = 0;
                if (!emissions_piece_cell(G, q, it, tid, &r, &b)) continue;
                CHECK((uint64_t)r * W + b == next && r < S);
                ++next;
            }
    CHECK(next == S * W);
}

static void walk(uint32_t W, uint64_t n, const std::vector<uint64_t> &cuts, uint64_t span_cap = ~0ull) {
    g_ctx[0] = W; g_ctx[1] = n; g_ctx[2] = cuts[0];
    uint64_t longest = 0;
    for (uint64_t c : cuts) longest = c > longest ? c : longest;
    uint64_t span_max = emissions_span_max(W, longest);
    if (span_max > span_cap) span_max = span_cap;                                          // a shorter span than the rule's: the same walk, more seams
    CHECK(emissions_workspace(W, span_max) < kEmissionsMaxWorkspace);
    uint64_t g0 = 0, next = 0;
    for (size_t ci = 0; g0 < n; ++ci) {
        const uint64_t bw = cuts[ci % cuts.size()], nw = n - g0 < bw ? n - g0 : bw;
        for (uint64_t a = 0; a < nw; a += span_max) {                                      // as qd_plan_emissions walks a batch
            const uint64_t S = nw - a < span_max ? nw - a : span_max;
            CHECK(g0 + a == next);
            span(g0 + a, S, W, span_max);
            next += S;
        }
        g0 += nw;
    }
    CHECK(next == n);
}

int main() {
    CHECK(emissions_span(1) == (1ull << 20) && emissions_span(128) == 8192 && emissions_span(4096) == 256 && emissions_span(96) == 10922);
    CHECK(emissions_tile_rows(1) == 1024 && emissions_tile_rows(2) == 1024 && emissions_tile_rows(3) == 512 && emissions_tile_rows(96) == 21 && emissions_tile_rows(4096) == 8);
    // the span rule keeps the workspace below the limit for every width up to the limit, whatever the batch
    for (uint32_t W = 1; W <= kEmissionsMaxWidth; ++W) CHECK(emissions_workspace(W, emissions_span_max(W, ~0ull)) < kEmissionsMaxWorkspace);
    Emission a = emissions_cell(3, 5, 9), b = emissions_cell(0, 7, 9), c = emissions_cell(3, 2, 4), ab = a, ba = b, abc, bca;
    emissions_join(ab, b); emissions_join(ba, a);
    CHECK(ab.first == 0 && ab.last == 3 && ab.cells == 2 && ab.lo == 5 && ab.hi == 7 && ab.end_bin == 5 && ab.peak_at == 0 && ab.peak_bin == 7 && ab.flags == 1);
    CHECK(ba.first == ab.first && ba.last == ab.last && ba.end_bin == ab.end_bin && ba.peak_at == ab.peak_at && ba.peak_bin == ab.peak_bin && ba.flags == ab.flags);
    abc = ab; emissions_join(abc, c); bca = b; emissions_join(bca, c); emissions_join(bca, a);
    CHECK(abc.end_bin == 2 && bca.end_bin == 2 && abc.cells == 3 && bca.cells == 3 && abc.lo == 2 && bca.lo == 2 && abc.peak_bin == bca.peak_bin);
    const uint32_t Ws[] = {1, 2, 4, 64, 96, 128, 1024, 2048, 4096};
    for (uint32_t W : Ws) {
        const uint64_t big = W >= 1024 ? 100 : 1500;
        walk(W, 1, {1});
        walk(W, 37, {37});
        walk(W, 37, {1});                                          // one-window batches
        walk(W, 333, {100, 7, 1, 64});                             // ragged
        walk(W, big, {big});
        walk(W, big, {big / 3 + 1});
        walk(W, 101, {101}, 50);                                   // batches longer than a span: a one-window span at the end
        walk(W, 333, {100, 7, 1, 64}, 33);                         // ragged spans in ragged batches
    }
    walk(4096, emissions_span(4096) + 1, {emissions_span(4096) + 1});      // the rule's own span, and one window more
    std::printf("ok: %llu spans, %llu cells\n", g_spans, g_cells);
    return 0;
}
"""


def test_every_lane_of_every_launch(tmp_path):
    """Over W in {1, 2, 4, 64, 96, 128, 1024, 2048, 4096}, ranges in one batch, in one-window batches, in ragged ones and in batches longer
    than a span: tiles tile each span and every cell of it has exactly one lane, consecutive lanes on consecutive words, with the local
    label order equal to the plane's; every slot belongs to one tile; every tile border (and the virtual row's) is visited once by the
    link; the emit pieces walk rows 0 ... S - 1 once in the list's order; the LDS words stay within the stated budget, and the span
    rule keeps the workspace below QD_EMISSIONS_MAX_WORKSPACE for every width up to the limit.  The geometry does not depend on the
    number of compute units: a span is cut into tiles of a fixed size."""
    src = tmp_path / "walk_emissions.cpp"
    src.write_text(WALKER)
    exe = tmp_path / "walk_emissions"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
