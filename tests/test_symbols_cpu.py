"""The symbol list without a GPU (include/quadrs_hip.h, "symbol list"; quadrs_amd/csrc/qd_symbols_plan.h):
  * qd_symbols_geometry against the two counting rules;
  * every refusal, its code, the order of the checks and the index of the first offender - all ahead of any device call;
  * the host planning (windows, offsets, tiles, groups) under ASan and UBSan as a stand-alone program;
  * the conditions of the GPU tests' streams, held on the oracle alone: both digits and both marks occur often enough in every case,
    the tie-balanced segments are balanced, a NaN sample gives 1 in both sinks, and the oracle's own chain recovers the planted bits of
    the end-to-end capture with the parameters the GPU test uses."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import symbols_util as U
from test_cuts_cpu import make_desc
from util import digits_from_norms, exact_ties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_SHARE = 0.10


def seg_array(engine, rows):
    return np.array(rows, dtype=engine.SEGMENT_DTYPE)


# ------------------------------------------------------------------ geometry

@pytest.mark.parametrize("W", [2, 64, 4096])
def test_geometry_follows_the_two_counting_rules(engine, W):
    for S in (1, W // 2, W, W + 3):
        counts = [0, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 3 * W + 5]
        segs = seg_array(engine, [(17 * k + 1, c) for k, c in enumerate(counts)])
        for epi in (engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
            offs = engine.symbols_geometry(engine.symbols_desc(epi, W, S), segs)
            want = [U.windows_of(epi, c, W, S) for c in counts]
            assert offs.dtype == np.uint64 and offs[0] == 0 and np.diff(offs.astype(np.int64)).tolist() == want, (W, S, epi, offs, want)
            # the rules as the reference runs them, as loops
            for c, w in zip(counts, want):
                if c > W:
                    loop = len(range(0, (c - W) // S)) if epi == engine.EPI_BUCKET2_U8 else len(range(0, c - W, S))
                    assert loop == w, (c, W, S, epi)
                else:
                    assert w == 0                                          # the stated departure: a short segment has no windows
    assert engine.symbols_geometry(engine.symbols_desc(engine.EPI_MARK_U8, W), seg_array(engine, [])).tolist() == [0]


def test_every_refusal_precedes_the_device(engine):
    Q, F = engine, engine._ffi
    L = F.lib()
    good = seg_array(engine, [(1, 300), (7, 64), (100, 1000), (5, 65)])
    iq = np.zeros((2000, 2), dtype=np.float32)

    def desc(**kw):
        d = Q.symbols_desc(Q.EPI_MARK_U8, 64, 16)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def code(d, segs=good, needle=None, run=False, out=None):
        before = None if out is None else out.copy()
        with pytest.raises(Q.QuadrsError) as err:
            Q.symbols_run(d, iq, segs, out=out) if run else Q.symbols_geometry(d, segs)
        if before is not None:
            assert (out == before).all()
        if needle is not None:
            assert needle in str(err.value), err.value
        return err.value.code

    for run in (False, True):
        assert code(desc(struct_size=40), run=run) == F.ERR_INVALID
        assert code(desc(epilogue=Q.EPI_NORMS_F32), run=run) == F.ERR_INVALID
        assert code(desc(epilogue=Q.EPI_GLYPH_U8), run=run) == F.ERR_INVALID
        assert code(desc(stride=0), run=run) == F.ERR_INVALID
        assert code(desc(windowing=2), run=run) == F.ERR_INVALID and code(desc(windowing=-1), run=run) == F.ERR_INVALID
        assert code(desc(width=48), run=run, needle="power-of-two") == F.ERR_PANIC
        assert code(desc(width=0), run=run) == F.ERR_PANIC
        assert code(desc(width=8192), run=run) == F.ERR_UNSUPPORTED
        assert code(desc(width=12288), run=run) == F.ERR_PANIC                                # no power of two: the plan's code comes first
        # the order within the desc: struct_size, epilogue, stride, windowing, width
        assert code(desc(epilogue=0, stride=0, width=48), run=run) == F.ERR_INVALID
        assert code(desc(stride=0, width=48), run=run) == F.ERR_INVALID
        assert code(desc(windowing=3, width=8192), run=run) == F.ERR_INVALID
        big = good.copy()
        big["count"][2] = (1 << 31) + 1
        assert code(desc(), big, needle="segment 2", run=run) == F.ERR_UNSUPPORTED
        assert code(desc(width=48), big, run=run) == F.ERR_PANIC                              # the desc before the segments
    # the plan's own code and words for the width
    with pytest.raises(Q.QuadrsError) as plan_err:
        Q.Plan(Q.FMT_CF32, U.SR, 1 << 12, width=48, stride=16, epilogue=Q.EPI_MARK_U8)
    with pytest.raises(Q.QuadrsError) as sym_err:
        Q.symbols_geometry(desc(width=48), good)
    assert plan_err.value.code == sym_err.value.code == F.ERR_PANIC and str(plan_err.value) == str(sym_err.value)
    ok = good.copy()
    ok["count"][2] = 1 << 31
    assert int(Q.symbols_geometry(desc(), ok)[-1]) > 0                                        # 2^31 itself is admissible
    # a segment past the buffer: QD_ERR_SHORT, list order, and no output byte is touched
    out = np.full(4096, 0x5A, dtype=np.uint8)
    far = good.copy()
    far["first"][1] = 2000 - 63
    far["first"][3] = 1 << 62
    assert code(desc(), far, needle="segment 1", run=True, out=out) == F.ERR_SHORT
    far["count"][0] = (1 << 31) + 1                                                           # list order across the two segment checks
    assert code(desc(), far, needle="segment 0", run=True, out=out) == F.ERR_UNSUPPORTED
    wrap = good.copy()
    wrap["first"][0] = (1 << 64) - 100                                                        # first + count wraps: still past the buffer
    assert code(desc(), wrap, needle="segment 0", run=True, out=out) == F.ERR_SHORT
    assert int(Q.symbols_geometry(desc(), wrap)[-1]) > 0                                      # the geometry has no buffer to hold it against
    # the raw call: memory kinds and NULL pointers
    d = desc()
    ptr = good.ctypes.data_as(C.c_void_p)
    args = (C.byref(d), iq.ctypes.data_as(C.c_void_p), 0, 2000, ptr, good.size, out.ctypes.data_as(C.c_void_p), 0, None)

    def but(**kw):
        a = list(args)
        for at, v in kw.items():
            a[int(at[1:])] = v
        return L.qd_symbols_run(*a)
    assert but(_2=3) == F.ERR_INVALID and but(_7=-1) == F.ERR_INVALID
    for at in ("_0", "_1", "_4", "_6"):                                                       # NULL desc, in, segments, out
        assert but(**{at: None}) == F.ERR_INVALID, at
    assert but(_3=1099) == F.ERR_SHORT and b"segment 2" in L.qd_last_error()                 # n_in one short of segment 2's end
    assert (out == 0x5A).all()
    # nothing to write is fine, without a device and without buffers
    assert but(_5=0, _4=None, _1=None, _6=None) == F.OK
    short = seg_array(engine, [(0, 64), (3, 10), (9, 0)])
    assert but(_4=short.ctypes.data_as(C.c_void_p), _5=3, _1=None, _6=None) == F.OK
    assert L.qd_symbols_geometry(C.byref(d), ptr, good.size, None) == F.OK                    # offsets may be NULL
    assert L.qd_symbols_geometry(None, ptr, good.size, None) == F.ERR_INVALID
    assert L.qd_symbols_geometry(C.byref(d), None, 2, None) == F.ERR_INVALID


def test_cuts_symbols_refusals_precede_the_device(engine):
    Q, F = engine, engine._ffi
    from test_cuts_cpu import N_STREAM, strict_cuts
    from test_cuts_cpu import SR as CUT_SR
    cuts = strict_cuts(engine)[:4]
    _, lo, count = Q.cuts_geometry(CUT_SR, N_STREAM, cuts)
    slab = np.zeros(count * 8, dtype=np.uint8)
    out = np.full(4096, 0x5A, dtype=np.uint8)

    def code(c, d, needle=None, **kw):
        with pytest.raises(Q.QuadrsError) as err:
            Q.cuts_symbols(0, CUT_SR, N_STREAM, slab, c, d, src_first=lo, src_count=count, out=out, **kw)
        assert (out == 0x5A).all()
        if needle is not None:
            assert needle in str(err.value), err.value
        return err.value.code
    good = Q.symbols_desc(Q.EPI_BUCKET2_U8, 16, 16)
    bad_cut = cuts.copy()
    bad_cut["decimate"][2] = 0
    assert code(bad_cut, good, needle="cut 2") == F.ERR_PANIC
    assert code(bad_cut, Q.symbols_desc(Q.EPI_BUCKET2_U8, 48, 16), needle="cut 2") == F.ERR_PANIC            # the cuts' validation first
    assert code(cuts, Q.symbols_desc(Q.EPI_BUCKET2_U8, 48, 16), needle="power-of-two") == F.ERR_PANIC
    assert code(cuts, Q.symbols_desc(Q.EPI_NORMS_F32, 16, 16)) == F.ERR_INVALID
    assert code(cuts, Q.symbols_desc(Q.EPI_BUCKET2_U8, 8192, 16)) == F.ERR_UNSUPPORTED
    largest = int(cuts["count"].max())
    k = int(np.argmax(cuts["count"]))
    assert code(cuts, Q.symbols_desc(Q.EPI_BUCKET2_U8, 16, 16, iq_bytes=8 * largest - 1), needle=f"cut {k}") == F.ERR_UNSUPPORTED
    assert "iq_bytes" in F.lib().qd_last_error().decode()
    assert code(cuts, good, chunk_bytes=1000) == F.ERR_INVALID                                              # qd_cuts_run's options check


# ------------------------------------------------------------------ the host planning under the sanitizers

def test_host_planning_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "symbols_host_check")
    src = os.path.join(ROOT, "scripts", "symbols_host_check.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-Wall",
                         "-Wextra", "-o", exe, src], capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()
    r = subprocess.run([exe, "100"], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"symbols_host_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_the_header_states_the_geometry_the_checks_use():
    import re
    text = open(os.path.join(ROOT, "quadrs_amd", "csrc", "qd_symbols_plan.h")).read()
    get = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))      # noqa: E731
    assert get("kSymThreads") == 256 and get("kSymSliceSamples") == 2048
    assert 2 * 4 * get("kSymSliceSamples") * 8 <= 160 * 1024                                  # two workgroups share a CU's LDS
    assert 2 * 4096 * 8 <= 4 * get("kSymSliceSamples") * 8                                    # two waves hold a 4096-point window each


# ------------------------------------------------------------------ the conditions of the GPU tests' streams, on the oracle alone

@pytest.mark.parametrize("W", U.WIDTHS)
def test_both_values_occur_in_every_case(oracle, W):
    for S in U.strides(W):
        segs = U.segments(W, S)
        assert 40 <= segs.size <= 48 and (segs["first"] % 2 == 1).all()
        for epi in (U.BUCKET, U.MARK):
            refs = U.references(oracle, epi, W, S)
            assert [r.size for r in refs] == [U.windows_of(epi, int(c), W, S) for c in segs["count"]]
            every = np.concatenate(refs)
            assert 0 < every.size <= 21_000, (W, S, every.size)
            share = float(every.mean())
            print(f"W={W} S={S} epi={epi}: {every.size} windows, share of ones {share:.3f}")
            assert MIN_SHARE <= share <= 1 - MIN_SHARE, (W, S, epi, share)


def test_a_nan_sample_gives_one_in_both_sinks(oracle):
    x = U.buffer(oracle)
    assert np.isnan(x[U.NAN_AT, 0]) and np.isnan(x).sum() == 1
    for W, S in ((2, 1), (16, 8), (64, 67), (1024, 1024)):
        segs = U.segments(W, S)
        k = 40                                                                # the segment laid across the NaN sample
        f, c = int(segs["first"][k]), int(segs["count"][k])
        assert f <= U.NAN_AT < f + c
        for epi in (U.BUCKET, U.MARK):
            ref = U.references(oracle, epi, W, S)[k]
            sees = [r for r in range(ref.size) if f + r * S <= U.NAN_AT < f + r * S + W]
            assert sees and (ref[sees] == 1).all(), (W, S, epi, sees, ref[sees])


@pytest.mark.parametrize("W", U.BALANCED_WIDTHS)
def test_the_tie_balanced_segments_are_balanced(oracle, W):
    """util.balanced_real_stream's claim on the segment as it lies in the buffer: real samples, in windows 0 ... 11 the odd-indexed
    samples sum to zero up to f32 rounding, and there the digit hangs on the order of the half sums - other orders change digits"""
    x = U.buffer(oracle)
    first, count = U.balanced_at(W)
    seg = x[first:first + count]
    assert first % 2 == 1 and not seg[:, 1].any()
    odd = np.array([abs(float(seg[r * W:(r + 1) * W][1::2, 0].astype(np.float64).sum())) for r in range(count // W - 1)])
    assert np.median(odd[U.N_BALANCED:]) > 1000 * odd[:U.N_BALANCED].max(), odd
    ch = oracle.Chain.from_bytes(seg.tobytes(), 0, U.SR)
    levels = ch.freq_levels(W, W)
    norms, _ = ch.spark_fft(W, W, max_windows=levels.size, want_codes=False)
    assert np.array_equal(digits_from_norms(norms, "sequential"), levels)
    bal = np.arange(U.N_BALANCED)
    changed = {o: int((digits_from_norms(norms, o) != levels)[bal].sum()) for o in ("pairwise", "f64", "reversed")}
    print(f"W={W}: digits {levels[bal].tolist()}, exact ties {int(exact_ties(norms)[bal].sum())}, changed by order {changed}")
    assert sum(changed.values()) > 0, changed
    # and it is one of the case's segments, whole, wherever the stride is the width
    segs = U.segments(W, W)
    assert any(int(f) == first and int(c) == count for f, c in segs)


def e2e_cuts(engine, oracle):
    """the cuts of the end-to-end capture's emissions, found on the oracle's norms by the CPU twin of Plan.emissions"""
    x = U.e2e_stream()
    norms, _ = oracle.Chain.from_bytes(x.tobytes(), 0, U.E2E_SR).spark_fft(U.E2E_W, U.E2E_W, want_codes=False)
    records, found = engine.emissions_of(norms, np.full(U.E2E_W, U.E2E_LEVEL, dtype=np.float32), min_cells=8)
    d = make_desc(engine, U.E2E_SR, x.shape[0], U.E2E_W, U.E2E_W)
    return records, found, np.array([engine.cut_of_emission(d, 0, r, engine.cut_rule(*U.E2E_RULE)) for r in records], dtype=engine.CUT_DTYPE)


def test_the_oracle_recovers_the_planted_bits(engine, oracle):
    x = U.e2e_stream()
    records, found, cuts = e2e_cuts(engine, oracle)
    assert found == records.size == len(U.E2E_BINS), records
    for r, b in zip(records, U.E2E_BINS):
        assert (int(r["lo"]), int(r["hi"])) == (b - 1, b + 1), (r, b)                        # symmetric about the packet's centre
    for cut, bits, b in zip(cuts, U.e2e_bits(), U.E2E_BINS):
        assert int(cut["shift_hz"]) == -(b - U.E2E_W // 2) * U.E2E_SR // U.E2E_W, cut
        ch = oracle.Chain.from_bytes(x.tobytes(), 0, U.E2E_SR).shift(int(cut["shift_hz"])).lowpass(int(cut["lowpass_hz"]), int(cut["decimate"]), int(cut["taps"]))
        got, y = ch.read_at(int(cut["first"]), int(cut["count"]))
        assert got == int(cut["count"])
        digits = oracle.Chain.from_bytes(y.tobytes(), 0, U.E2E_SR // int(cut["decimate"])).freq_levels(U.E2E_SINK_W, U.E2E_SINK_W)
        err, found_bits = engine.bits_scan(digits, U.e2e_scale(cut))
        print(f"bin {b}: D {int(cut['decimate'])} T {int(cut['taps'])} count {int(cut['count'])}, {digits.size} digits, scale {U.e2e_scale(cut):.3f}, error {err:.2f}")
        assert found_bits.tolist() == bits.tolist(), (b, found_bits.tolist(), bits.tolist())
