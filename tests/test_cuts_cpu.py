"""The cut list without a GPU (include/quadrs_hip.h, "cut list"):
  * qd_cut_of_emission against a Python restatement of its integer arithmetic, digit for digit, on seeded random records and descs and on
    its edges, and every refusal;
  * qd_cuts_geometry's offsets and hull, and every refusal of qd_cuts_run: all validation precedes any device call;
  * the conventions (sign of the shift, bin centre, lowpass width) on the reference alone: the emissions of a stream of tone bursts, cut
    by the oracle's own chain, land on DC at the tones' amplitude;
  * the condition of the strict GPU cases (test_gpu_cuts.py): no NCO multiplier component is ambiguous in any span of STRICT_CUTS, so the
    NCO rule excuses nothing there and the comparison is byte for byte;
  * the host planning (quadrs_amd/csrc/qd_cuts_plan.h) in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from util import ambiguous_components

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 21_000_000
N_STREAM = 1 << 17
SHIFTS = (0, 999_983, 1_000_003, -3_000_017)
SHAPES = ((1, 2), (4, 40), (7, 64), (32, 200))
BIG = (1024, 4096)
SPAN_FLOOR = 40_000


def header_geometry():
    """the kernel's geometry as quadrs_amd/csrc/qd_cuts_plan.h states it: (threads, LDS tile samples)"""
    text = open(os.path.join(ROOT, "quadrs_amd", "csrc", "qd_cuts_plan.h")).read()
    get = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))      # noqa: E731
    return get("kCutsThreads"), get("kCutsTileSamples")


def tile_outputs(D, T):
    threads, samples = header_geometry()
    return min(threads, (samples - T) // D)


def strict_cuts(engine):
    """32 cuts over a 2^17-sample stream at 21 MHz: every (D, T) of SHAPES with 1, 255, 256, 257, one tile + 1 and three tiles + 5 outputs,
    (1024, 4096) with 5, the shifts taken in turn so that every shape meets every shift; spans start past sample 40 000 at odd offsets and
    overlap their neighbours'"""
    rows = []
    for si, (D, T) in enumerate(SHAPES):
        tile = tile_outputs(D, T)
        for ci, count in enumerate((1, 255, 256, 257, tile + 1, 3 * tile + 5)):
            rows.append((SHIFTS[(si + ci) % 4], D, T, count))
    rows += [(s, BIG[0], BIG[1], 5) for s in SHIFTS]
    rows += [(s, 32, 200, 3 * tile_outputs(32, 200) + 5) for s in SHIFTS[:3]] + [(0, 4, 40, 1)]
    cuts = np.zeros(len(rows), dtype=engine.CUT_DTYPE)
    for i, (s, D, T, count) in enumerate(rows):
        first = -(-(SPAN_FLOOR + 1 + 1013 * i) // D) if D < 1024 else 40 + i % 4
        cuts[i] = (s, 150_000 + 20_011 * (i % 5), D, T, first, count)
    assert len(rows) == 32
    return cuts


DEEP_N = (1 << 34) + 12_345


def deep_cuts(engine):
    """[(name, slab base, slab samples, cut)]: a cut near sample 2^33 + 12 345 and one that ends at the end of the described stream of
    2^34 + 12 345 samples; the slab base is a multiple of D"""
    out = []
    D = 7
    T = next(t for t in range(40, 56, 2) if (DEEP_N - t) % D == 0)
    count = 2 * tile_outputs(D, T) + 9
    first = (DEEP_N - T) // D - count
    base = first * D - 3 * D
    out.append(("end", base, DEEP_N - base, np.array((1_000_003, 400_000, D, T, first, count), dtype=engine.CUT_DTYPE)))
    D, T = 4, 40
    first = ((1 << 33) + 12_345) // D + 1
    base = first * D - 5 * D
    count = tile_outputs(D, T) + 3
    out.append(("x33", base, (first * D - base) + count * D + T + 11, np.array((-3_000_017, 900_000, D, T, first, count), dtype=engine.CUT_DTYPE)))
    return out


def span_of(cut):
    a = int(cut["first"]) * int(cut["decimate"])
    return a, a + int(cut["count"]) * int(cut["decimate"]) + int(cut["taps"])


# ------------------------------------------------------------------ the emission arithmetic

def make_desc(engine, sr, n, W, S, shift=None, lowpass=None):
    d = engine._ffi.ChainDesc()
    d.struct_size = C.sizeof(engine._ffi.ChainDesc)
    d.format, d.sample_rate, d.n_samples, d.width, d.stride = 0, sr, n, W, S
    if shift is not None:
        d.has_shift, d.shift_hz = 1, shift
    if lowpass is not None:
        d.has_lowpass, d.lowpass_hz, d.decimate, d.taps = 1, lowpass[0], lowpass[1], lowpass[2]
    return d


def restated(d, fw, e, guard, oversample, pad, taps, max_decimate):
    """the arithmetic of include/quadrs_hip.h in Python's integers: (shift_hz, lowpass_hz, decimate, taps, first, count)"""
    cdiv = lambda a, b: -((-a) // b)      # noqa: E731
    sr, n, W, S = int(d.sample_rate), int(d.n_samples), int(d.width), int(d.stride)
    D0, T0 = (int(d.decimate), int(d.taps)) if d.has_lowpass else (1, 0)
    f0 = int(d.shift_hz) if d.has_shift else 0
    R = sr // D0
    lo, hi = int(e["lo"]), int(e["hi"])
    nu = ((lo + hi - W) * R + W) // (2 * W)
    s = (f0 - nu) % sr
    hs = sr // 2
    if s >= hs:
        s -= sr
    if s <= -hs:
        s = 1 - hs
    lp = max(1, cdiv((hi - lo + 1 + 2 * guard) * R, 2 * W))
    D = min(max(sr // (2 * oversample * lp), 1), max_decimate or 1024)
    T = taps or min(4096, max(40, 8 * D))
    a = (fw + int(e["first"])) * S * D0
    b = min(n, (fw + int(e["last"])) * S * D0 + W * D0 + T0)
    first = max(0, (a - T) // D - pad)
    end = cdiv(max(b - T, 0), D) + pad + cdiv(T - T // 2, D)
    count = max(0, min(end, (n - T) // D) - first)
    return s, lp, D, T, first, count


def emission(engine, first, last, lo, hi):
    e = np.zeros(1, dtype=engine.EMISSION_DTYPE)[0]
    e["first"], e["last"], e["lo"], e["hi"], e["cells"] = first, last, lo, hi, 1
    return e


def held(engine, d, fw, e, guard=1, oversample=2, pad=1, taps=0, max_decimate=0):
    got = engine.cut_of_emission(d, fw, e, engine.cut_rule(guard, oversample, pad, taps, max_decimate))
    want = restated(d, fw, e, guard, oversample, pad, taps, max_decimate)
    assert tuple(int(got[k]) for k in ("shift_hz", "lowpass_hz", "decimate", "taps", "first", "count")) == want, (want, got)
    return got


def test_emission_arithmetic_random(engine):
    rng = np.random.default_rng(20261021)
    seen = set()
    for _ in range(4000):
        W = int(rng.integers(2, 4097))
        sr = int(rng.integers(1000, 1 << int(rng.integers(11, 41))))
        lowpass = (int(rng.integers(1, sr)), int(rng.integers(1, 65)), int(rng.integers(2, 500))) if rng.random() < 0.5 else None
        shift = int(rng.integers(-(sr // 2) + 1, sr // 2)) if rng.random() < 0.5 else None
        S = int(rng.integers(1, 2 * W))
        n = int(rng.integers(1, 1 << int(rng.integers(8, 36))))
        step = S * (lowpass[1] if lowpass else 1)
        n_windows = max(1, n // step)
        first = int(rng.integers(0, n_windows))
        last = first + int(rng.integers(0, max(1, n_windows - first)))
        lo = int(rng.integers(0, W))
        hi = int(rng.integers(lo, W))
        d = make_desc(engine, sr, n, W, S, shift, lowpass)
        got = held(engine, d, int(rng.integers(0, 3)) * int(rng.integers(0, 1000)), emission(engine, first, last, lo, hi),
                   guard=int(rng.integers(0, 4)), oversample=int(rng.integers(1, 5)), pad=int(rng.integers(0, 9)),
                   taps=int(rng.choice([0, 0, 2, 64, 4096])), max_decimate=int(rng.choice([0, 0, 1, 16, 1024])))
        seen.add((int(got["count"]) == 0, int(got["first"]) == 0, shift is None, lowpass is None))
    assert len(seen) >= 12, seen            # zero and non-zero counts, saturated firsts, with and without each stage


def test_emission_arithmetic_edges(engine):
    E = lambda *a: emission(engine, *a)      # noqa: E731
    d = make_desc(engine, 2_000_000, 1 << 17, 64, 64)
    assert int(held(engine, d, 0, E(10, 20, 0, 3))["shift_hz"]) > 0                       # lo = 0: the lowest bins sit at negative frequencies
    assert int(held(engine, d, 0, E(10, 20, 60, 63))["shift_hz"]) < 0                     # hi = W - 1
    whole = held(engine, d, 0, E(10, 20, 0, 63))                                          # every bin: the centre is half a bin below 0 Hz
    assert int(whole["shift_hz"]) == 15_625 and int(whole["decimate"]) == 1
    # a wrap across +-sr/2, both parities of sr: the plan's own shift put the band's edge at DC
    for sr in (2_000_000, 2_000_001):
        for f0 in (sr // 2 - 1, -(sr // 2) + 1, sr // 2 - 1000, -(sr // 2) + 1000):
            dd = make_desc(engine, sr, 1 << 17, 64, 64, shift=f0)
            for lo, hi in ((0, 0), (0, 5), (60, 63), (63, 63), (31, 33)):
                got = held(engine, dd, 0, E(3, 9, lo, hi))
                assert abs(int(got["shift_hz"])) < sr // 2
    assert int(held(engine, make_desc(engine, 2_000_001, 1 << 17, 64, 64, shift=-1_000_000), 0, E(3, 9, 32, 32))["shift_hz"]) == -999_999
    assert int(held(engine, make_desc(engine, 4, 1 << 17, 2, 2, shift=1), 0, E(3, 9, 0, 0))["shift_hz"]) == -1      # s = -hs is pulled to 1 - hs
    # `first` saturating at 0, b clamped at the stream's end, a count that comes out 0
    assert int(held(engine, d, 0, E(0, 4, 20, 22))["first"]) == 0
    assert int(held(engine, d, 0, E(0, 0, 20, 22), pad=1000)["first"]) == 0
    tail = held(engine, d, 0, E(2040, 2047, 20, 22))
    assert (int(tail["first"]) + int(tail["count"])) * int(tail["decimate"]) + int(tail["taps"]) <= 1 << 17
    assert int(held(engine, make_desc(engine, 2_000_000, 30, 4, 4), 0, E(0, 5, 1, 2))["count"]) == 0                 # a stream shorter than the filter
    assert int(held(engine, make_desc(engine, 2_000_000, 1 << 17, 64, 64), 5000, E(0, 5, 1, 2))["count"]) == 0       # windows past the stream
    with_lp = make_desc(engine, 21_000_000, 1 << 20, 128, 32, shift=280_000, lowpass=(200_000, 32, 400))
    held(engine, with_lp, 7, E(10, 40, 50, 70), guard=3, oversample=1, pad=0, taps=256)
    assert int(held(engine, with_lp, 0, E(10, 40, 64, 64), max_decimate=16)["decimate"]) == 16


def test_emission_arithmetic_refusals(engine):
    Q, F = engine, engine._ffi
    d = make_desc(engine, 2_000_000, 1 << 17, 64, 64)
    e = emission(engine, 1, 2, 3, 4)

    def code(desc=d, fw=0, rec=e, rule=None, **kw):
        with pytest.raises(Q.QuadrsError) as err:
            Q.cut_of_emission(desc, fw, rec, rule or Q.cut_rule(**kw))
        return err.value.code
    assert code(oversample=0) == F.ERR_INVALID
    assert code(taps=1) == F.ERR_INVALID
    assert code(rec=emission(engine, 1, 2, 5, 4)) == F.ERR_INVALID                        # lo > hi
    assert code(rec=emission(engine, 1, 2, 5, 64)) == F.ERR_INVALID                       # hi >= W
    assert code(rec=emission(engine, 3, 2, 3, 4)) == F.ERR_INVALID                        # first > last
    bad = Q.cut_rule()
    bad.struct_size = 8
    assert code(rule=bad) == F.ERR_INVALID
    wrong = make_desc(engine, 2_000_000, 1 << 17, 64, 64)
    wrong.struct_size = 100
    assert code(desc=wrong) == F.ERR_INVALID
    assert code(desc=make_desc(engine, 0, 1 << 17, 64, 64)) == F.ERR_INVALID
    assert code(desc=make_desc(engine, 2_000_000, 1 << 17, 64, 0)) == F.ERR_INVALID
    assert code(desc=make_desc(engine, 1 << 48, 1 << 17, 64, 64)) == F.ERR_UNSUPPORTED
    assert code(fw=1 << 60) == F.ERR_UNSUPPORTED
    L = F.lib()
    cut, rule = F.Cut(), Q.cut_rule()
    rec = F.Emission.from_buffer_copy(np.asarray(e).reshape(1).tobytes())
    assert L.qd_cut_of_emission(C.byref(d), 0, C.byref(rec), None, C.byref(cut)) == F.ERR_INVALID
    assert L.qd_cut_of_emission(None, 0, C.byref(rec), C.byref(rule), C.byref(cut)) == F.ERR_INVALID
    assert L.qd_cut_of_emission(C.byref(d), 0, C.byref(rec), C.byref(rule), C.byref(cut)) == F.OK
    held(engine, make_desc(engine, (1 << 48) - 1, 1 << 17, 64, 64), 0, e, oversample=1)   # the largest rate taken


# ------------------------------------------------------------------ geometry and refusals

def test_geometry_offsets_and_hull(engine):
    cuts = strict_cuts(engine)
    offs, lo, count = engine.cuts_geometry(SR, N_STREAM, cuts)
    assert offs.tolist() == np.concatenate([[0], np.cumsum(cuts["count"])]).tolist()
    spans = [span_of(c) for c in cuts]
    assert (lo, lo + count) == (min(a for a, _ in spans), max(b for _, b in spans))
    assert lo >= SPAN_FLOOR and lo + count <= SPAN_FLOOR + (1 << 16)
    assert engine.cuts_geometry(SR, N_STREAM, cuts[:0])[1:] == (0, 0)
    empty = cuts[:3].copy()
    empty["count"] = 0
    empty["first"] = 1 << 40                                                              # a cut without outputs has no span to check
    offs, lo, count = engine.cuts_geometry(SR, N_STREAM, empty)
    assert offs.tolist() == [0, 0, 0, 0] and (lo, count) == (0, 0)
    L = engine._ffi.lib()
    a, b = C.c_uint64(), C.c_uint64()
    assert L.qd_cuts_geometry(SR, N_STREAM, cuts.ctypes.data_as(C.c_void_p), cuts.size, None, C.byref(a), C.byref(b)) == 0      # offsets may be NULL


def test_every_refusal_precedes_the_device(engine):
    Q, F = engine, engine._ffi
    good = strict_cuts(engine)[:4]
    _, lo, count = Q.cuts_geometry(SR, N_STREAM, good)
    slab = np.zeros(count * 8, dtype=np.uint8)
    total = int(good["count"].sum())

    def code(cuts, fmt=0, n=N_STREAM, src_first=lo, src_count=count, src=slab, out=None, needle=None):
        before = None if out is None else out.copy()
        with pytest.raises(Q.QuadrsError) as err:
            Q.cuts_run(fmt, SR, n, src, cuts, src_first=src_first, src_count=src_count, out=out)
        if before is not None:
            assert (out == before).all()
        if needle is not None:
            assert needle in str(err.value), err.value
        return err.value.code

    def with_(k, **kw):
        c = good.copy()
        for name, v in kw.items():
            c[name][k] = v
        return c
    assert code(with_(2, decimate=0), needle="cut 2") == F.ERR_PANIC
    assert code(with_(1, taps=1), needle="cut 1") == F.ERR_PANIC
    assert code(with_(3, shift_hz=SR // 2), needle="cut 3") == F.ERR_PANIC
    assert code(with_(3, shift_hz=-(SR // 2))) == F.ERR_PANIC
    assert code(with_(0, decimate=1025), needle="cut 0") == F.ERR_UNSUPPORTED
    assert code(with_(0, taps=4098)) == F.ERR_UNSUPPORTED
    assert code(with_(0, count=(1 << 31) + 1)) == F.ERR_UNSUPPORTED
    assert code(with_(1, taps=1, decimate=1025)) == F.ERR_PANIC                            # within one cut: the order the header states
    both = with_(3, decimate=0)
    both["taps"][1] = 5000
    assert code(both, needle="cut 1") == F.ERR_UNSUPPORTED                                # list order: the first offender is named
    # a cut is one full block: QD_ERR_SHORT, and no output byte is touched
    out = np.full(2 * total, 7.5, dtype=np.float32)
    short = with_(3, first=(N_STREAM - int(good["taps"][3])) // int(good["decimate"][3]) - int(good["count"][3]) + 1)
    assert code(short, out=out, src_first=0, src_count=N_STREAM, src=np.zeros(N_STREAM * 8, dtype=np.uint8), needle="cut 3") == F.ERR_SHORT
    assert code(good, n=span_of(good[0])[1] - 1, out=out) == F.ERR_SHORT
    assert code(with_(0, first=1 << 62), out=out) == F.ERR_SHORT
    # spans outside the slab
    assert code(good, src_first=lo + 1, needle="cut") == F.ERR_INVALID
    assert code(good, src_count=count - 1) == F.ERR_INVALID
    assert code(good, fmt=4) == F.ERR_INVALID and code(good, fmt=-1) == F.ERR_INVALID
    L = F.lib()
    ptr = good.ctypes.data_as(C.c_void_p)
    args = (0, SR, N_STREAM, slab.ctypes.data_as(C.c_void_p), 0, lo, count, ptr, good.size, out.ctypes.data_as(C.c_void_p), 0, None, None)
    def but(**kw):
        a = list(args)
        for at, v in kw.items():
            a[int(at[1:])] = v
        return L.qd_cuts_run(*a)
    assert but(_4=3) == F.ERR_INVALID and but(_10=-1) == F.ERR_INVALID                    # unknown memory kinds
    for at in ("_3", "_7", "_9"):                                                         # NULL src, cuts, out
        assert but(**{at: None}) == F.ERR_INVALID, at
    assert (out == 7.5).all()
    # nothing to write is fine, without a device and without buffers
    assert but(_8=0, _7=None, _3=None, _9=None) == F.OK
    zero = good.copy()
    zero["count"] = 0
    assert Q.cuts_run(0, SR, N_STREAM, slab, zero, src_first=lo, src_count=count)[0].shape == (0, 2)


# ------------------------------------------------------------------ the conventions, on the reference alone

BURST_SR = 2_000_000
BURST_TONES = (300_000, -450_000, 123_457, -61_001, 700_000)
_BURSTS = {}


def burst_stream():
    """2^17 samples at 2 MHz: complex noise of sigma 0.01 and five tone bursts of amplitude 0.5, one after the other (read-only)"""
    if "x" not in _BURSTS:
        rng = np.random.default_rng(20261021)
        n = 1 << 17
        z = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        t = np.arange(n)
        for k, f in enumerate(BURST_TONES):
            a = 6_000 + 25_000 * k
            z[a:a + 16_384] += 0.5 * np.exp(2j * np.pi * f / BURST_SR * t[a:a + 16_384])
        x = np.stack([z.real, z.imag], axis=1).astype(np.float32)
        x.setflags(write=False)
        _BURSTS["x"] = x
    return _BURSTS["x"]


def test_burst_stream_cuts_land_on_dc(engine, oracle):
    x = burst_stream()
    n = x.shape[0]
    norms, _ = oracle.Chain.from_bytes(x.tobytes(), 0, BURST_SR).spark_fft(64, 64, want_codes=False)
    records, found = engine.emissions_of(norms, np.full(64, 4.0, dtype=np.float32), min_cells=8)
    assert found == records.size == len(BURST_TONES), records
    d = make_desc(engine, BURST_SR, n, 64, 64)
    for r in records:
        cut = engine.cut_of_emission(d, 0, r, engine.cut_rule(1, 2, 1))
        assert int(cut["decimate"]) >= 2 and int(cut["count"]) > 256, cut
        ch = oracle.Chain.from_bytes(x.tobytes(), 0, BURST_SR)
        if int(cut["shift_hz"]):
            ch = ch.shift(int(cut["shift_hz"]))
        got, y = ch.lowpass(int(cut["lowpass_hz"]), int(cut["decimate"]), int(cut["taps"])).read_at(int(cut["first"]), int(cut["count"]))
        assert got == int(cut["count"])
        q = y.shape[0] // 4
        z = y[q:q + 64, 0].astype(np.float64) + 1j * y[q:q + 64, 1]
        peak = int(np.argmax(np.abs(np.fft.fftshift(np.fft.fft(z)))))
        assert abs(peak - 32) <= 2, (r, cut, peak)
        assert np.abs(z).mean() > 0.4, (r, cut, np.abs(z).mean())


# ------------------------------------------------------------------ the condition of the strict GPU cases

def test_strict_spans_hold_no_ambiguous_multiplier(engine, oracle):
    cuts = strict_cuts(engine)
    assert set(cuts["shift_hz"].tolist()) == set(SHIFTS)
    assert {(int(c["decimate"]), int(c["taps"])) for c in cuts} == set(SHAPES) | {BIG}
    for D, T in SHAPES:
        tile = tile_outputs(D, T)
        counts = {int(c["count"]) for c in cuts if int(c["decimate"]) == D and int(c["taps"]) == T}
        assert {1, 255, 256, 257, tile + 1, 3 * tile + 5} <= counts, (D, T, counts)
        assert {int(c["shift_hz"]) for c in cuts if int(c["decimate"]) == D} == set(SHIFTS)
    assert tile_outputs(*BIG) == 5                                                        # a handful of outputs per tile: correct, not tuned
    for c in list(cuts) + [d[3] for d in deep_cuts(engine)]:
        a, b = span_of(c)
        assert a > SPAN_FLOOR and int(c["taps"]) % 2 == 0
        if int(c["shift_hz"]):
            assert ambiguous_components(oracle.shift_ratio(int(c["shift_hz"]), SR), a, b) == [], c
    for name, base, count, c in deep_cuts(engine):
        a, b = span_of(c)
        assert base % int(c["decimate"]) == 0 and base <= a and b <= base + count <= DEEP_N and count * 8 <= 1 << 20
        assert (name == "end") == (b == DEEP_N) and a > 1 << 33
    assert ambiguous_components(oracle.shift_ratio(999_983, SR), 0, 1) != []              # sample 0 is always ambiguous: no strict span starts there


# ------------------------------------------------------------------ the host planning under the sanitizers

def test_host_planning_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "cuts_host_check")
    src = os.path.join(ROOT, "scripts", "cuts_host_check.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-Wall",
                         "-Wextra", "-o", exe, src], capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()
    r = subprocess.run([exe, "60"], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"cuts_host_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
