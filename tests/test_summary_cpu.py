"""The level summary's host half (include/quadrs_hip.h, "level summary"): qd_summary's layout, qd_summary_fold against a numpy
restatement, merge == whole, qd_summary_quantile against a sorted array, and the error codes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32
INF = F32(np.inf)


def np_summary(norms):
    """The summary of norms rows (n, W), restated with numpy: a dict of the fields.  NaN is ignored by the folds (f32::max / f32::min,
    src/ffts.rs:101-107) and counted; every other value goes to hist[bits(|x|) >> 20]."""
    a = np.ascontiguousarray(norms, dtype=F32)
    n, W = a.shape
    nan = np.isnan(a)
    peak = np.where(nan, F32(0), a).max(axis=0, initial=F32(0)).astype(F32)
    floor = np.where(nan, INF, a).min(axis=0, initial=INF).astype(F32)
    buckets = (a.view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(20)
    hist = np.bincount(buckets[~nan].ravel(), minlength=2048).astype(np.uint64)
    return dict(width=W, n_windows=n, n_nan=int(nan.sum()), min=floor.min(initial=INF), max=peak.max(initial=F32(0)), hist=hist,
                peak=peak, floor=floor)


def same(s, ref):
    """a quadrs_amd Summary equals an np_summary dict, bit for bit"""
    assert (s.width, s.n_windows, s.n_nan) == (ref["width"], ref["n_windows"], ref["n_nan"])
    assert F32(s.min).tobytes() == F32(ref["min"]).tobytes() and F32(s.max).tobytes() == F32(ref["max"]).tobytes()
    assert np.array_equal(s.hist, ref["hist"])
    assert s.peak.tobytes() == ref["peak"].tobytes() and s.floor.tobytes() == ref["floor"].tobytes()
    assert int(s.hist.sum()) + s.n_nan == s.n_windows * s.width                 # the invariant
    assert not s.hist[2041:].any()
    return True


def edge_rows():
    """rows of 8 holding 0, a subnormal, FLT_MAX, +inf, NaNs of both signs, and bucket edges with their predecessors"""
    bits = [0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF]
    for j in (1, 2, 7, 8, 9, 1015, 1016, 1017, 2039, 2040):                     # exact bucket edges j << 20 and nextafter below them
        bits += [j << 20, (j << 20) - 1]
    bits += [0x3F800000, 0x3DA3D70A, 0x3A83126F]                                # 1.0, 0.08, 0.001
    while len(bits) % 8:
        bits.append(0x3F000000)
    return np.array(bits, dtype=np.uint32).view(F32).reshape(-1, 8)


@pytest.fixture(scope="module")
def cupboard_norms(oracle, cupboard):
    return oracle.Chain.from_bytes(cupboard, oracle.FMT_CF32, 400).spark_fft(4, 2, want_codes=False)[0]


@pytest.fixture(scope="module")
def fsk_norms(oracle, fsk):
    return oracle.Chain.from_bytes(fsk, oracle.FMT_CF32, 21_000_000).lowpass(2_000_000, 16, 40).spark_fft(128, 128, want_codes=False)[0]


def test_struct_layout(engine):
    from quadrs_amd import _ffi
    S = _ffi.Summary
    assert C.sizeof(S) == 4 + 4 + 8 + 8 + 4 + 4 + 2048 * 8
    assert [(getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_] == [(0, 4), (4, 4), (8, 8), (16, 8), (24, 4), (28, 4), (32, 16384)]
    s = engine.summary_init(5)
    assert s.c.struct_size == C.sizeof(S) and s.width == 5 and s.n_windows == 0 and s.n_nan == 0
    assert s.max == 0 and s.min == INF and not s.hist.any()
    assert (s.peak == 0).all() and (s.floor == INF).all()


def test_fold_matches_numpy(engine, cupboard_norms, fsk_norms):
    for norms in (cupboard_norms, fsk_norms, edge_rows()):
        assert norms.shape[0] > 1
        assert same(engine.summary_fold(norms), np_summary(norms))
    e = engine.summary_fold(edge_rows())
    assert e.n_nan == 4 and e.hist[2040] == 2 and e.max == INF and e.min == 0
    assert e.hist[0] == 3 and e.hist[7] == 3      # bits 0, 1 and (1 << 20) - 1; the largest subnormal shares bucket 7 with 7 << 20 and (8 << 20) - 1


def test_fold_without_arrays(engine, fsk_norms):
    from quadrs_amd import _ffi
    L = _ffi.lib()
    s = _ffi.Summary()
    assert L.qd_summary_init(C.byref(s), None, None, 128) == 0
    a = np.ascontiguousarray(fsk_norms)
    assert L.qd_summary_fold(C.byref(s), None, None, a.ctypes.data_as(C.c_void_p), a.shape[0]) == 0
    ref = np_summary(a)
    assert s.n_windows == a.shape[0] and F32(s.max) == ref["max"] and F32(s.min) == ref["min"]
    assert np.array_equal(np.ctypeslib.as_array(s.hist), ref["hist"])


@pytest.mark.parametrize("cuts", [(1,), (7,), (3, 4), (1, 9)])
def test_merge_of_parts_is_the_whole(engine, fsk_norms, cuts):
    norms = fsk_norms[:12]
    whole = engine.summary_fold(norms)
    edges = [0, *cuts, norms.shape[0]]
    merged = engine.summary_init(norms.shape[1])
    for a, b in zip(edges[:-1], edges[1:]):
        engine.summary_merge(merged, engine.summary_fold(norms[a:b]))
    assert merged.tobytes() == whole.tobytes()
    rows = edge_rows()                             # NaN, inf and zero split across the parts
    whole = engine.summary_fold(rows)
    for cut in range(1, rows.shape[0]):
        m = engine.summary_fold(rows[:cut]).merge(engine.summary_fold(rows[cut:]))
        assert m.tobytes() == whole.tobytes()


@pytest.mark.parametrize("q", [0.0, 0.5, 0.999, 1.0])
def test_quantile(engine, cupboard_norms, fsk_norms, q):
    for norms in (cupboard_norms, fsk_norms, edge_rows()):
        s = engine.summary_fold(norms)
        vals = np.sort(norms[~np.isnan(norms)].ravel())
        r = max(1, int(np.ceil(q * vals.size)))
        v = vals[r - 1]                            # the r-th smallest
        lo, hi = s.quantile(q)
        j = int(lo.view(np.uint32)) >> 20
        assert int(lo.view(np.uint32)) == j << 20
        assert hi.view(np.uint32) == (0x7F800000 if j >= 2040 else (j + 1) << 20)
        assert (lo <= v < hi) or (j == 2040 and v == INF)


def test_error_codes(engine):
    from quadrs_amd import _ffi
    a, b = engine.summary_init(4), engine.summary_init(8)
    with pytest.raises(engine.QuadrsError) as e:
        engine.summary_merge(a, b)
    assert e.value.code == _ffi.ERR_INVALID
    with pytest.raises(engine.QuadrsError) as e:
        a.quantile(0.5)                            # N == 0
    assert e.value.code == _ffi.ERR_INVALID
    a.fold(np.full((1, 4), np.nan, dtype=F32))     # only NaNs: still N == 0
    assert a.n_nan == 4
    with pytest.raises(engine.QuadrsError) as e:
        a.quantile(0.5)
    assert e.value.code == _ffi.ERR_INVALID
    a.fold(np.ones((1, 4), dtype=F32))
    for q in (-0.01, 1.01, float("nan")):
        with pytest.raises(engine.QuadrsError) as e:
            a.quantile(q)
        assert e.value.code == _ffi.ERR_INVALID
    assert a.quantile(1.0) == (F32(1.0), F32(np.uint32(0x3F900000).view(F32)))
    bad = _ffi.Summary()                           # struct_size never set
    assert _ffi.lib().qd_summary_fold(C.byref(bad), None, None, None, 0) == _ffi.ERR_INVALID


def test_cupboard_levels_bracket_the_readme_range(engine, cupboard_norms):
    """The README's OOK walk-through runs this file with -range 0.001:0.01 ("adjusted the range so it was blank when the radio was
    off").  The oracle's norms agree: the largest is below the upper bound 0.01 and the median's bucket lies below the lower bound
    0.001 (checked on the oracle's norms with numpy: max 0.0031573..., median 0.00018159...)."""
    s = engine.summary_fold(cupboard_norms)
    assert F32(cupboard_norms.max()) == s.max and np.median(cupboard_norms) < 0.001
    assert s.max < F32(0.01)
    assert s.quantile(0.5)[1] <= F32(0.001)
