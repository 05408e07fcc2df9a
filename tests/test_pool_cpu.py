"""The peak-hold rows' host half (include/quadrs_hip.h, "peak-hold rows"): qd_pool_init, qd_pool_fold against a numpy fold, parts ==
whole at every split point, pool >= n == the summary's peak / floor, and the error codes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32
INF = F32(np.inf)
N = 37
WIDTHS = [1, 2, 4, 64, 1024]
POOLS = [1, 2, 3, 7, 37, 50]


def np_pool(norms, pool, at=0):
    """rows (at + i) // pool of the fold of norms rows (n, W), restated with numpy: np.fmax / np.fmin ignore a NaN operand as f32::max /
    f32::min do; identities 0.0 / +inf.  The windows in front of `at` contribute nothing."""
    a = np.ascontiguousarray(norms, dtype=F32)
    n, W = a.shape
    R = -(-(at + n) // pool)
    peak, floor = np.zeros((R, W), dtype=F32), np.full((R, W), INF, dtype=F32)
    for r in range(R):
        lo, hi = max(r * pool - at, 0), min((r + 1) * pool - at, n)
        if hi > lo:
            peak[r] = np.fmax(peak[r], np.fmax.reduce(a[lo:hi], axis=0))
            floor[r] = np.fmin(floor[r], np.fmin.reduce(a[lo:hi], axis=0))
    # an all-NaN group reduces to NaN; the fold leaves the identity there
    return np.where(np.isnan(peak), F32(0), peak).astype(F32), np.where(np.isnan(floor), INF, floor).astype(F32)


def rows_with_edges(W, n=N, seed=5):
    """n rows of W norms-like values (non-negative) with NaN, +inf, 0.0 and subnormals planted, a whole row and a whole column of NaN"""
    rng = np.random.default_rng(seed + W)
    a = rng.random((n, W), dtype=F32) * F32(8)
    special = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF], dtype=np.uint32).view(F32)
    idx = rng.integers(0, n * W, size=max(n * W // 5, 8))
    a.reshape(-1)[idx] = special[rng.integers(0, special.size, size=idx.size)]
    a[11] = np.nan                                   # pool == 1: a group that is NaN throughout
    if W >= 4:
        a[:, W // 2] = np.nan                        # ... and a bin that is NaN in every group
    a[0, 0], a[1, 0], a[2, 0], a[3, 0] = np.nan, F32(0), np.uint32(1).view(F32), INF
    return a


def same(got, ref):
    return got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[0].shape == ref[0].shape


def test_init(engine):
    peak, floor = engine.pool_init(5, 3)
    assert peak.shape == floor.shape == (3, 5) and peak.dtype == floor.dtype == F32
    assert not peak.view(np.uint32).any() and (floor.view(np.uint32) == 0x7F800000).all()
    from quadrs_amd import _ffi
    only = np.full(4, F32(-7.5))
    assert _ffi.lib().qd_pool_init(None, only.ctypes.data_as(C.c_void_p), 2, 2) == 0 and (only == INF).all()
    assert _ffi.lib().qd_pool_init(None, None, 2, 2) == 0


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("pool", POOLS)
def test_fold_matches_numpy(engine, W, pool):
    a = rows_with_edges(W)
    assert np.isnan(a).any() and np.isinf(a).any() and (a == 0).any() and ((a > 0) & (a < F32(1.2e-38))).any()
    got = engine.pool_fold(a, pool)
    assert got[0].shape == (-(-N // pool), W)
    assert same(got, np_pool(a, pool))
    if pool == 1:
        keep = ~np.isnan(a)
        assert got[0][keep].tobytes() == a[keep].tobytes() and got[1][keep].tobytes() == a[keep].tobytes()
        assert not got[0][11].any() and (got[1][11] == INF).all()


@pytest.mark.parametrize("W", [1, 4, 64])
@pytest.mark.parametrize("pool", POOLS)
def test_two_parts_at_every_split_point(engine, W, pool):
    a = rows_with_edges(W)
    whole = engine.pool_fold(a, pool)
    for at in range(N + 1):
        into = engine.pool_init(W, -(-N // pool))
        engine.pool_fold(a[at:], pool, at=at, into=into)             # the later part first: the order is free
        engine.pool_fold(a[:at], pool, at=0, into=into)
        assert same(into, whole), at


@pytest.mark.parametrize("W", WIDTHS)
def test_one_row_is_the_summary(engine, W):
    a = rows_with_edges(W)
    s = engine.summary_fold(a)
    for pool in (N, N + 1, 50, 1 << 40):
        peak, floor = engine.pool_fold(a, pool)
        assert peak.shape == (1, W) and peak[0].tobytes() == s.peak.tobytes() and floor[0].tobytes() == s.floor.tobytes()


def test_one_array_only(engine):
    a = rows_with_edges(4)
    ref = engine.pool_fold(a, 3)
    peak, floor = engine.pool_init(4, 13)
    assert engine.pool_fold(a, 3, into=(peak, None))[0].tobytes() == ref[0].tobytes()
    assert engine.pool_fold(a, 3, into=(None, floor))[1].tobytes() == ref[1].tobytes()


def test_error_codes(engine):
    from quadrs_amd import _ffi
    a = rows_with_edges(4)
    with pytest.raises(engine.QuadrsError) as e:
        engine.pool_fold(a, 0, into=engine.pool_init(4, 1))
    assert e.value.code == _ffi.ERR_INVALID
    with pytest.raises(engine.QuadrsError) as e:
        engine.pool_fold(a, 3, into=(None, None))
    assert e.value.code == _ffi.ERR_INVALID
    L = _ffi.lib()
    peak, _ = engine.pool_init(4, 1)
    pp = peak.ctypes.data_as(C.c_void_p)
    assert L.qd_pool_fold(pp, None, 4, 1, 0, None, 1) == _ffi.ERR_INVALID          # no norms
    assert L.qd_pool_fold(pp, None, 0, 1, 0, None, 0) == _ffi.ERR_INVALID          # no width
    assert L.qd_pool_fold(pp, None, 4, 1, 0, None, 0) == 0                         # nothing to fold


def test_plan_level_refusals_precede_any_gpu_call(engine):
    """qd_plan_pool without a plan is refused before anything else is looked at, as every plan call is."""
    from quadrs_amd import _ffi
    peak, floor = engine.pool_init(4, 1)
    rc = _ffi.lib().qd_plan_pool(None, None, _ffi.MEM_HOST, 0, 0, 0, 1, 1, peak.ctypes.data_as(C.c_void_p), floor.ctypes.data_as(C.c_void_p),
                                 _ffi.MEM_HOST, None)
    assert rc == _ffi.ERR_INVALID
    assert not peak.any() and (floor == INF).all()
