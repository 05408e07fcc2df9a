"""The level counts' host half (include/quadrs_hip.h, "percentile traces and persistence counts"): qd_density_init / _fold / _merge /
_quantile against referees written here — np.add.at over the clipped bucket numbers for the counts, Python integers and math.ceil for the
quantile — on random norms and on planted values (every bucket edge and the value just below it, zeros of both signs, subnormals, the
largest finite value, +inf, NaNs of both signs), parts == whole in every order, and the error codes.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

F32 = np.float32
NAN_BITS, INF_BITS, MAX_BITS = 0x7FC00000, 0x7F800000, 0x7F7FFFFF
BUCKETS = 2041
LEVELS = [1, 2, 64, 256]


def level0s(L):
    return [0, 1000, BUCKETS - L]


def ref_counts(norms, pool, level0, L, at=0, rows=None):
    """uint32[R, W, L]: np.add.at on clip((bits & 0x7fffffff) >> 20, level0, level0 + L - 1) - level0, NaNs dropped"""
    a = np.ascontiguousarray(norms, dtype=F32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    n, W = a.shape
    R = -(-(at + n) // pool) if rows is None else rows
    out = np.zeros((R, W, L), np.uint32)
    level = np.clip((a >> 20).astype(np.int64), level0, level0 + L - 1) - level0
    r = np.broadcast_to(((at + np.arange(n)) // pool)[:, None], a.shape)
    b = np.broadcast_to(np.arange(W)[None, :], a.shape)
    keep = a <= INF_BITS
    np.add.at(out, (r[keep], b[keep], level[keep]), 1)
    return out


def ref_quantile(counts, level0, q):
    """(lo, hi, n) by the header's rule, in Python integers; math.ceil(q * N) on floats as specified"""
    R, W, L = counts.shape
    lo, hi, n = np.empty((R, W), np.uint32), np.empty((R, W), np.uint32), np.empty((R, W), np.uint32)
    for r in range(R):
        for b in range(W):
            cell = [int(x) for x in counts[r, b]]
            N = sum(cell)
            n[r, b] = N
            if N == 0:
                lo[r, b] = hi[r, b] = NAN_BITS
                continue
            want = max(1, math.ceil(q * float(N)))
            cum, j = 0, 0
            for j, c in enumerate(cell):
                cum += c
                if cum >= want:
                    break
            lo[r, b] = 0 if j == 0 else (level0 + j) << 20
            hi[r, b] = INF_BITS if j == L - 1 else (level0 + j + 1) << 20
    return lo.view(F32), hi.view(F32), n


def same(got, ref):
    return len(got) == len(ref) and all(g.shape == r.shape and g.dtype == r.dtype and g.tobytes() == r.tobytes() for g, r in zip(got, ref))


def planted(W):
    """rows of W bins that hold every bucket edge k << 20 and the value just below it, 0.0 and -0.0, subnormals, 0x7f7fffff, +inf, NaNs of
    both signs and negative values, then random norms around 1.0; float32[n, W]"""
    edges = (np.arange(1, 2041, dtype=np.uint32) << 20)
    bits = np.concatenate([
        edges, edges - 1, edges | np.uint32(0x80000000),
        np.array([0, 0x80000000, 1, 2, 0x7FFFFF, 0x807FFFFF, 0x800000, MAX_BITS, 0xFF7FFFFF, INF_BITS, 0xFF800000, NAN_BITS, 0xFFC00000, 0x7F800001,
                  0xFFFFFFFF, 0x7FFFFFFF], dtype=np.uint32)])
    rng = np.random.default_rng(W)
    noise = np.abs(rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(F32).view(np.uint32)
    bits = np.concatenate([bits, noise])
    bits = np.concatenate([bits, np.zeros(-len(bits) % W, np.uint32)])
    rng.shuffle(bits)
    return bits.view(F32).reshape(-1, W)


@pytest.fixture(scope="module")
def rows():
    cache = {}

    def get(W):
        if W not in cache:
            cache[W] = planted(W)
            cache[W].setflags(write=False)
        return cache[W]
    return get


def test_init(engine):
    c = engine.density_init(5, 4, 3)
    assert c.shape == (3, 5, 4) and c.dtype == np.uint32 and not c.any()
    c[:] = 7
    from quadrs_amd import _ffi
    assert _ffi.lib().qd_density_init(c.ctypes.data_as(C.c_void_p), 5, 4, 2) == 0 and not c[:2].any() and (c[2] == 7).all()
    assert (_ffi.DENSITY_MAX_LEVELS, _ffi.DENSITY_BUCKETS, _ffi.DENSITY_MAX_Q) == (256, BUCKETS, 8)


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("W", [1, 4, 64])
def test_fold_matches_the_referee(engine, rows, W, L):
    a = rows(W)
    u = a.view(np.uint32)
    assert np.isnan(a).any() and np.isinf(a).any() and (u == 0).any() and (u == 0x80000000).any() and (u == 1).any() and (u == MAX_BITS).any()
    for level0 in level0s(L):
        for pool in (1, 3, a.shape[0], a.shape[0] + 5):
            got = engine.density_fold(a, pool, level0, L)
            ref = ref_counts(a, pool, level0, L)
            assert got.shape == ref.shape and got.dtype == np.uint32 and got.tobytes() == ref.tobytes(), (level0, pool)
    # every value is somewhere unless it is a NaN
    got = engine.density_fold(a, a.shape[0], 0, L)
    assert (got.sum(axis=2)[0] == (~np.isnan(a)).sum(axis=0)).all()


def test_the_grid_is_the_summarys_scale(engine, rows):
    a = rows(4)
    full = engine.density_fold(a, a.shape[0], 1000, 256)
    s = engine.summary_fold(a)
    hist = np.array(s.c.hist[:], dtype=np.uint64)
    mine = full.sum(axis=(0, 1), dtype=np.uint64)
    assert (mine[1:255] == hist[1001:1255]).all()
    assert mine[0] == hist[:1001].sum() and mine[255] == hist[1255:].sum()


@pytest.mark.parametrize("L", [2, 64])
def test_parts_are_the_whole_in_every_order(engine, rows, L):
    a = rows(4)[:96]
    n = a.shape[0]
    level0 = 1000
    for pool in (1, 5, n):
        whole = engine.density_fold(a, pool, level0, L)
        R = whole.shape[0]
        for at in range(n + 1):                                  # two parts, cut at every window
            c = engine.density_init(4, L, R)
            engine.density_fold(a[at:], pool, level0, L, at=at, into=c)
            engine.density_fold(a[:at], pool, level0, L, at=0, into=c)
            assert c.tobytes() == whole.tobytes(), (pool, at)
        rng = np.random.default_rng(pool)
        cuts = sorted(set(rng.integers(0, n, 9).tolist()) | {0, n})
        parts = list(zip(cuts[:-1], cuts[1:]))
        rng.shuffle(parts)
        c = engine.density_init(4, L, R)
        merged = engine.density_init(4, L, R)
        for lo, hi in parts:
            engine.density_fold(a[lo:hi], pool, level0, L, at=lo, into=c)
            one = engine.density_init(4, L, R)
            engine.density_merge(merged, engine.density_fold(a[lo:hi], pool, level0, L, at=lo, into=one))
        assert c.tobytes() == whole.tobytes() and merged.tobytes() == whole.tobytes(), pool


@pytest.mark.parametrize("L", LEVELS)
def test_quantile_matches_the_referee(engine, rows, L):
    a = rows(4)
    for level0 in level0s(L):
        counts = engine.density_fold(a, 100, level0, L)
        counts = np.concatenate([counts, np.zeros((1, 4, L), np.uint32)])       # a row of empty cells
        counts[1, 0, :] = 0; counts[1, 0, 0] = 9                               # all weight in level 0
        counts[1, 1, :] = 0; counts[1, 1, L - 1] = 9                           # ... in level L - 1
        counts[1, 2, :] = 0; counts[1, 2, 0] = 5; counts[1, 2, L - 1] += 5    # q N an exact integer at q = 0.5: r = 5 is still level 0
        for q in (0.0, 5e-324, 1e-9, 0.5, 1.0):
            got = engine.density_quantile(counts, level0, q)
            assert same(got, ref_quantile(counts, level0, q)), (level0, q)
            assert (got[0].view(np.uint32)[-1] == NAN_BITS).all() and (got[1].view(np.uint32)[-1] == NAN_BITS).all() and not got[2][-1].any()
        lo, hi, n = engine.density_quantile(counts, level0, 0.5)
        assert lo[1, 0] == 0.0 and n[1, 0] == 9 and np.isinf(hi[1, 1])
        if L > 1:
            assert lo[1, 2] == 0.0 and hi[1, 2].view(np.uint32) == (level0 + 1) << 20
            assert engine.density_quantile(counts, level0, 0.6)[0][1, 2].view(np.uint32) == (level0 + L - 1) << 20
            assert lo[1, 1].view(np.uint32) == (level0 + L - 1) << 20


def test_quantile_brackets_the_order_statistic(engine, rows):
    a = rows(1)
    vals = np.sort(np.abs(a[~np.isnan(a)]))
    counts = engine.density_fold(a, a.shape[0], 990, 64)
    for q in (0.0, 0.1, 0.5, 0.9, 1.0):
        lo, hi, n = engine.density_quantile(counts, 990, q)
        v = vals[max(1, math.ceil(q * len(vals))) - 1]
        assert n[0, 0] == len(vals) and lo[0, 0] <= v and (v < hi[0, 0] or np.isinf(hi[0, 0])), q


def test_error_codes(engine, rows):
    from quadrs_amd import _ffi
    L = _ffi.lib()
    a = np.ascontiguousarray(rows(4)[:8])
    ap = a.ctypes.data_as(C.c_void_p)
    c = engine.density_fold(a, 3, 1000, 8)
    keep = c.copy()
    cp = c.ctypes.data_as(C.c_void_p)
    fold = L.qd_density_fold
    assert fold(None, 4, 1000, 8, 3, 0, ap, 8) == _ffi.ERR_INVALID
    assert fold(cp, 4, 1000, 8, 3, 0, None, 8) == _ffi.ERR_INVALID
    assert fold(cp, 0, 1000, 8, 3, 0, ap, 8) == _ffi.ERR_INVALID
    assert fold(cp, 4, 1000, 8, 0, 0, ap, 8) == _ffi.ERR_INVALID
    assert fold(cp, 4, 1000, 0, 3, 0, ap, 8) == _ffi.ERR_INVALID
    assert fold(cp, 4, 1000, 257, 3, 0, ap, 8) == _ffi.ERR_INVALID
    assert fold(cp, 4, BUCKETS - 7, 8, 3, 0, ap, 8) == _ffi.ERR_INVALID
    assert fold(cp, 4, 0xFFFFFFFF, 2, 3, 0, ap, 8) == _ffi.ERR_INVALID
    assert fold(cp, 4, 1000, 8, 3, 0, None, 0) == 0                          # no windows
    assert c.tobytes() == keep.tobytes()
    # a row that would pass 2^31 windows: refused before anything is added, also to the rows before it
    big = engine.density_init(4, 8, 3)
    big[1, 2, 3] = (1 << 31) - 2
    keep = big.copy()
    assert fold(big.ctypes.data_as(C.c_void_p), 4, 1000, 8, 3, 0, ap, 8) == _ffi.ERR_INVALID and big.tobytes() == keep.tobytes()
    assert fold(big.ctypes.data_as(C.c_void_p), 4, 1000, 8, 3, 0, ap, 3) == 0 and big[0].sum() == (~np.isnan(a[:3])).sum()
    # merge
    merge = L.qd_density_merge
    one = engine.density_init(4, 8, 3)
    one[1, 2, 0] = 3
    keep = big.copy()
    bp, op = big.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)
    assert merge(bp, op, 4, 8, 3) == _ffi.ERR_INVALID and big.tobytes() == keep.tobytes()
    one[1, 2, 0] = 2
    assert merge(bp, op, 4, 8, 3) == 0 and big[1, 2].sum() == 1 << 31
    assert merge(None, op, 4, 8, 3) == _ffi.ERR_INVALID and merge(bp, None, 4, 8, 3) == _ffi.ERR_INVALID
    assert merge(bp, op, 0, 8, 3) == _ffi.ERR_INVALID and merge(bp, op, 4, 0, 3) == _ffi.ERR_INVALID
    with pytest.raises(ValueError):
        engine.density_merge(big, engine.density_init(4, 8, 2))
    # quantile
    quant = L.qd_density_quantile
    lo = np.full((3, 4), F32(-7.5))
    lp = lo.ctypes.data_as(C.c_void_p)
    assert quant(cp, 4, 1000, 8, 3, 0.5, None, None, None) == _ffi.ERR_INVALID
    assert quant(None, 4, 1000, 8, 3, 0.5, lp, None, None) == _ffi.ERR_INVALID
    for q in (-1e-9, 1.0000001, float("nan"), float("inf")):
        assert quant(cp, 4, 1000, 8, 3, q, lp, None, None) == _ffi.ERR_INVALID
    assert quant(cp, 4, BUCKETS - 7, 8, 3, 0.5, lp, None, None) == _ffi.ERR_INVALID
    assert quant(cp, 4, 1000, 0, 3, 0.5, lp, None, None) == _ffi.ERR_INVALID
    assert quant(cp, 0, 1000, 8, 3, 0.5, lp, None, None) == _ffi.ERR_INVALID
    assert (lo == F32(-7.5)).all()
    assert quant(cp, 4, 1000, 8, 3, 0.5, lp, None, None) == 0 and quant(cp, 4, 1000, 8, 3, 0.5, None, lp, None) == 0
    n = np.zeros((3, 4), np.uint32)
    assert quant(cp, 4, 1000, 8, 3, 0.5, None, None, n.ctypes.data_as(C.c_void_p)) == 0 and (n == c.sum(axis=2)).all()
