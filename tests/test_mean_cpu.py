"""The average-trace rows' host half (include/quadrs_hip.h, "average-trace rows"): qd_mean_init / _fold / _merge / _finish against a referee
written here with Python integers — the exact sum per cell in units of 2^-149, math.fsum for the f64 sum, and an f32 rounding that is
proven nearest / ties-to-even by exact comparison with both neighbours (no float division anywhere) — the planted rounding cases, parts ==
whole in every order, and the error codes.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from test_pool_cpu import F32, N, POOLS, WIDTHS, rows_with_edges

NAN_BITS, INF_BITS, MAX_BITS = 0x7FC00000, 0x7F800000, 0x7F7FFFFF
WORDS = 10


def units(bits):
    """a finite non-negative f32's value as an integer count of 2^-149"""
    e, m = bits >> 23, bits & 0x7FFFFF
    return (m | (1 << 23) if e else m) << (max(e, 1) - 1)


def round_f32(num, den):
    """the bit pattern of num / den (integers, in units of 2^-149, the result known to be finite) rounded to f32, nearest, ties to even:
    a guess from the bit length, walked until lo <= num / den < up for f32 neighbours lo and up = np.nextafter(lo, inf), then the nearer
    of the two by exact integer comparison, the even pattern on a tie"""
    q = num // den
    L = q.bit_length()
    b = q if L <= 24 else ((L - 24) << 23) + (q >> (L - 24))
    b = min(b, MAX_BITS)
    while units(b) * den > num:
        b -= 1
    while b < MAX_BITS and units(b + 1) * den <= num:
        b += 1
    if b == MAX_BITS:
        return b
    lo = np.uint32(b).view(F32)
    up = int(np.nextafter(lo, F32(np.inf)).view(np.uint32))
    assert up == b + 1 and units(b) * den <= num < units(up) * den
    below, above = num - units(b) * den, units(up) * den - num              # distances times den
    if below != above:
        return b if below < above else up
    return b if b % 2 == 0 else up


def ref_cell(bits):
    """(mean bits, f64 sum, count) of one cell's values, given as u32 bit patterns (any sign, NaNs included)"""
    vals = [int(b) & 0x7FFFFFFF for b in bits]
    vals = [b for b in vals if b <= INF_BITS]
    if not vals:
        return NAN_BITS, 0.0, 0
    if INF_BITS in vals:
        return INF_BITS, math.inf, len(vals)
    total = math.fsum(float(np.uint32(b).view(F32)) for b in vals)          # exact, rounded once
    return round_f32(sum(units(b) for b in vals), len(vals)), total, len(vals)


def ref_mean(norms, pool, at=0):
    """(mean_rows, sum_rows, count_rows) of rows (at + i) // pool of the norms rows (n, W), by ref_cell"""
    a = np.ascontiguousarray(norms, dtype=F32).view(np.uint32)
    n, W = a.shape
    R = -(-(at + n) // pool)
    mean, total, count = np.empty((R, W), np.uint32), np.empty((R, W), np.float64), np.empty((R, W), np.uint32)
    for r in range(R):
        lo, hi = max(r * pool - at, 0), min((r + 1) * pool - at, n)
        for c in range(W):
            mean[r, c], total[r, c], count[r, c] = ref_cell(a[lo:hi, c])
    return mean.view(F32), total, count


def same3(got, ref):
    return all(g.shape == r.shape and g.dtype == r.dtype and g.tobytes() == r.tobytes() for g, r in zip(got, ref)) and len(got) == len(ref) == 3


def naive_mean(norms, pool):
    """what a sequential f32 accumulation would give: the sum in window order, divided by the count in f32"""
    a = np.ascontiguousarray(norms, dtype=F32)
    n, W = a.shape
    R = -(-n // pool)
    out = np.zeros((R, W), F32)
    for r in range(R):
        acc, cnt = np.zeros(W, F32), np.zeros(W, F32)
        with np.errstate(all="ignore"):
            for row in np.abs(a[r * pool:(r + 1) * pool]):
                keep = ~np.isnan(row)
                acc = np.where(keep, acc + row, acc).astype(F32)
                cnt += keep
            out[r] = acc / cnt
    return out


@pytest.fixture(scope="module")
def referee():
    cache = {}

    def get(W, pool):
        if (W, pool) not in cache:
            cache[W, pool] = ref_mean(rows_with_edges(W), pool)
        return cache[W, pool]
    return get


def test_init(engine):
    acc = engine.mean_init(5, 3)
    assert acc.shape == (3, 5, WORDS) and acc.dtype == np.uint64 and not acc.any()
    acc[:] = 7
    from quadrs_amd import _ffi
    assert _ffi.MEAN_WORDS == WORDS
    assert _ffi.lib().qd_mean_init(acc.ctypes.data_as(C.c_void_p), 5, 2) == 0 and not acc[:2].any() and (acc[2] == 7).all()
    mean, total, count = engine.mean_finish(engine.mean_init(2, 2))
    assert (mean.view(np.uint32) == NAN_BITS).all() and not total.any() and not np.signbit(total).any() and not count.any()


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("pool", POOLS)
def test_fold_and_finish_match_the_referee(engine, referee, W, pool):
    a = rows_with_edges(W)
    assert np.isnan(a).any() and np.isinf(a).any() and (a == 0).any() and ((a > 0) & (a < F32(1.2e-38))).any()
    assert W < 64 or (a.view(np.uint32) == MAX_BITS).any()
    got = engine.mean_finish(engine.mean_fold(a, pool))
    assert got[0].shape == (-(-N // pool), W)
    assert same3(got, referee(W, pool))
    if pool >= 7 and W >= 64:
        # teeth: a sequential f32 sum divided by the count is not the mean in some finite cells of this very input
        naive = naive_mean(a, pool)
        finite = np.isfinite(got[0]) & np.isfinite(naive)
        assert (naive.view(np.uint32)[finite] != got[0].view(np.uint32)[finite]).any()
    if pool == 1:
        keep = ~np.isnan(a)
        assert got[0][keep].tobytes() == np.abs(a)[keep].tobytes()
        assert got[1][keep].tobytes() == np.abs(a)[keep].astype(np.float64).tobytes()
        assert (got[2] == keep).all() and (got[0].view(np.uint32)[~keep] == NAN_BITS).all() and not got[1][~keep].any()


def f32_bits(x):
    return int(np.asarray(x, dtype=F32).view(np.uint32))


def _planted_cases():
    one, eps = 0x3F800000, 1                                    # 1.0 and one unit in its last place (2^-23)
    p100, p47 = f32_bits(2.0 ** 100), f32_bits(2.0 ** 47)
    nan, ninf = NAN_BITS, INF_BITS
    # column -> (values, expected mean bits or None, expected f64 sum or None, expected count)
    return [
        ([one, one + eps], one, None, 2),                                           # mean tie -> 1.0 (even)
        ([one + eps, one + 2 * eps], one + 2 * eps, None, 2),                       # mean tie -> 1 + 2^-22 (even)
        ([1, 0], 0, 2.0 ** -149, 2),                                                # 2^-150 -> 0
        ([3, 0], 2, 3 * 2.0 ** -149, 2),                                            # 1.5 quanta -> 2 quanta
        ([p100, p47], None, 2.0 ** 100, 2),                                         # sum tie -> 2^100 (even)
        ([p100, p47, 1], None, 2.0 ** 100 + 2.0 ** 48, 3),                          # the sticky bit reaches across all limbs
        ([MAX_BITS] * 3, MAX_BITS, 3 * float(np.uint32(MAX_BITS).view(F32)), 3),    # the sum is not an f32, the mean is
        ([MAX_BITS, 1], 0x7EFFFFFF, float(np.uint32(MAX_BITS).view(F32)), 2),       # the highest and the lowest limb
        ([nan, nan | 0x80000000, nan], nan, 0.0, 0),                                # no values: no mean
        ([one, ninf, nan], ninf, math.inf, 2),                                      # +inf anywhere
        ([0x80000000], 0, 0.0, 1),                                                  # -0.0 counts as 0.0
        ([0x80000000 | one, one], one, 2.0, 2),                                     # the sign bit is dropped
    ]


PLANTED_CASES = _planted_cases()                # shared with the GPU's planted streams (tests/util.py, planted_cells)


def test_planted_rounding_cases(engine):
    cases, nan = PLANTED_CASES, NAN_BITS
    rows = np.full((3, len(cases)), nan, dtype=np.uint32)
    for c, (vals, *_) in enumerate(cases):
        rows[:len(vals), c] = vals
    mean, total, count = engine.mean_finish(engine.mean_fold(rows.view(F32), 3))
    for c, (vals, want_mean, want_sum, want_count) in enumerate(cases):
        ref = ref_cell(vals)
        got = (int(mean.view(np.uint32)[0, c]), float(total[0, c]), int(count[0, c]))
        assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2] == want_count, (c, got, ref)
        assert want_mean is None or got[0] == want_mean, (c, hex(got[0]))
        assert want_sum is None or got[1] == want_sum, (c, got[1])
        assert not math.copysign(1.0, got[1]) < 0


@pytest.mark.parametrize("W", [1, 4, 64])
@pytest.mark.parametrize("pool", POOLS)
def test_parts_equal_the_whole(engine, W, pool):
    a = rows_with_edges(W)
    R = -(-N // pool)
    whole = engine.mean_fold(a, pool)
    out = engine.mean_finish(whole)
    for at in range(N + 1):
        into = engine.mean_init(W, R)
        engine.mean_fold(a[at:], pool, at=at, into=into)             # the later part first: the order is free
        engine.mean_fold(a[:at], pool, at=0, into=into)
        assert into.tobytes() == whole.tobytes(), at
        # two accumulators, merged
        x = engine.mean_fold(a[:at], pool, into=engine.mean_init(W, R))
        y = engine.mean_fold(a[at:], pool, at=at, into=engine.mean_init(W, R))
        assert engine.mean_merge(x, y).tobytes() == whole.tobytes(), at
        assert same3(engine.mean_finish(x), out)
    # the windows of each group in a shuffled order, one call per window
    rng = np.random.default_rng(pool * 100 + W)
    into = engine.mean_init(W, R)
    for i in rng.permutation(N):
        engine.mean_fold(a[i:i + 1], pool, at=int(i), into=into)
    assert into.tobytes() == whole.tobytes() and same3(engine.mean_finish(into), out)
    b = a.copy()
    for r in range(R):
        b[r * pool:(r + 1) * pool] = a[r * pool:(r + 1) * pool][rng.permutation(min((r + 1) * pool, N) - r * pool)]
    assert engine.mean_fold(b, pool).tobytes() == whole.tobytes()


@pytest.mark.parametrize("W", WIDTHS)
def test_one_row(engine, referee, W):
    a = rows_with_edges(W)
    ref = referee(W, N)
    for pool in (N, N + 1, 50, 1 << 31, 1 << 40):
        got = engine.mean_finish(engine.mean_fold(a, pool))
        assert got[0].shape == (1, W) and same3(got, ref)


def test_one_output_only(engine):
    from quadrs_amd import _ffi
    a = rows_with_edges(4)
    acc = engine.mean_fold(a, 3)
    ref = engine.mean_finish(acc)
    for which in range(3):
        out = np.zeros_like(ref[which])
        ptrs = [None, None, None]
        ptrs[which] = out.ctypes.data_as(C.c_void_p)
        assert _ffi.lib().qd_mean_finish(acc.ctypes.data_as(C.c_void_p), 4, acc.shape[0], *ptrs) == 0
        assert out.tobytes() == ref[which].tobytes()


def test_error_codes(engine):
    from quadrs_amd import _ffi
    L, INVALID = _ffi.lib(), _ffi.ERR_INVALID
    a = rows_with_edges(4)
    with pytest.raises(engine.QuadrsError) as e:
        engine.mean_fold(a, 0, into=engine.mean_init(4, 1))
    assert e.value.code == INVALID
    acc = engine.mean_init(4, 1)
    ap, norms = acc.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)
    out = np.zeros(4, F32)
    op = out.ctypes.data_as(C.c_void_p)
    assert L.qd_mean_init(None, 4, 1) == INVALID and L.qd_mean_init(ap, 0, 1) == INVALID
    assert L.qd_mean_fold(ap, 4, 0, 0, norms, 1) == INVALID                         # pool 0
    assert L.qd_mean_fold(ap, 0, 1, 0, norms, 0) == INVALID                         # no width
    assert L.qd_mean_fold(None, 4, 1, 0, norms, 1) == INVALID                       # no accumulator
    assert L.qd_mean_fold(ap, 4, 1, 0, None, 1) == INVALID                          # no norms
    assert L.qd_mean_fold(ap, 4, 1, 0, None, 0) == 0                                # nothing to fold
    assert L.qd_mean_merge(None, ap, 4, 1) == INVALID and L.qd_mean_merge(ap, None, 4, 1) == INVALID and L.qd_mean_merge(ap, ap, 0, 1) == INVALID
    assert L.qd_mean_finish(None, 4, 1, op, None, None) == INVALID and L.qd_mean_finish(ap, 0, 1, op, None, None) == INVALID
    assert L.qd_mean_finish(ap, 4, 1, None, None, None) == INVALID                  # all outputs NULL
    assert not acc.any() and not out.any()
    # a count driven to 2^31 by hand: one more window is refused and nothing changes, whichever half of word 9 holds the count
    a = np.ones((8, 4), F32)
    norms = a.ctypes.data_as(C.c_void_p)
    for full in (1 << 31, (1 << 31) << 32, ((1 << 30) << 32) + (1 << 30)):
        acc = engine.mean_fold(a[:2], 5, into=engine.mean_init(4, 2))
        acc[0, 1, 9] = full
        before = acc.copy()
        assert L.qd_mean_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 2, norms, 1) == INVALID
        assert acc.tobytes() == before.tobytes()
        assert L.qd_mean_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 5, norms, 3) == 0          # the other row still takes windows
        before = acc.copy()
        other = engine.mean_fold(a[:1], 5, into=engine.mean_init(4, 2))
        assert L.qd_mean_merge(acc.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p), 4, 2) == INVALID
        assert L.qd_mean_merge(other.ctypes.data_as(C.c_void_p), acc.ctypes.data_as(C.c_void_p), 4, 2) == INVALID
        assert acc.tobytes() == before.tobytes()
    acc[0, 1, 9] = (1 << 31) - 1                                                    # room for exactly one
    assert L.qd_mean_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 2, norms, 1) == 0
    with pytest.raises(ValueError):
        engine.mean_merge(engine.mean_init(4, 2), engine.mean_init(4, 1))


def test_plan_level_refusals_precede_any_gpu_call(engine):
    """qd_plan_mean without a plan is refused before anything else is looked at, as every plan call is."""
    from quadrs_amd import _ffi
    out = np.full(4, F32(-7.5))
    rc = _ffi.lib().qd_plan_mean(None, None, _ffi.MEM_HOST, 0, 0, 0, 1, 1, out.ctypes.data_as(C.c_void_p), None, None, _ffi.MEM_HOST, None)
    assert rc == _ffi.ERR_INVALID and (out == F32(-7.5)).all()
