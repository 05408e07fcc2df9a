"""The deviation-trace rows' host half (include/quadrs_hip.h, "deviation-trace rows"): qd_spread_init / _fold / _merge / _finish against a
referee written here with Python integers only — A the sum in units of 2^-149, B the sum of squares in units of 2^-298, D = n B - A^2, the
f64 sum of squared deviations by one correctly rounded int / int division, and the f32 root by a binary search over f32 patterns followed
by an exact midpoint comparison (no float division and no float sqrt anywhere in the referee) — the planted rounding and cancellation
cases, the cell's two halves against qd_mean_* and qd_power_*, parts == whole in every order, each output alone, the error codes, and the
resources of the two kernels in the build.  No GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from test_pool_cpu import F32, N, POOLS, WIDTHS, rows_with_edges
from test_power_cpu import units

NAN_BITS, INF_BITS, MAX_BITS = 0x7FC00000, 0x7F800000, 0x7F7FFFFF
NAN64_BITS = 0x7FF8000000000000
WORDS = 28
NAMES = ("std", "ssd", "count", "mean", "rms")


def f64_bits(x):
    return int(np.float64(x).view(np.uint64))


def exact_d(vals):
    """(n, D) of a cell's finite magnitudes: D = n B - A^2 in units of 2^-298"""
    u = [units(b) for b in vals]
    n, A, B = len(u), sum(u), sum(x * x for x in u)
    D = n * B - A * A
    assert D >= 0
    return n, D


def root_over_n_f32(D, n):
    """the bit pattern of sqrt(D) / n (D in units of 2^-298) rounded to f32, nearest, ties to even: the largest pattern lo with
    val(lo)^2 n^2 <= D by binary search, then 4 D against n^2 (lo + up)^2, the even pattern on a tie.  The search runs over every
    finite pattern unless the integer root hands it a bracket of three that it has checked at both ends (the GPU tests referee whole worlds)"""
    lo, hi, n2 = 0, MAX_BITS, n * n
    X = math.isqrt(D) // n
    L = X.bit_length()
    g = X if L <= 24 else ((L - 24) << 23) + (X >> (L - 24))
    if 1 <= g < MAX_BITS - 1 and units(g - 1) ** 2 * n2 <= D < units(g + 2) ** 2 * n2:
        lo, hi = g - 1, g + 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if units(mid) ** 2 * n2 <= D:
            lo = mid
        else:
            hi = mid - 1
    assert lo < MAX_BITS
    a, b = units(lo), units(lo + 1)
    assert a * a * n2 <= D < b * b * n2
    mid = n2 * (a + b) ** 2
    if 4 * D != mid:
        return lo if 4 * D < mid else lo + 1
    return lo if lo % 2 == 0 else lo + 1


def ref_cell(bits):
    """(std bits, ssd f64 bits, count) of one cell's values, given as u32 bit patterns (any sign, NaNs included)"""
    vals = [int(b) & 0x7FFFFFFF for b in bits]
    vals = [b for b in vals if b <= INF_BITS]
    if not vals:
        return NAN_BITS, 0, 0
    if INF_BITS in vals:
        return NAN_BITS, NAN64_BITS, len(vals)
    n, D = exact_d(vals)
    if D == 0:
        return 0, 0, n
    ssd = math.ldexp(D / n, -298)                 # CPython's int / int is correctly rounded; the ldexp is exact (a normal result)
    assert ssd >= 2.0 ** -329
    return root_over_n_f32(D, n), f64_bits(ssd), n


def ref_spread(norms, pool, at=0):
    """(std_rows f32, ssd_rows f64, count_rows u32) of rows (at + i) // pool of the norms rows (n, W), by ref_cell"""
    a = np.ascontiguousarray(norms, dtype=F32).view(np.uint32)
    n, W = a.shape
    R = -(-(at + n) // pool)
    std, ssd, count = np.empty((R, W), np.uint32), np.empty((R, W), np.uint64), np.empty((R, W), np.uint32)
    for r in range(R):
        lo, hi = max(r * pool - at, 0), min((r + 1) * pool - at, n)
        for c in range(W):
            std[r, c], ssd[r, c], count[r, c] = ref_cell(a[lo:hi, c])
    return std.view(F32), ssd.view(np.float64), count


def same(got, ref):
    """every array of `ref` against the one at its place in `got`, byte for byte (None in ref: not compared)"""
    return len(got) == len(ref) and all(r is None or (g is not None and g.shape == r.shape and g.dtype == r.dtype and g.tobytes() == r.tobytes())
                                        for g, r in zip(got, ref))


def twin5(engine, norms, pool, at=0):
    return engine.spread_finish(engine.spread_fold(norms, pool, at=at))


def halves(engine, norms, pool):
    """what the mean's and the power's own twins give for the same norms: (mean, rms, count)"""
    mean = engine.mean_finish(engine.mean_fold(norms, pool))
    power = engine.power_finish(engine.power_fold(norms, pool))
    assert mean[2].tobytes() == power[2].tobytes()
    return mean[0], power[0], mean[2]


@pytest.fixture(scope="module")
def referee():
    cache = {}

    def get(W, pool):
        if (W, pool) not in cache:
            cache[W, pool] = ref_spread(rows_with_edges(W), pool)
        return cache[W, pool]
    return get


def test_init(engine):
    acc = engine.spread_init(5, 3)
    assert acc.shape == (3, 5, WORDS) and acc.dtype == np.uint64 and not acc.any()
    acc[:] = 7
    from quadrs_amd import _ffi
    assert _ffi.SPREAD_WORDS == WORDS
    assert _ffi.lib().qd_spread_init(acc.ctypes.data_as(C.c_void_p), 5, 2) == 0 and not acc[:2].any() and (acc[2] == 7).all()
    std, ssd, count, mean, rms = engine.spread_finish(engine.spread_init(2, 2))
    for t in (std, mean, rms):
        assert (t.view(np.uint32) == NAN_BITS).all()
    assert not ssd.view(np.uint64).any() and not count.any()


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("pool", POOLS)
def test_the_cell_is_the_means_and_the_powers(engine, W, pool):
    """words 0-8, 9-26 and 27 are qd_mean_fold's words 0-8, qd_power_fold's words 0-17 and the count word; mean_rows and rms_rows are
    qd_mean_finish's and qd_power_finish's"""
    a = rows_with_edges(W)
    acc = engine.spread_fold(a, pool)
    m, p = engine.mean_fold(a, pool), engine.power_fold(a, pool)
    assert acc[..., 0:9].tobytes() == m[..., 0:9].tobytes()
    assert acc[..., 9:27].tobytes() == p[..., 0:18].tobytes()
    assert acc[..., 27].tobytes() == m[..., 9].tobytes() == p[..., 18].tobytes()
    got = engine.spread_finish(acc)
    mean, rms, count = halves(engine, a, pool)
    assert same(got, (None, None, count, mean, rms))


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("pool", POOLS)
def test_fold_and_finish_match_the_referee(engine, referee, W, pool):
    a = rows_with_edges(W)
    assert np.isnan(a).any() and np.isinf(a).any() and (a == 0).any() and ((a > 0) & (a < F32(1.2e-38))).any()
    got = twin5(engine, a, pool)
    assert got[0].shape == (-(-N // pool), W)
    assert same(got[:3], referee(W, pool))
    if pool == 1:
        keep, inf = ~np.isnan(a), np.isinf(a)
        assert (got[2] == keep).all()
        assert not got[0][keep & ~inf].view(np.uint32).any() and not got[1][keep & ~inf].view(np.uint64).any()       # std +0, ssd 0.0
        assert got[3][keep].tobytes() == np.abs(a)[keep].tobytes() and got[4][keep].tobytes() == np.abs(a)[keep].tobytes()
        assert (got[0].view(np.uint32)[~keep | inf] == NAN_BITS).all() and (got[1].view(np.uint64)[inf] == NAN64_BITS).all()
        assert not got[1].view(np.uint64)[~keep].any()


def fold_cells(engine, cases):
    """one cell per column: the values of cases[c], padded with NaN (which adds nothing), folded into one row"""
    depth = max([len(v) for v in cases] + [1])
    rows = np.full((depth, len(cases)), NAN_BITS, dtype=np.uint32)
    for c, vals in enumerate(cases):
        rows[:len(vals), c] = vals
    acc = engine.spread_fold(rows.view(F32), depth)
    std, ssd, count, mean, rms = engine.spread_finish(acc)
    m, r, cnt = halves(engine, rows.view(F32), depth)
    assert same((count, mean, rms), (cnt, m, r))
    return [(int(std.view(np.uint32)[0, c]), int(ssd.view(np.uint64)[0, c]), int(count[0, c])) for c in range(len(cases))], acc


def one_pass_variance(vals):
    """the running f64 formula: sum of v^2 / n - (sum of v / n)^2, in window order"""
    s = q = 0.0
    for b in vals:
        d = float(np.uint32(b).view(F32))
        s += d
        q += d * d
    return q / len(vals) - (s / len(vals)) ** 2


def _planted_cells():
    pair24 = [0x4B7FFFFE, 0x4B7FFFFF] * 2048
    pair_sqrt2 = [0x3FB504F3, 0x3FB504F4] * 1500
    pair_max = [0x7F7FFFFE, 0x7F7FFFFF] * 2048
    cases = [[0, 1], [0, 2], [0, 3], [0, 5], [0, 7], pair24, pair_sqrt2, pair_max, [MAX_BITS] * 3 + [0], [MAX_BITS, 0]]
    want = [0, 1, 2, 2, 4, 0x3F000000, 0x33800000, 0x73000000, 0x7EDDB3D6, 0x7EFFFFFF]
    equal = [[b] * k for b in (0, 1, 0x00800000, 0x3F800000, 0x4B7FFFFF, MAX_BITS) for k in (1, 2, 7)]
    others = [[0x3F800000], [0x80000000, 0], [0xBF800000, 0x3F800000, 0xC0000000], [NAN_BITS, 0x3F800000, 0xFFC00001, 0x40000000],
              [0x3F800000, INF_BITS, 0x40000000], [0xFF800000], [NAN_BITS, NAN_BITS | 0x80000000], []]
    return cases, want, equal, others


# shared with the GPU's planted streams (tests/util.py, planted_cells)
PLANTED_CASES, PLANTED_WANT, PLANTED_EQUAL, PLANTED_OTHERS = _planted_cells()
PAIR24_SSD = 1024.0                              # the 2^24 pair's sum of squared deviations


def test_planted_cells(engine):
    cases, want, equal, others = PLANTED_CASES, PLANTED_WANT, PLANTED_EQUAL, PLANTED_OTHERS
    pair24, pair_sqrt2 = cases[5], cases[6]
    got, _ = fold_cells(engine, cases + equal + others)
    for c, vals in enumerate(cases + equal + others):
        assert got[c] == ref_cell(vals), (c, [hex(x) for x in got[c]], [hex(x) for x in ref_cell(vals)])
    for c, w in enumerate(want):
        assert got[c][0] == w, (c, hex(got[c][0]))
    for c in range(len(cases), len(cases) + len(equal)):
        assert got[c][0] == 0 and got[c][1] == 0                     # all equal: std +0, ssd 0.0
    # the 2^24 pair: sigma is 0.5 exactly, the sum of squared deviations 1024, and the running f64 formula goes negative
    assert got[5][1] == f64_bits(PAIR24_SSD) == f64_bits(1024.0) and one_pass_variance(pair24) < 0
    # the sqrt(2) pair: the one-pass formula is off by a factor of seven
    v = one_pass_variance(pair_sqrt2)
    assert got[6][0] == 0x33800000 and int(F32(math.sqrt(v)).view(np.uint32)) == 0x34600000
    tail = got[len(cases) + len(equal):]
    assert tail[0] == (0, 0, 1) and tail[1] == (0, 0, 2)             # one value; -0.0 and 0.0
    assert tail[3][2] == 2 and tail[4] == (NAN_BITS, NAN64_BITS, 3) and tail[5] == (NAN_BITS, NAN64_BITS, 1)
    assert tail[6] == (NAN_BITS, 0, 0) and tail[7] == (NAN_BITS, 0, 0)


def random_cells(n_cells=300, seed=2025):
    """cells of 2, 3, 17 and 100 values whose exponents lie within three binades of a random one"""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n_cells):
        n = (2, 3, 17, 100)[i % 4]
        e0 = int(rng.integers(0, 255))
        e = np.clip(e0 + rng.integers(0, 4, n), 0, 254).astype(np.uint32)
        m = rng.integers(0, 1 << 23, n).astype(np.uint32)
        if i % 5 == 0:
            m &= np.uint32(0x7)                                     # short mantissas: exact roots and ties happen
        cases.append([int(x) for x in (e << 23) | m])
    return cases


def test_random_cells_match_the_referee(engine):
    """random_cells(): 300 cells, seed 2025"""
    cases = random_cells()
    assert len(cases) == 300
    got, _ = fold_cells(engine, cases)
    for c, vals in enumerate(cases):
        assert got[c] == ref_cell(vals), (c, [hex(v) for v in vals])
        ssd = float(np.uint64(got[c][1]).view(np.float64))
        assert ssd == 0.0 or 2.0 ** -329 <= ssd < 2.0 ** 287


@pytest.mark.parametrize("W", [1, 4, 64])
@pytest.mark.parametrize("pool", POOLS)
def test_parts_equal_the_whole(engine, W, pool):
    a = rows_with_edges(W)
    R = -(-N // pool)
    whole = engine.spread_fold(a, pool)
    out = engine.spread_finish(whole)
    for at in range(N + 1):
        into = engine.spread_init(W, R)
        engine.spread_fold(a[at:], pool, at=at, into=into)            # the later part first: the order is free
        engine.spread_fold(a[:at], pool, at=0, into=into)
        assert into.tobytes() == whole.tobytes(), at
        x = engine.spread_fold(a[:at], pool, into=engine.spread_init(W, R))
        y = engine.spread_fold(a[at:], pool, at=at, into=engine.spread_init(W, R))
        assert engine.spread_merge(x, y).tobytes() == whole.tobytes(), at
        assert same(engine.spread_finish(x), out)
    rng = np.random.default_rng(pool * 100 + W)
    into = engine.spread_init(W, R)
    for i in rng.permutation(N):
        engine.spread_fold(a[i:i + 1], pool, at=int(i), into=into)
    assert into.tobytes() == whole.tobytes() and same(engine.spread_finish(into), out)
    b = a.copy()
    for r in range(R):
        b[r * pool:(r + 1) * pool] = a[r * pool:(r + 1) * pool][rng.permutation(min((r + 1) * pool, N) - r * pool)]
    assert engine.spread_fold(b, pool).tobytes() == whole.tobytes()


@pytest.mark.parametrize("W", WIDTHS)
def test_one_row(engine, referee, W):
    a = rows_with_edges(W)
    ref = referee(W, N)
    for pool in (N, N + 1, 50, 1 << 31, 1 << 40):
        got = twin5(engine, a, pool)
        assert got[0].shape == (1, W) and same(got[:3], ref)


def test_each_output_alone(engine):
    a = rows_with_edges(4)
    acc = engine.spread_fold(a, 3)
    ref = engine.spread_finish(acc)
    for which, name in enumerate(NAMES):
        got = engine.spread_finish(acc, outputs=(name,))
        assert [g is not None for g in got] == [i == which for i in range(5)]
        assert got[which].tobytes() == ref[which].tobytes(), name
    got = engine.spread_finish(acc, outputs=("std", "rms"))
    assert same(got, (ref[0], None, None, None, ref[4])) and got[1] is None and got[3] is None
    with pytest.raises(ValueError):
        engine.spread_finish(acc, outputs=("variance",))


def test_error_codes(engine):
    from quadrs_amd import _ffi
    L, INVALID = _ffi.lib(), _ffi.ERR_INVALID
    a = rows_with_edges(4)
    with pytest.raises(engine.QuadrsError) as e:
        engine.spread_fold(a, 0, into=engine.spread_init(4, 1))
    assert e.value.code == INVALID
    acc = engine.spread_init(4, 1)
    ap, norms = acc.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)
    out = np.zeros(4, F32)
    rows = _ffi.SpreadRows(out.ctypes.data, None, None, None, None)
    none = _ffi.SpreadRows(None, None, None, None, None)
    assert L.qd_spread_init(None, 4, 1) == INVALID and L.qd_spread_init(ap, 0, 1) == INVALID
    assert L.qd_spread_fold(ap, 4, 0, 0, norms, 1) == INVALID                        # pool 0
    assert L.qd_spread_fold(ap, 0, 1, 0, norms, 0) == INVALID                        # no width
    assert L.qd_spread_fold(None, 4, 1, 0, norms, 1) == INVALID                      # no accumulator
    assert L.qd_spread_fold(ap, 4, 1, 0, None, 1) == INVALID                         # no norms
    assert L.qd_spread_fold(ap, 4, 1, 0, None, 0) == 0                               # nothing to fold
    assert L.qd_spread_merge(None, ap, 4, 1) == INVALID and L.qd_spread_merge(ap, None, 4, 1) == INVALID and L.qd_spread_merge(ap, ap, 0, 1) == INVALID
    assert L.qd_spread_finish(None, 4, 1, C.byref(rows)) == INVALID and L.qd_spread_finish(ap, 0, 1, C.byref(rows)) == INVALID
    assert L.qd_spread_finish(ap, 4, 1, C.byref(none)) == INVALID and L.qd_spread_finish(ap, 4, 1, None) == INVALID     # no output at all
    assert not acc.any() and not out.any()
    # a count driven to 2^31 by hand: one more window is refused and nothing changes, whichever half of word 27 holds the count
    a = np.ones((8, 4), F32)
    norms = a.ctypes.data_as(C.c_void_p)
    for full in (1 << 31, (1 << 31) << 32, ((1 << 30) << 32) + (1 << 30)):
        acc = engine.spread_fold(a[:2], 5, into=engine.spread_init(4, 2))
        acc[0, 1, 27] = full
        before = acc.copy()
        assert L.qd_spread_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 2, norms, 1) == INVALID
        assert acc.tobytes() == before.tobytes()
        assert L.qd_spread_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 5, norms, 3) == 0        # the other row still takes windows
        before = acc.copy()
        other = engine.spread_fold(a[:1], 5, into=engine.spread_init(4, 2))
        assert L.qd_spread_merge(acc.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p), 4, 2) == INVALID
        assert L.qd_spread_merge(other.ctypes.data_as(C.c_void_p), acc.ctypes.data_as(C.c_void_p), 4, 2) == INVALID
        assert acc.tobytes() == before.tobytes()
    acc[0, 1, 27] = (1 << 31) - 1                                                   # room for exactly one
    assert L.qd_spread_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 2, norms, 1) == 0
    with pytest.raises(ValueError):
        engine.spread_merge(engine.spread_init(4, 2), engine.spread_init(4, 1))


def test_plan_level_refusals_precede_any_gpu_call(engine):
    """qd_plan_spread without a plan is refused before anything else is looked at, as every plan call is."""
    from quadrs_amd import _ffi
    out = np.full(4, F32(-7.5))
    rows = _ffi.SpreadRows(out.ctypes.data, None, None, None, None)
    rc = _ffi.lib().qd_plan_spread(None, None, _ffi.MEM_HOST, 0, 0, 0, 1, 1, C.byref(rows), _ffi.MEM_HOST, None)
    assert rc == _ffi.ERR_INVALID and (out == F32(-7.5)).all()


def test_the_kernels_keep_their_cells_in_registers(engine):
    """hipcc's resource remarks of the build that produced the library: k_spread and k_spread_finish without scratch and without spills"""
    from quadrs_amd import build as B
    if not os.path.exists(B.RESOURCES) or os.path.getmtime(B.RESOURCES) < os.path.getmtime(B.OUT) - 600:
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    mine = {k: v for k, v in res.items() if "k_spread" in k}
    assert len(mine) == 2 and any("k_spread_finish" in k for k in mine), sorted(mine)
    for k, v in mine.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
