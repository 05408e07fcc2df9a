"""The RMS-trace rows' host half (include/quadrs_hip.h, "RMS-trace rows"): qd_power_init / _fold / _merge / _finish against a referee written
here with Python integers — the exact sum of squares per cell in units of 2^-298, its f64 by one correctly rounded conversion of that
integer, and the f32 root from math.isqrt plus an exact comparison with both f32 neighbours (no float division and no float sqrt anywhere
in the referee) — the planted rounding cases, parts == whole in every order, and the error codes.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from test_pool_cpu import F32, N, POOLS, WIDTHS, rows_with_edges

NAN_BITS, INF_BITS, MAX_BITS = 0x7FC00000, 0x7F800000, 0x7F7FFFFF
WORDS = 19


def units(bits):
    """a non-negative f32's value (the pattern 0x7f800000 read as 2^128) as an integer count of 2^-149"""
    e, m = bits >> 23, bits & 0x7FFFFF
    return (m | (1 << 23) if e else m) << (max(e, 1) - 1)


def root_f32(num, den):
    """the bit pattern of sqrt(num / den) (num an integer count of 2^-298, den >= 1) rounded to f32, nearest, ties to even: X =
    isqrt(num // den) is floor(sqrt(num / den)) in units of 2^-149, the largest f32 at or below it is lo, and lo^2 den <= num < up^2 den for
    its successor up; 4 num against den (lo + up)^2 picks the nearer, the even pattern on a tie"""
    X = math.isqrt(num // den)
    L = X.bit_length()
    b = X if L <= 24 else ((L - 24) << 23) + (X >> (L - 24))
    assert b <= MAX_BITS
    lo, up = units(b), units(b + 1)
    assert lo * lo * den <= num < up * up * den
    mid = den * (lo + up) ** 2
    if 4 * num != mid:
        return b if 4 * num < mid else b + 1
    return b if b % 2 == 0 else b + 1


def exact_sumsq(bits):
    """the sum of squares of a cell's finite values as an integer count of 2^-298"""
    return sum(units(int(b) & 0x7FFFFFFF) ** 2 for b in bits if int(b) & 0x7FFFFFFF < INF_BITS)


def ref_cell(bits):
    """(rms bits, f64 sum of squares, count) of one cell's values, given as u32 bit patterns (any sign, NaNs included)"""
    vals = [int(b) & 0x7FFFFFFF for b in bits]
    vals = [b for b in vals if b <= INF_BITS]
    if not vals:
        return NAN_BITS, 0.0, 0
    if INF_BITS in vals:
        return INF_BITS, math.inf, len(vals)
    total = exact_sumsq(vals)
    return root_f32(total, len(vals)), math.ldexp(float(total), -298), len(vals)      # float(int) rounds once, to nearest even; ldexp is exact


def ref_power(norms, pool, at=0):
    """(rms_rows, sumsq_rows, count_rows) of rows (at + i) // pool of the norms rows (n, W), by ref_cell"""
    a = np.ascontiguousarray(norms, dtype=F32).view(np.uint32)
    n, W = a.shape
    R = -(-(at + n) // pool)
    rms, total, count = np.empty((R, W), np.uint32), np.empty((R, W), np.float64), np.empty((R, W), np.uint32)
    for r in range(R):
        lo, hi = max(r * pool - at, 0), min((r + 1) * pool - at, n)
        for c in range(W):
            rms[r, c], total[r, c], count[r, c] = ref_cell(a[lo:hi, c])
    return rms.view(F32), total, count


def same3(got, ref):
    return all(g.shape == r.shape and g.dtype == r.dtype and g.tobytes() == r.tobytes() for g, r in zip(got, ref)) and len(got) == len(ref) == 3


@pytest.fixture(scope="module")
def referee():
    cache = {}

    def get(W, pool):
        if (W, pool) not in cache:
            cache[W, pool] = ref_power(rows_with_edges(W), pool)
        return cache[W, pool]
    return get


def test_init(engine):
    acc = engine.power_init(5, 3)
    assert acc.shape == (3, 5, WORDS) and acc.dtype == np.uint64 and not acc.any()
    acc[:] = 7
    from quadrs_amd import _ffi
    assert _ffi.POWER_WORDS == WORDS
    assert _ffi.lib().qd_power_init(acc.ctypes.data_as(C.c_void_p), 5, 2) == 0 and not acc[:2].any() and (acc[2] == 7).all()
    rms, total, count = engine.power_finish(engine.power_init(2, 2))
    assert (rms.view(np.uint32) == NAN_BITS).all() and not total.any() and not np.signbit(total).any() and not count.any()


def test_the_limbs_are_the_documented_ones(engine):
    """word by word: v = m m << (2 s mod 32) in three 32-bit pieces from limb 2 s / 32 on, the count word as the mean's"""
    vals = [0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3FC00001, 0x7F7FFFFF, 0x80000003, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFFFFFFF]
    acc = engine.power_fold(np.array([vals], dtype=np.uint32).view(F32), 1)
    for c, b in enumerate(vals):
        want = [0] * WORDS
        b &= 0x7FFFFFFF
        e, m = b >> 23, b & 0x7FFFFF
        if e == 255:
            want[18] = (1 << 32) if m == 0 else 0
        else:
            m |= (1 << 23) if e else 0
            sh = 2 * (max(e, 1) - 1)
            v = (m * m) << (sh & 31)
            j = sh >> 5
            want[j], want[j + 1], want[j + 2], want[18] = v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF, v >> 64, 1
        assert [int(x) for x in acc[0, c]] == want, hex(b)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("pool", POOLS)
def test_fold_and_finish_match_the_referee(engine, referee, W, pool):
    a = rows_with_edges(W)
    assert np.isnan(a).any() and np.isinf(a).any() and (a == 0).any() and ((a > 0) & (a < F32(1.2e-38))).any()
    got = engine.power_finish(engine.power_fold(a, pool))
    assert got[0].shape == (-(-N // pool), W)
    assert same3(got, referee(W, pool))
    if pool == 1:
        keep = ~np.isnan(a)
        d = np.abs(a).astype(np.float64)
        assert got[0][keep].tobytes() == np.abs(a)[keep].tobytes()
        with np.errstate(over="ignore"):
            assert got[1][keep].tobytes() == (d * d)[keep].tobytes()                   # a 48-bit product: exact in f64
        assert (got[2] == keep).all() and (got[0].view(np.uint32)[~keep] == NAN_BITS).all() and not got[1][~keep].any()


VALUE_CLASSES = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,
                 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x3F800000, 0x3FC00001]


def test_pool_one_identities_over_the_value_classes(engine):
    vals = VALUE_CLASSES
    a = np.array([vals], dtype=np.uint32)
    rms, total, count = engine.power_finish(engine.power_fold(a.view(F32), 1))
    for c, b in enumerate(vals):
        mag = b & 0x7FFFFFFF
        got = (int(rms.view(np.uint32)[0, c]), float(total[0, c]), int(count[0, c]))
        if mag > INF_BITS:
            assert got == (NAN_BITS, 0.0, 0), hex(b)
        elif mag == INF_BITS:
            assert got == (INF_BITS, math.inf, 1), hex(b)
        else:
            d = float(np.uint32(mag).view(F32))
            assert got == (mag, d * d, 1) and got == ref_cell([b]), hex(b)
            assert got[1] == 0.0 or got[1] >= 2.0 ** -298                              # zero or a normal f64
        assert not math.copysign(1.0, got[1]) < 0


def fold_cells(engine, cases):
    """one cell per column: the values of cases[c], padded with NaN (which adds nothing), folded into one row"""
    depth = max(len(v) for v in cases)
    rows = np.full((depth, len(cases)), NAN_BITS, dtype=np.uint32)
    for c, vals in enumerate(cases):
        rows[:len(vals), c] = vals
    acc = engine.power_fold(rows.view(F32), depth)
    rms, total, count = engine.power_finish(acc)
    return [(int(rms.view(np.uint32)[0, c]), float(total[0, c]), int(count[0, c])) for c in range(len(cases))], acc


def shortcut_rms(vals):
    """(float)sqrt(sum of (double)v^2 / count): what the f64 shortcut gives"""
    s = 0.0
    for b in vals:
        d = float(np.uint32(b).view(F32))
        s += d * d
    return int(F32(math.sqrt(s / len(vals))).view(np.uint32))


def _planted_cases():
    x1, x3 = (100 << 23) | 1, (100 << 23) | 3
    tie = [x1] * 9 + [0] * 7                                       # root 3 x / 4 exactly: halfway between two f32
    trap = [x3] * 9 + [0] * 6 + [(40 << 23) | 0x123456]            # just above a tie, by less than f64 sees
    big, small = (150 << 23) | 0x7FFFFF, (120 << 23) | 1
    running = [big] + [small] * 1000
    ends = [MAX_BITS, 1]                                           # bits in the first and in the last limb of one cell
    cases = [tie, trap, [1, 0, 0, 0], [3, 0, 0, 0], [5, 0, 0, 0], [7, 0, 0, 0], [MAX_BITS] * 3, running, ends, [MAX_BITS, MAX_BITS, 1],
             [NAN_BITS, NAN_BITS | 0x80000000], [0x3F800000, INF_BITS, NAN_BITS], [0x80000000], [0xBF800000, 0x3F800000]]
    want_rms = [0x31C00002, 0x31C00005, 0, 2, 2, 4, MAX_BITS, None, None, None, NAN_BITS, INF_BITS, 0, 0x3F800000]
    return cases, want_rms


# shared with the GPU's planted streams (tests/util.py, planted_cells)
PLANTED_CASES, PLANTED_WANT_RMS = _planted_cases()
TRAP, TRAP_SHORTCUT_RMS = PLANTED_CASES[1], 0x31C00004            # what the f64 shortcut gives for the trap
# an exact f64 tie in the highest limb that only the lowest limb breaks: the sticky bit crosses all of them
P127, P100 = 254 << 23, 227 << 23                                 # 2^127 and 2^100: squares 2^254 and 2^200, twice the latter half an ulp
PLANTED_TIES = [[P127, P100, P100], [P127, P100, P100, 1], [P127, P100, P100, P100]]
PLANTED_TIES_SUMSQ = [2.0 ** 254, 2.0 ** 254 + 2.0 ** 202, 2.0 ** 254 + 2.0 ** 202]


def test_planted_rounding_cases(engine):
    cases, want_rms = PLANTED_CASES, PLANTED_WANT_RMS
    trap, running = TRAP, PLANTED_CASES[7]
    got, acc = fold_cells(engine, cases)
    for c, vals in enumerate(cases):
        ref = ref_cell(vals)
        assert got[c] == ref, (c, got[c], ref)
        assert want_rms[c] is None or got[c][0] == want_rms[c], (c, hex(got[c][0]))
        assert not math.copysign(1.0, got[c][1]) < 0
    # the trap discriminates: the f64 shortcut rounds it the other way (and gets the plain tie's neighbour right)
    assert shortcut_rms(trap) == TRAP_SHORTCUT_RMS == 0x31C00004 and got[1][0] == 0x31C00005
    # the top of the range: the sum of squares of three largest values is finite in f64
    assert math.isfinite(got[6][1]) and got[6][1] == 3 * float(np.uint32(MAX_BITS).view(F32)) ** 2
    # a running f64 sum of squares in window order is not the exact one
    s = 0.0
    for b in running:
        d = float(np.uint32(b).view(F32))
        s += d * d
    assert s != got[7][1] and got[7][1] == math.ldexp(float(exact_sumsq(running)), -298)
    # the first and the last limb of one cell both hold bits, and the lowest one decides the sticky bit of the f64
    assert acc[0, 8, 0] != 0 and acc[0, 8, 17] != 0 and not acc[0, 8, 1:15].any()
    ties = PLANTED_TIES
    tie_sum, acc2 = fold_cells(engine, ties)
    assert tie_sum[0][1] == 2.0 ** 254 and tie_sum[1][1] == 2.0 ** 254 + 2.0 ** 202 and tie_sum[2][1] == 2.0 ** 254 + 2.0 ** 202
    assert [t[1] for t in tie_sum] == PLANTED_TIES_SUMSQ
    assert acc2[0, 1, 0] == 1 and acc2[0, 1, 17] != 0
    for c, vals in enumerate(ties):
        assert tie_sum[c] == ref_cell(vals)


def random_cells(n_cells=300, seed=2024):
    """cells of every size class with exponents drawn wide and narrow, so that candidates start at either side of their root"""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n_cells):
        n = int(rng.choice([1, 2, 3, 4, 5, 7, 16, 33]))
        e0 = int(rng.integers(0, 255))
        spread = int(rng.choice([0, 1, 3, 30]))
        e = np.clip(e0 + rng.integers(-spread, spread + 1, n), 0, 254).astype(np.uint32)
        m = rng.integers(0, 1 << 23, n).astype(np.uint32)
        if i % 3 == 0:
            m &= np.uint32(0x7)                                     # short mantissas: exact squares and ties happen
        cases.append([int(x) for x in (e << 23) | m])
    return cases


def test_random_cells_match_the_referee(engine):
    """random_cells(): 300 cells, seed 2024"""
    cases = random_cells()
    assert len(cases) == 300
    got, _ = fold_cells(engine, cases)
    for c, vals in enumerate(cases):
        assert got[c] == ref_cell(vals), (c, [hex(v) for v in vals])


@pytest.mark.parametrize("W", [1, 4, 64])
@pytest.mark.parametrize("pool", POOLS)
def test_parts_equal_the_whole(engine, W, pool):
    a = rows_with_edges(W)
    R = -(-N // pool)
    whole = engine.power_fold(a, pool)
    out = engine.power_finish(whole)
    for at in range(N + 1):
        into = engine.power_init(W, R)
        engine.power_fold(a[at:], pool, at=at, into=into)            # the later part first: the order is free
        engine.power_fold(a[:at], pool, at=0, into=into)
        assert into.tobytes() == whole.tobytes(), at
        # two accumulators, merged
        x = engine.power_fold(a[:at], pool, into=engine.power_init(W, R))
        y = engine.power_fold(a[at:], pool, at=at, into=engine.power_init(W, R))
        assert engine.power_merge(x, y).tobytes() == whole.tobytes(), at
        assert same3(engine.power_finish(x), out)
    # the windows of each group in a shuffled order, one call per window
    rng = np.random.default_rng(pool * 100 + W)
    into = engine.power_init(W, R)
    for i in rng.permutation(N):
        engine.power_fold(a[i:i + 1], pool, at=int(i), into=into)
    assert into.tobytes() == whole.tobytes() and same3(engine.power_finish(into), out)
    b = a.copy()
    for r in range(R):
        b[r * pool:(r + 1) * pool] = a[r * pool:(r + 1) * pool][rng.permutation(min((r + 1) * pool, N) - r * pool)]
    assert engine.power_fold(b, pool).tobytes() == whole.tobytes()


@pytest.mark.parametrize("W", WIDTHS)
def test_one_row(engine, referee, W):
    a = rows_with_edges(W)
    ref = referee(W, N)
    for pool in (N, N + 1, 50, 1 << 31, 1 << 40):
        got = engine.power_finish(engine.power_fold(a, pool))
        assert got[0].shape == (1, W) and same3(got, ref)


def test_one_output_only(engine):
    from quadrs_amd import _ffi
    a = rows_with_edges(4)
    acc = engine.power_fold(a, 3)
    ref = engine.power_finish(acc)
    for which in range(3):
        out = np.zeros_like(ref[which])
        ptrs = [None, None, None]
        ptrs[which] = out.ctypes.data_as(C.c_void_p)
        assert _ffi.lib().qd_power_finish(acc.ctypes.data_as(C.c_void_p), 4, acc.shape[0], *ptrs) == 0
        assert out.tobytes() == ref[which].tobytes()


def test_error_codes(engine):
    from quadrs_amd import _ffi
    L, INVALID = _ffi.lib(), _ffi.ERR_INVALID
    a = rows_with_edges(4)
    with pytest.raises(engine.QuadrsError) as e:
        engine.power_fold(a, 0, into=engine.power_init(4, 1))
    assert e.value.code == INVALID
    acc = engine.power_init(4, 1)
    ap, norms = acc.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)
    out = np.zeros(4, F32)
    op = out.ctypes.data_as(C.c_void_p)
    assert L.qd_power_init(None, 4, 1) == INVALID and L.qd_power_init(ap, 0, 1) == INVALID
    assert L.qd_power_fold(ap, 4, 0, 0, norms, 1) == INVALID                        # pool 0
    assert L.qd_power_fold(ap, 0, 1, 0, norms, 0) == INVALID                        # no width
    assert L.qd_power_fold(None, 4, 1, 0, norms, 1) == INVALID                      # no accumulator
    assert L.qd_power_fold(ap, 4, 1, 0, None, 1) == INVALID                         # no norms
    assert L.qd_power_fold(ap, 4, 1, 0, None, 0) == 0                               # nothing to fold
    assert L.qd_power_merge(None, ap, 4, 1) == INVALID and L.qd_power_merge(ap, None, 4, 1) == INVALID and L.qd_power_merge(ap, ap, 0, 1) == INVALID
    assert L.qd_power_finish(None, 4, 1, op, None, None) == INVALID and L.qd_power_finish(ap, 0, 1, op, None, None) == INVALID
    assert L.qd_power_finish(ap, 4, 1, None, None, None) == INVALID                 # all outputs NULL
    assert not acc.any() and not out.any()
    # a count driven to 2^31 by hand: one more window is refused and nothing changes, whichever half of word 18 holds the count
    a = np.ones((8, 4), F32)
    norms = a.ctypes.data_as(C.c_void_p)
    for full in (1 << 31, (1 << 31) << 32, ((1 << 30) << 32) + (1 << 30)):
        acc = engine.power_fold(a[:2], 5, into=engine.power_init(4, 2))
        acc[0, 1, 18] = full
        before = acc.copy()
        assert L.qd_power_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 2, norms, 1) == INVALID
        assert acc.tobytes() == before.tobytes()
        assert L.qd_power_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 5, norms, 3) == 0         # the other row still takes windows
        before = acc.copy()
        other = engine.power_fold(a[:1], 5, into=engine.power_init(4, 2))
        assert L.qd_power_merge(acc.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p), 4, 2) == INVALID
        assert L.qd_power_merge(other.ctypes.data_as(C.c_void_p), acc.ctypes.data_as(C.c_void_p), 4, 2) == INVALID
        assert acc.tobytes() == before.tobytes()
    acc[0, 1, 18] = (1 << 31) - 1                                                   # room for exactly one
    assert L.qd_power_fold(acc.ctypes.data_as(C.c_void_p), 4, 5, 2, norms, 1) == 0
    with pytest.raises(ValueError):
        engine.power_merge(engine.power_init(4, 2), engine.power_init(4, 1))


def test_plan_level_refusals_precede_any_gpu_call(engine):
    """qd_plan_power without a plan is refused before anything else is looked at, as every plan call is."""
    from quadrs_amd import _ffi
    out = np.full(4, F32(-7.5))
    rc = _ffi.lib().qd_plan_power(None, None, _ffi.MEM_HOST, 0, 0, 0, 1, 1, out.ctypes.data_as(C.c_void_p), None, None, _ffi.MEM_HOST, None)
    assert rc == _ffi.ERR_INVALID and (out == F32(-7.5)).all()
