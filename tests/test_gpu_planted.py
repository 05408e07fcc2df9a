"""The device folds of a norms plan (qd_plan_mean, _power, _spread, _pool, _summarize, _density) on planted values: streams of impulse
windows (tests/util.py: a window whose first sample is (a, 0) has the norm |a| in every bin, which test_planted_streams_cpu.py holds to
the oracle and the first test here to the device) let every bin's cell receive chosen f32 patterns, so the rounding ties, the trap above
a tie that f64 cannot see, sticky bits across all limbs, cancellation pairs, every exponent, every bucket end, +inf and all-NaN groups
reach the fold kernels — at the widths where their geometry changes and at depths whose rows are stored whole, stored after the LDS
meeting, or cut and finished from the limb accumulator (test_planted_streams_cpu.py says which is which).  Every comparison is byte for
byte: with the Python-integer referees of the CPU fold tests, with the CPU twin on the device's own norms, and with the literal patterns
the CPU tests carry."""
import numpy as np
import pytest

import test_density_cpu as D
import test_mean_cpu as M
import test_power_cpu as P
import test_spread_cpu as S
import util
from util import PLANT_INF, PLANT_MAX, PLANT_NAN

pytestmark = pytest.mark.gpu

F32 = np.float32
SR = util.PLANTED_SR
SHAPES = [(W, depth) for W in util.PLANTED_WIDTHS for depth in util.planted_depths(W)]
QS = (0.0, 0.5, 1.0)


def f64_bits(x):
    return int(np.float64(x).view(np.uint64))


# per sink: cell -> (f32 bits, f64 bits, count) by the integer referee, evaluated once per cell
_REF = {"mean": {}, "power": {}, "spread": {}}


def referee(sink, cell):
    key = tuple(cell)
    if key not in _REF[sink]:
        if sink == "spread":
            _REF[sink][key] = S.ref_cell(cell)
        else:
            bits, total, count = (M if sink == "mean" else P).ref_cell(cell)
            _REF[sink][key] = (bits, f64_bits(total), count)
    return _REF[sink][key]


def literals():
    """per sink: cell -> (f32 bits or None, f64 bits or None), the expected patterns that the CPU tests state as literals"""
    lit = {"mean": {}, "power": {}, "spread": {}}
    for vals, want_mean, want_sum, _ in M.PLANTED_CASES:
        lit["mean"][tuple(vals)] = (want_mean, None if want_sum is None else f64_bits(want_sum))
    for vals, want in zip(P.PLANTED_CASES, P.PLANTED_WANT_RMS):
        lit["power"][tuple(vals)] = (want, None)
    for vals, want in zip(P.PLANTED_TIES, P.PLANTED_TIES_SUMSQ):
        lit["power"][tuple(vals)] = (None, f64_bits(want))
    for vals, want in zip(S.PLANTED_CASES, S.PLANTED_WANT):
        lit["spread"][tuple(vals)] = (want, None)
    lit["spread"][tuple(S.PLANTED_CASES[5])] = (0x3F000000, f64_bits(S.PAIR24_SSD))
    for vals in S.PLANTED_EQUAL:
        lit["spread"][tuple(vals)] = (0, 0)                      # all equal: std +0, ssd 0.0
    return {k: {c: w for c, w in v.items() if util.plantable(c)} for k, v in lit.items()}


LITERALS = literals()


class Stream:
    """one planted stream: its cells, bytes, matrix of planted bits, the two plans, the device copy and the plan's own norms"""

    def __init__(self, engine, cells, depth, W):
        import torch
        self.cells, self.depth, self.W = cells, depth, W
        self.data, self.m = util.cases_stream(cells, depth, W)
        self.n = self.m.size
        n_samples = len(self.data) // 8
        self.plan = engine.Plan(engine.FMT_CF32, SR, n_samples, width=W)
        self.small = engine.Plan(engine.FMT_CF32, SR, n_samples, width=W, chunk_bytes=util.PLANTED_SMALL_CHUNK)
        assert self.plan.n_windows == self.n == self.plan.complete_windows()
        self.dev = torch.frombuffer(bytearray(self.data), dtype=torch.uint8).cuda()
        self.norms = self.plan.run_host(self.data)
        self.norms.setflags(write=False)
        self.refs = {}

    def ref(self, sink):
        """(f32 bits uint32[R], f64 bits uint64[R], count uint32[R]) by the integer referee"""
        if sink not in self.refs:
            r = [referee(sink, c) for c in self.cells]
            self.refs[sink] = (np.array([x[0] for x in r], np.uint32), np.array([x[1] for x in r], np.uint64), np.array([x[2] for x in r], np.uint32))
        return self.refs[sink]


@pytest.fixture(scope="module")
def streams(engine):
    cache = {}

    def get(W, depth):
        if (W, depth) not in cache:
            cache[W, depth] = Stream(engine, util.planted_case_set(W, depth), depth, W)
        return cache[W, depth]
    return get


def host(t):
    import torch
    torch.cuda.synchronize()
    out = [None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else x) for x in t]
    return tuple(x.view(np.uint32) if x is not None and x.dtype == np.int32 else x for x in out)      # a torch count_rows is int32: the same bits


def bits_of(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_rows(got, ref, what):
    """every bin of row c of the (R, W) array `got` holds the pattern ref[c]"""
    g = bits_of(got)
    assert g.shape == (ref.size, got.shape[1]) and g.dtype == ref.dtype, what
    bad = np.flatnonzero((g != ref[:, None]).any(axis=1))
    assert bad.size == 0, (what, int(bad[0]), [hex(int(x)) for x in g[bad[0], :4]], hex(int(ref[bad[0]])))


def assert_planted(norms, m):
    """the norms rows (n, W) hold the planted pattern of their window in every bin (a planted NaN: a NaN)"""
    bits, want = norms.view(np.uint32), m.reshape(-1)
    assert norms.shape[0] == want.size
    nan = want == PLANT_NAN
    assert np.isnan(norms[nan]).all()
    assert (bits[~nan] == want[~nan][:, None]).all()


def check_sink(s, sink, got, twin, names=(0, 1, 2)):
    """the outputs `names` of got = (f32, f64, u32, ...) against the referee, the CPU twin on the device's norms and the literals"""
    ref = s.ref(sink)
    for k in names:
        assert_rows(got[k], ref[k], (sink, s.W, s.depth, k, "referee"))
        assert got[k].dtype == twin[k].dtype and got[k].tobytes() == twin[k].tobytes(), (sink, s.W, s.depth, k, "twin")
    seen = 0
    for c, cell in enumerate(s.cells):
        want = LITERALS[sink].get(tuple(cell))
        if want is None:
            continue
        seen += 1
        for k in (0, 1):
            if want[k] is not None and k in names:
                assert (bits_of(got[k])[c] == want[k]).all(), (sink, c, k, hex(int(bits_of(got[k])[c, 0])), hex(want[k]))
    return seen


@pytest.mark.parametrize("W,depth", SHAPES)
def test_the_plans_norms_are_the_planted_values(engine, streams, W, depth):
    """the precondition of everything below: qd_plan_run gives every window's planted pattern in every bin, from either plan and from
    the device copy; and the batches of the second plan are the ones test_planted_streams_cpu.py classifies"""
    import torch
    s = streams(W, depth)
    assert len(s.data) < util.PLANTED_CAP and s.norms.shape == (s.n, W)
    assert_planted(s.norms, s.m)
    assert_planted(s.small.run_host(s.data), s.m)
    out = torch.empty(s.n, W, dtype=torch.float32, device="cuda")
    s.plan.run_device(s.dev, out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == s.norms.tobytes()
    for p in (s.plan, s.small):
        assert util.planted_small_batch(W) % max(int(p.info.tile_windows), 1) == 0
    # the stream holds what it is for
    kinds = s.m.reshape(-1)
    assert (kinds == PLANT_NAN).any() and (kinds == 0).any() and (kinds == PLANT_MAX).any()
    if depth >= 16:
        assert tuple(P.TRAP) in {tuple(c) for c in s.cells} and (kinds == PLANT_INF).any() and (kinds == 1).any()


@pytest.mark.parametrize("W,depth", SHAPES)
def test_mean(engine, streams, W, depth):
    s = streams(W, depth)
    twin = engine.mean_finish(engine.mean_fold(s.norms, depth))
    seen = check_sink(s, "mean", host(s.plan.mean(s.dev, depth)), twin)                 # default chunk_bytes, device -> device
    assert seen == check_sink(s, "mean", s.small.mean(s.data, depth), twin)             # chunk_bytes = 64 KiB, host -> host
    assert seen >= len([c for c in LITERALS["mean"] if len(c) <= depth]) or W == 2048


@pytest.mark.parametrize("W,depth", SHAPES)
def test_power(engine, streams, W, depth):
    s = streams(W, depth)
    twin = engine.power_finish(engine.power_fold(s.norms, depth))
    got = host(s.plan.power(s.dev, depth))
    seen = check_sink(s, "power", got, twin)
    assert seen == check_sink(s, "power", s.small.power(s.data, depth), twin)
    if depth >= 16:
        # the trap discriminates on the device too: the f64 shortcut's answer is the pattern below
        c = s.cells.index(P.TRAP)
        assert P.shortcut_rms(P.TRAP) == P.TRAP_SHORTCUT_RMS == 0x31C00004 and (got[0].view(np.uint32)[c] == 0x31C00005).all()
        assert (got[0].view(np.uint32)[s.cells.index(P.PLANTED_CASES[0])] == 0x31C00002).all()       # the tie itself: to even


@pytest.mark.parametrize("W,depth", SHAPES)
def test_spread(engine, streams, W, depth):
    s = streams(W, depth)
    twin = engine.spread_finish(engine.spread_fold(s.norms, depth))
    got = host(s.plan.spread(s.dev, depth))
    seen = check_sink(s, "spread", got, twin)
    assert seen == check_sink(s, "spread", s.small.spread(s.data, depth), twin)
    # std alone: the kernel skips the work of the absent outputs
    for alone in (host(s.plan.spread(s.dev, depth, outputs=("std",))), s.small.spread(s.data, depth, outputs=("std",))):
        assert [x is None for x in alone] == [False, True, True, True, True]
        check_sink(s, "spread", alone, twin, names=(0,))
    # the folds agree with each other: the cell's halves are the mean's and the power's, from either ending of a row
    for p, src in ((s.plan, s.dev), (s.small, s.data)):
        mean, power = host(p.mean(src, depth)), host(p.power(src, depth))
        five = host(p.spread(src, depth))
        assert five[3].tobytes() == mean[0].tobytes() and five[4].tobytes() == power[0].tobytes()
        assert bits_of(five[2]).tobytes() == bits_of(mean[2]).tobytes() == bits_of(power[2]).tobytes()
    assert_rows(got[3], s.ref("mean")[0], "spread's mean rows by the mean's referee")
    assert_rows(got[4], s.ref("power")[0], "spread's rms rows by the power's referee")
    std, rms = got[0], got[4]
    assert ((std <= rms) | np.isnan(std)).all()
    assert (np.isnan(std) == np.isnan(bits_of(got[1]).view(np.float64)) | (bits_of(got[2]) == 0)).all()
    equal = [c for c, cell in enumerate(s.cells) if len(cell) >= 1 and len(set(cell)) == 1 and cell[0] < PLANT_INF]
    assert len(equal) >= 18 or W == 2048
    assert not std.view(np.uint32)[equal].any() and not bits_of(got[1])[equal].any()


@pytest.mark.parametrize("W", util.PLANTED_WIDTHS)
def test_pool_one_returns_the_value(engine, W):
    """pool == 1 over the value classes: the value itself as mean and rms, sum == (double) v, sumsq == (double) v (double) v, std +0.
    Left out of test_power_cpu.VALUE_CLASSES, which an impulse cannot plant: the members with a sign bit (0x80000000, 0x80000001,
    0x807FFFFF, 0x80800000, 0xFF7FFFFF, 0xFFC00000, 0xFFFFFFFF, 0xFF800000) and the NaN with a payload 0x7F800001."""
    vals = [b for b in P.VALUE_CLASSES if util.plantable([b])]
    assert vals == [0, 1, 0x007FFFFF, 0x00800000, PLANT_MAX, PLANT_NAN, PLANT_INF, 0x3F800000, 0x3FC00001]
    s = Stream(engine, [[b] for b in vals], 1, W)
    assert_planted(s.norms, s.m)
    bits = np.array(vals, np.uint32)
    d = bits.view(F32).astype(np.float64)
    nan, inf = bits == PLANT_NAN, bits == PLANT_INF
    value = np.where(nan, np.uint32(PLANT_NAN), bits).astype(np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        total = np.where(nan, 0.0, d).view(np.uint64)
        sumsq = np.where(nan, 0.0, d * d).view(np.uint64)
    count = (~nan).astype(np.uint32)
    for p, src in ((s.plan, s.dev), (s.small, s.data)):
        mean, power, five = host(p.mean(src, 1)), host(p.power(src, 1)), host(p.spread(src, 1))
        assert_rows(mean[0], value, "mean"), assert_rows(mean[1], total, "sum"), assert_rows(mean[2], count, "count")
        assert_rows(power[0], value, "rms"), assert_rows(power[1], sumsq, "sumsq"), assert_rows(power[2], count, "count")
        assert_rows(five[3], value, "spread mean"), assert_rows(five[4], value, "spread rms"), assert_rows(five[2], count, "spread count")
        assert_rows(five[0], np.where(nan | inf, np.uint32(PLANT_NAN), np.uint32(0)).astype(np.uint32), "std")
        assert_rows(five[1], np.where(inf, np.uint64(S.NAN64_BITS), np.uint64(0)).astype(np.uint64), "ssd")
        for sink, got in (("mean", mean), ("power", power), ("spread", five)):
            for k in (0, 1, 2):
                assert_rows(got[k], s.ref(sink)[k], (sink, k, "referee"))


@pytest.fixture(scope="module")
def sweeps(engine):
    """the bucket sweep at width W: one Stream per part (tests/util.py, bucket_sweep_parts), every window a cell of its own"""
    cache = {}

    def get(W):
        if W not in cache:
            cache[W] = [Stream(engine, [[int(b)] for b in part], 1, W) for part in util.bucket_sweep_parts(W)]
        return cache[W]
    return get


@pytest.mark.parametrize("W", util.PLANTED_WIDTHS)
def test_peaks_floors_and_histogram_over_the_bucket_sweep(engine, sweeps, W):
    """both ends of every bucket of the summary's scale: integer max / min of the planted patterns per group of two and over a whole part,
    and every bucket of the histogram on the device"""
    parts = sweeps(W)
    hist = np.zeros(2048, dtype=np.uint64)
    for i, s in enumerate(parts):
        assert_planted(s.norms, s.m)
        bits = s.m.reshape(-1)
        last = i == len(parts) - 1
        assert not (bits == PLANT_NAN).any() and (bits == PLANT_INF).any() == last
        for p, src in ((s.plan, s.dev), (s.small, s.data)):
            for pool in (2, s.n):
                peak, floor = host(p.pool(src, pool))
                R = -(-s.n // pool)
                pad = np.concatenate([bits, np.repeat(bits[-1:], R * pool - s.n)]).reshape(R, pool)
                assert_rows(peak, pad.max(axis=1), ("peak", pool)), assert_rows(floor, pad.min(axis=1), ("floor", pool))
            sm = p.summarize(src)
            want = np.bincount(bits >> 20, minlength=2048).astype(np.uint64) * np.uint64(W)
            assert sm.hist.dtype == np.uint64 and (sm.hist == want).all() and sm.n_nan == 0 and sm.n_windows == s.n
            assert int(F32(sm.max).view(np.uint32)) == int(bits.max()) and int(F32(sm.min).view(np.uint32)) == int(bits.min())
            assert (sm.peak.view(np.uint32) == bits.max()).all() and (sm.floor.view(np.uint32) == bits.min()).all()
            if last:
                assert int(F32(sm.max).view(np.uint32)) == PLANT_INF and bits[-2] == PLANT_MAX
                cut = p.summarize(src, n_windows=s.n - 1)          # the +inf window left out
                assert int(F32(cut.max).view(np.uint32)) == PLANT_MAX and cut.hist[2040] == 0 and cut.hist[2039] == 2 * W
        hist += sm.hist
        if i == 0:
            assert int(F32(sm.min).view(np.uint32)) == 0
    assert (hist[:2040] == 2 * W).all() and hist[2040] == W and not hist[2041:].any()


def planted_rows(m, W):
    """the norms rows (n, W) that an impulse stream of the planted matrix gives, as float32"""
    return np.broadcast_to(m.reshape(-1)[:, None], (m.size, W)).view(F32)


@pytest.mark.parametrize("W", util.PLANTED_WIDTHS)
def test_density_over_the_bucket_sweep(engine, sweeps, W):
    """pool = n over every part of the sweep and pool = 2 over pairs of bucket ends around both edges of each grid: the counts against
    test_density_cpu.ref_counts of the planted matrix, the traces against ref_quantile; both clamps are hit"""
    low = high = 0
    for level0, L in util.PLANTED_GRIDS:
        for s in sweeps(W):
            ref = D.ref_counts(planted_rows(s.m, 1), s.n, level0, L)                                # (1, 1, L): every bin alike
            traces = np.stack([D.ref_quantile(ref, level0, q)[0].view(np.uint32) for q in QS])      # (3, 1, 1)
            k = s.m.reshape(-1) >> 20
            below, above = int((k < level0).sum()), int((k > level0 + L - 1).sum())
            low, high = low + below, high + above
            for p, src in ((s.plan, s.dev), (s.small, s.data)):
                counts, tr = host(p.density(src, s.n, level0, L, q=QS))
                counts = counts.view(np.uint32)
                assert counts.shape == (1, W, L) and (counts == ref).all(), (level0, L)
                assert tr.shape == (3, 1, W) and (tr.view(np.uint32) == traces).all(), (level0, L)
                # what lies outside the grid is in its first and in its last level
                first, end = below + int((k == level0).sum()), above + int((k == level0 + L - 1).sum())
                assert (counts[0, :, 0] == (first if L > 1 else s.n)).all() and (counts[0, :, L - 1] == (end if L > 1 else s.n)).all()
        buckets = util.density_pair_buckets(level0, L, W)
        cells = [[k << 20, (k << 20) | 0xFFFFF] if k < 2040 else [PLANT_INF] for k in buckets]
        s = Stream(engine, cells, 2, W)
        assert_planted(s.norms, s.m)
        ref = D.ref_counts(planted_rows(s.m, 1), 2, level0, L)                                      # (R, 1, L)
        traces = np.stack([D.ref_quantile(ref, level0, q)[0].view(np.uint32) for q in QS])          # (3, R, 1)
        at = np.clip(np.array(buckets), level0, level0 + L - 1) - level0
        assert (ref[np.arange(len(buckets)), 0, at] == [len(c) for c in cells]).all() and ref.sum() == sum(len(c) for c in cells)
        assert (traces[0] == traces[2]).all() and (traces[0, :, 0] == np.where(at == 0, 0, (level0 + at) << 20)).all()
        for p, src in ((s.plan, s.dev), (s.small, s.data)):
            counts, tr = host(p.density(src, 2, level0, L, q=QS))
            assert counts.shape == (len(buckets), W, L) and (counts.view(np.uint32) == ref).all(), (level0, L)
            assert tr.shape == (3, len(buckets), W) and (tr.view(np.uint32) == traces).all(), (level0, L)
        low, high = low + int((np.array(buckets) < level0).sum()), high + int((np.array(buckets) > level0 + L - 1).sum())
        if (level0, L) in ((1000, 64), (1500, 1)):
            assert min(buckets) < level0 and max(buckets) > level0 + L - 1
    assert low > 0 and high > 0
