"""Windowed FFT sinks on the GPU (qd_chain_desc.windowing = 1: Blackman-Harris in front of the transform) against the reference's own
take_fft: oracle.Chain.take_fft(W, n, (0, n S), windowing=1) over the same stage list steps by exactly S, so it returns the windowed
rows at 0, S, 2S, ... — each read by the read_exact_at a spark_fft window is read by, the lowpass truncating against that read.

Shift-free chains compare bit for bit.  Shifted chains keep assert_norms_close's default bound and the NCO rule,
as the cascade and rows tests do.  Every plan here passes windowing=1 (the rectangular control apart)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cascade import SHAPES as CASC, SR as CASC_SR, _data, _has_shift, _oracle
from test_gpu_footprint import _one_run
from test_gpu_parity import _signal, _to_format, assert_codes_edge_aware, assert_norms_close
from util import POISON_WORDS, footprint_violations

pytestmark = pytest.mark.gpu

SR = 21_000_000
BH = 1
WINDOWED = 4194304            # qd_plan_info.kernel_flags bit 22
CAP = 384                     # windows a case compares (several tiles of every tiling, several workgroups)
LP_SHORT, LP_LONG = (2_000_000, 16, 40), (200_000, 32, 400)      # both have truncated outputs inside the window (T / 2 >= D)


def _stages(shift, lp):
    return ([("shift", shift)] if shift is not None else []) + ([("lowpass", lp)] if lp is not None else [])


def referee(chain, W, S, n_windows, cap=CAP):
    """the reference's windowed rows at 0, S, 2S, ...: as many of the plan's windows as take_fft's slice rules admit (visible >
    output_len, end < len), at most cap.  Returns float32[n, W]."""
    ln = chain.len()
    n = min(int(n_windows), cap, (ln - W) // S + 1)
    assert n >= 1, (ln, W, S, n_windows)
    if S == 1:                                          # visible > output_len needs a step of 2: the even rows, then the odd ones
        m = min(n // 2, (ln - 2) // 2)
        assert m >= 1
        rc0, even, o0 = chain.take_fft(W, m, (0, 2 * m), BH)
        rc1, odd, o1 = chain.take_fft(W, m, (1, 2 * m + 1), BH)
        assert rc0 == 0 and rc1 == 0, (rc0, rc1)
        assert np.array_equal(o0, 2 * np.arange(m, dtype=np.uint64)) and np.array_equal(o1, 2 * np.arange(m, dtype=np.uint64) + 1)
        rows = np.empty((2 * m, W), dtype=np.float32)
        rows[0::2], rows[1::2] = even, odd
        return rows
    while n > 1 and n * S >= ln:                        # the slice's end lies inside the sink
        n -= 1
    end = n * S if n * S < ln else ln - 1               # (one row: any slice from 0 puts it at 0)
    rc, rows, offs = chain.take_fft(W, n, (0, end), BH)
    assert rc == 0, rc
    assert np.array_equal(offs, S * np.arange(n, dtype=np.uint64)), offs[:8]
    return rows


def _chain(oracle, data, fmt, sr, stages):
    return _oracle(oracle, data, fmt, stages, sr)


def check(ref, got, stages, W, S, sr, what):
    assert got.shape == ref.shape and ref.shape[0] >= 1
    assert np.isfinite(ref).all() and ref.max() > 0
    if _has_shift(stages):
        assert_norms_close(ref, got, what, explain=((stages, W, S, sr), 0))
    else:
        assert_norms_close(ref, got, what, min_exact=1.0, max_ulp=0.0)


def run_case(engine, oracle, data, fmt, sr, stages, W, S, what, family=None, **plan_kw):
    n = len(data) // {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
    plan = engine.Plan(fmt, sr, n, stages=stages, width=W, stride=S, windowing=BH, **plan_kw)
    if family:
        assert family in plan.kernel_name(), plan.kernel_name()
    ref = referee(_chain(oracle, data, fmt, sr, stages), W, S, min(plan.n_windows, plan.complete_windows()))
    got = plan.run_host(data, 0, ref.shape[0])
    check(ref, got, stages, W, S, sr, what)
    return plan, ref


# ------------------------------------------------------------------ the generic kernel

@pytest.mark.parametrize("lp", [None, LP_SHORT, LP_LONG], ids=["nofir", "T40", "T400"])
@pytest.mark.parametrize("sk", ["S=W", "S=W/4", "S=2W"])
@pytest.mark.parametrize("W", [4, 16, 64, 256, 1024])
def test_generic_cf32_fsk_head(engine, oracle, fsk, W, sk, lp):
    S = {"S=W": W, "S=W/4": W // 4, "S=2W": 2 * W}[sk]
    if (lp == LP_LONG and W == 1024 and S != W) or (lp == LP_SHORT and W == 1024 and S < W):
        # 1024 * 32 + 400 source samples a window exceed one workgroup's LDS; side by side they run as a two-stage plan (DynGeo in both
        # stages), at any other stride the library has no plan for the chain, windowed or not: the same refusal.  So do 1024 * 16 + 40
        # with the shared FIR's buffers of overlapping windows.
        for windowing in (0, BH):
            with pytest.raises(engine.QuadrsError) as ei:
                engine.Plan(0, SR, len(fsk) // 8, stages=_stages(None, lp), width=W, stride=S, windowing=windowing, kernel_policy=1)
            assert ei.value.code == engine._ffi.ERR_UNSUPPORTED
        return
    run_case(engine, oracle, fsk, 0, SR, _stages(None, lp), W, S, f"window generic W={W} S={S} lp={lp}", family="DynGeo", kernel_policy=1)


@pytest.mark.parametrize("fmt,lp", [(1, LP_SHORT), (2, None), (3, LP_LONG)], ids=["cs8", "cu8", "cs16"])
def test_generic_formats(engine, oracle, fmt, lp):
    data = _to_format(_signal(np.random.default_rng(40 + fmt), 40_000), fmt)
    run_case(engine, oracle, data, fmt, SR, _stages(None, lp), 64, 16, f"window generic fmt={fmt}", family="DynGeo", kernel_policy=1)


@pytest.mark.parametrize("shift", [280000, -1234567])
@pytest.mark.parametrize("lp,S", [(None, 64), (LP_LONG, 16), (LP_SHORT, 128)], ids=["nofir", "T400-shared", "T40-gaps"])
def test_generic_shifted(engine, oracle, fsk, shift, lp, S):
    run_case(engine, oracle, fsk, 0, SR, _stages(shift, lp), 64, S, f"window generic shift={shift} lp={lp}", family="DynGeo", kernel_policy=1)


# ------------------------------------------------------------------ cascades

@pytest.mark.parametrize("shape", ["LL", "SLSLS"])
@pytest.mark.parametrize("W", [16, 128])
def test_cascades(engine, oracle, shape, W):
    run_case(engine, oracle, _data(0, 120_000), 0, CASC_SR, CASC[shape], W, W // 4, f"window cascade {shape} W={W}", family="k_cascade")


# ------------------------------------------------------------------ plan-time builds of k_chain

BUILDS = {
    # fmt, n, shift, lowpass, W, S
    "recipe-long-filter": (0, 300_000, 280000, (200_000, 32, 192), 128, 128),
    "overlapping": (3, 120_000, None, (300_000, 16, 100), 64, 32),
    "plain-D12": (0, 120_000, None, (700_000, 12, 40), 64, 64),
}


def _build_data(name):
    fmt, n = BUILDS[name][:2]
    return _to_format(_signal(np.random.default_rng(len(name)), n), fmt)


@pytest.mark.parametrize("name", sorted(BUILDS))
def test_plan_time_builds(engine, oracle, name):
    fmt, n, shift, lp, W, S = BUILDS[name]
    plan, _ = run_case(engine, oracle, _build_data(name), fmt, SR, _stages(shift, lp), W, S, f"window build {name}", family="qd::k_chain<", kernel_policy=2)
    assert plan.info.kernel_kind == 2, plan.kernel_name()
    assert plan.info.kernel_flags & WINDOWED, plan.kernel_name()
    plain = engine.Plan(fmt, SR, n, stages=_stages(shift, lp), width=W, stride=S, kernel_policy=2)
    assert not plain.info.kernel_flags & WINDOWED and plain.info.kernel_flags | WINDOWED == plan.info.kernel_flags


# ------------------------------------------------------------------ a window's bytes do not depend on the run that computes it

INVARIANT = {
    "generic": dict(fmt=0, n=300_000, sr=SR, stages=_stages(280000, LP_LONG), W=64, S=16, kw=dict(kernel_policy=1)),
    "cascade": dict(fmt=0, n=600_000, sr=CASC_SR, stages=CASC["SLSLS"], W=128, S=32, kw={}),
    "plan-time": dict(fmt=3, n=300_000, sr=SR, stages=_stages(None, (300_000, 16, 100)), W=64, S=32, kw=dict(kernel_policy=2)),
}


@pytest.mark.parametrize("name", sorted(INVARIANT))
def test_same_bytes_as_the_whole_run(engine, name):
    import torch
    c = INVARIANT[name]
    fmt, n, sr, stages, W, S, kw = c["fmt"], c["n"], c["sr"], c["stages"], c["W"], c["S"], c["kw"]
    bps = {0: 8, 3: 4}[fmt]
    data = _to_format(_signal(np.random.default_rng(7), n), fmt)
    plan = engine.Plan(fmt, sr, n, stages=stages, width=W, stride=S, windowing=BH, **kw)
    if name == "plan-time":
        assert plan.info.kernel_kind == 2 and plan.info.kernel_flags & WINDOWED
    whole = plan.run_host(data)
    nw = plan.n_windows
    assert nw > 500 and whole.any()
    rect = engine.Plan(fmt, sr, n, stages=stages, width=W, stride=S, **kw).run_host(data)
    assert (rect != whole).mean() > 0.99                               # the window is applied
    raw = np.frombuffer(data, dtype=np.uint8)
    for w0, cnt in ((1, 7), (333, 150), (nw - 19, 19)):
        s0, sc = plan.src_range(w0, cnt)
        assert plan.run_host(raw[s0 * bps:(s0 + sc) * bps], first_window=w0, n_windows=cnt, src_first=s0).tobytes() == whole[w0:w0 + cnt].tobytes()
    # a device slab that starts three samples early: neither its address nor its first sample is on a load vector
    dev = torch.from_numpy(raw.copy()).cuda()
    for w0, cnt in ((5, 200), (nw - 40, 40)):
        s0, sc = plan.src_range(w0, cnt)
        out = torch.zeros(cnt, W, dtype=torch.float32, device="cuda")
        plan.run_device(dev[(s0 - 3) * bps:(s0 + sc) * bps], out, w0, cnt, src_first=s0 - 3, src_count=sc + 3)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == whole[w0:w0 + cnt].tobytes()
    small = engine.Plan(fmt, sr, n, stages=stages, width=W, stride=S, windowing=BH, chunk_bytes=1 << 16, **kw)
    assert small.run_host(data).tobytes() == whole.tobytes()
    assert small.stats().chunks > 10
    sh = engine.Plan(fmt, sr, n, stages=stages, width=W, stride=S, windowing=BH, shard_devices=[0] * 3, **kw)
    assert sh.run_sharded_host(data).tobytes() == whole.tobytes()


# ------------------------------------------------------------------ a window larger than the LDS tile

def test_two_stage_plan(engine, oracle):
    n, W = 200_000, 1024
    data = _to_format(_signal(np.random.default_rng(3), n), 0)
    plan, ref = run_case(engine, oracle, data, 0, SR, _stages(None, (200_000, 64, 400)), W, W, "window two stages")
    assert plan.kernel_name().startswith("two stages"), plan.kernel_name()
    assert ref.shape[0] == plan.n_windows == 3


# ------------------------------------------------------------------ the other sinks, shift-free (norms are exact)

SINK_CHAINS = {"generic": (_stages(None, LP_SHORT), SR, dict(kernel_policy=1)), "cascade": (CASC["LL"], CASC_SR, {}),
               "plan-time": (_stages(None, (300_000, 16, 100)), SR, dict(kernel_policy=2))}


@pytest.mark.parametrize("name", sorted(SINK_CHAINS))
def test_glyph_mark_and_bucket_sinks(engine, oracle, name):
    stages, sr, kw = SINK_CHAINS[name]
    W, S, n = 32, 8, 150_000
    x = np.frombuffer(_data(0, n, seed=11), dtype=np.float32).reshape(-1, 2).copy()
    x[20_000:, 1] *= -1                                 # the conjugate stream: the tone changes sides, so both bucket digits occur
    data = x.tobytes()
    norms = referee(_chain(oracle, data, 0, sr, stages), W, S, 1 << 30)
    nw = norms.shape[0]
    lo, hi = float(np.quantile(norms, 0.3)), float(np.quantile(norms, 0.97))
    g = oracle.lib().qo_glyph_code
    codes = np.array([g(float(v), lo, hi) for v in norms.reshape(-1)], dtype=np.uint8).reshape(norms.shape)
    assert len(np.unique(codes)) >= 8
    mk = dict(stages=stages, width=W, stride=S, windowing=BH, **kw)
    got = engine.Plan(0, sr, n, epilogue=engine.EPI_GLYPH_U8, rng=(lo, hi), **mk).run_host(data, 0, nw)
    assert_codes_edge_aware(codes, got, norms, lo, hi, f"window glyph {name}")
    # marks: a row is blank when every cell is (src/fft.rs:54-55); min high enough that both bytes occur
    mn = float(np.quantile(norms.max(axis=1), 0.5))
    want = (norms >= np.float32(mn)).any(axis=1).astype(np.uint8)
    assert 0.2 < want.mean() < 0.8
    marks = engine.Plan(0, sr, n, epilogue=engine.EPI_MARK_U8, rng=(mn, 1.0), **mk).run_host(data, 0, nw)
    assert np.array_equal(marks, want)
    # bucket digits: two sequential f32 half sums in natural bin order (src/fft.rs:95-97)
    pb = engine.Plan(0, sr, n, epilogue=engine.EPI_BUCKET2_U8, **mk)
    nb = min(int(pb.n_windows), nw)
    digits = pb.run_host(data, 0, nb)
    nat = np.roll(norms[:nb], W // 2, axis=1)
    first = np.cumsum(nat[:, : W // 2], axis=1, dtype=np.float32)[:, -1]
    second = np.cumsum(nat[:, W // 2:], axis=1, dtype=np.float32)[:, -1]
    ref_digits = np.where(first < second, 0, 1).astype(np.uint8)
    f64a, f64b = nat[:, : W // 2].astype(np.float64).sum(axis=1), nat[:, W // 2:].astype(np.float64).sum(axis=1)
    tie = np.abs(f64a - f64b) <= 8 * np.spacing(np.maximum(f64a, f64b).astype(np.float32)).astype(np.float64)
    diff = digits != ref_digits
    assert not (diff & ~tie).any(), np.nonzero(diff & ~tie)
    assert 0 < ref_digits.mean() < 1


# ------------------------------------------------------------------ the folds of a windowed norms plan

@pytest.mark.parametrize("name", sorted(SINK_CHAINS))
def test_folds_of_a_windowed_plan(engine, oracle, name):
    stages, sr, kw = SINK_CHAINS[name]
    W, S, n = 64, 16, 150_000
    data = _data(0, n, seed=13)
    norms = referee(_chain(oracle, data, 0, sr, stages), W, S, 1 << 30)
    nw = norms.shape[0]
    plan = engine.Plan(0, sr, n, stages=stages, width=W, stride=S, windowing=BH, **kw)
    for pool in (1, 7, nw):
        got = plan.mean(data, pool, n_windows=nw, device_out=False)
        want = engine.mean_finish(engine.mean_fold(norms, pool))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), pool
    assert plan.summarize(data, n_windows=nw).tobytes() == engine.summary_fold(norms).tobytes()


# ------------------------------------------------------------------ windowing=0 is today's plan

@pytest.mark.parametrize("kw", [dict(shift_hz=280000, lowpass=LP_LONG), dict(), dict(stages=CASC["LL"])], ids=["fsk", "nofir", "cascade"])
def test_rectangular_control(engine, fsk, kw):
    a = engine.Plan(0, SR, 65536, width=64, stride=16, **kw)
    b = engine.Plan(0, SR, 65536, width=64, stride=16, windowing=engine.WINDOW_RECT, **kw)
    assert a.kernel_name() == b.kernel_name() and bytes(a.info) == bytes(b.info)
    assert a.run_host(fsk).tobytes() == b.run_host(fsk).tobytes()
    w = engine.Plan(0, SR, 65536, width=64, stride=16, windowing=BH, **kw)
    assert (w.n_windows, w.src_range(3, 9), w.info.raw_per_window, w.info.raw_step) == (a.n_windows, a.src_range(3, 9), a.info.raw_per_window, a.info.raw_step)


# ------------------------------------------------------------------ footprint: only the slab is read, only the windows are written

class _Case:
    def __init__(self, fmt, n, stages, W, S, kw):
        self.fmt, self.n, self.stages, self.W, self.S, self.kw, self.sr, self.name = fmt, n, stages, W, S, kw, SR, "window"


@pytest.mark.parametrize("name", ["generic", "plan-time"])
def test_footprint(engine, oracle, name):
    case = {"generic": _Case(0, 200_000, _stages(None, LP_LONG), 64, 16, dict(kernel_policy=1)),
            "plan-time": _Case(3, 200_000, _stages(None, (300_000, 16, 100)), 64, 32, dict(kernel_policy=2))}[name]
    data = np.frombuffer(_to_format(_signal(np.random.default_rng(5), case.n), case.fmt), dtype=np.uint8)
    plan = engine.Plan(case.fmt, SR, case.n, stages=case.stages, width=case.W, stride=case.S, windowing=BH, **case.kw)
    assert (plan.info.kernel_kind == 2 and plan.info.kernel_flags & WINDOWED) if name == "plan-time" else "DynGeo" in plan.kernel_name()
    ref = referee(_chain(oracle, data.tobytes(), case.fmt, SR, case.stages), case.W, case.S, plan.n_windows, cap=1 << 30)
    G = max(int(plan.info.tile_windows), 1)
    for w0, cnt in ((0, ref.shape[0]), (G + 1, 3 * G + 2)):          # the whole referee range; an interior range off the tile grid
        runs = [_one_run(engine, plan, case, "device", data, w0, cnt, which) for which in range(len(POISON_WORDS))]
        bad = footprint_violations(runs, ref[w0:w0 + cnt], None, 4)  # shift-free: bit for bit; no guard byte written; the source unchanged
        assert not bad, (name, w0, cnt, bad)
