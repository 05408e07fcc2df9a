"""Cascaded stage lists on the GPU (qd_plan_create_stages, qd_cascade.h) against the oracle's nested Samples.

Shift-free cascades are bit-exact on every bin; with a shift the NCO multipliers may round ~1e-8 of the time the other way
(DESIGN.md section 4), so those chains use assert_norms_close's default bound.  Every sub-range / slab / chunk / shard run
of a cascade plan equals its whole-stream run byte for byte: each NCO sits on absolute rows of its own stage's index."""
import numpy as np
import pytest

from test_gpu_parity import _signal, _to_format, assert_codes_edge_aware, assert_norms_close

pytestmark = pytest.mark.gpu

SR = 2_000_000
SHAPES = {
    "LS": [("lowpass", (200_000, 4, 40)), ("shift", 30_000)],
    "LL": [("lowpass", (200_000, 4, 40)), ("lowpass", (30_000, 4, 64))],
    "SLL": [("shift", 300_000), ("lowpass", (200_000, 4, 40)), ("lowpass", (30_000, 4, 64))],
    "LLS": [("lowpass", (200_000, 4, 40)), ("lowpass", (30_000, 4, 64)), ("shift", -20_000)],
    "SLSLS": [("shift", 300_000), ("lowpass", (200_000, 4, 40)), ("shift", 15_000), ("lowpass", (30_000, 4, 64)), ("shift", 3_000)],
}
PROBE = [("lowpass", (100_000, 4, 40)), ("lowpass", (10_000, 8, 200))]


def _oracle(O, data, fmt, stages, sr=SR):
    ch = O.Chain.from_bytes(data, fmt, sr)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch


def _has_shift(stages):
    return any(k == "shift" for k, _ in stages)


def _check_norms(ref, got, stages, what):
    if _has_shift(stages):
        assert_norms_close(ref, got, what)
    else:
        assert_norms_close(ref, got, what, min_exact=1.0, max_ulp=0.0)


def _data(fmt, n, seed=5):
    return _to_format(_signal(np.random.default_rng(seed), n), fmt)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("W", [4, 16, 128, 1024])
@pytest.mark.parametrize("sk", ["S=W", "S=W/4", "S=2W"])
def test_cascade_norms_cf32(engine, oracle, shape, W, sk):
    stages = SHAPES[shape]
    S = {"S=W": W, "S=W/4": max(W // 4, 1), "S=2W": 2 * W}[sk]
    n = 120_000 if W < 1024 else 400_000
    data = _data(0, n)
    plan = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S)
    assert plan.complete_windows() == plan.n_windows
    assert "k_cascade" in plan.kernel_name()
    got = plan.run_host(data)
    ref, _ = _oracle(oracle, data, 0, stages).spark_fft(W, S, want_codes=False)
    _check_norms(ref, got, stages, f"cascade {shape} W={W} S={S}")


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_cascade_norms_formats(engine, oracle, shape, fmt):
    stages, W, S, n = SHAPES[shape], 64, 16, 150_000
    data = _data(fmt, n, seed=fmt)
    plan = engine.Plan(fmt, SR, n, stages=stages, width=W, stride=S)
    got = plan.run_host(data)
    ref, _ = _oracle(oracle, data, fmt, stages).spark_fft(W, S, want_codes=False)
    _check_norms(ref, got, stages, f"cascade {shape} fmt={fmt}")


@pytest.mark.parametrize("shape", ["LL", "SLSLS"])
def test_cascade_glyph_and_bucket(engine, oracle, shape):
    stages, W, S, n = SHAPES[shape], 32, 8, 150_000
    data = _data(0, n, seed=11)
    ch = _oracle(oracle, data, 0, stages)
    rmin, rmax = 0.0005, 0.02
    ref_norms, ref_codes = ch.spark_fft(W, S, rng=(rmin, rmax))
    codes = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_GLYPH_U8, rng=(rmin, rmax)).run_host(data)
    assert_codes_edge_aware(ref_codes, codes, ref_norms, rmin, rmax, f"cascade glyph {shape}")
    levels = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_BUCKET2_U8).run_host(data)
    ref_levels = ch.freq_levels(W, S)
    assert levels.shape == ref_levels.shape
    nat = np.roll(ref_norms[: len(ref_levels)].astype(np.float64), W // 2, axis=1)      # fftshift undone: natural bin order
    first, second = nat[:, : W // 2].sum(axis=1), nat[:, W // 2:].sum(axis=1)
    tie = np.abs(first - second) <= 8 * np.spacing(np.maximum(first, second).astype(np.float32)).astype(np.float64)
    diff = levels != ref_levels
    assert not (diff & ~tie).any(), np.nonzero(diff & ~tie)


def test_cascade_envelope(engine, oracle):
    # 512 * 15 + 500 = 8 180 intermediate samples per window: inside the 8 192 envelope
    stages = [("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 15, 500))]
    n, W, S = 400_000, 512, 512
    data = _data(0, n, seed=3)
    plan = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S)
    got = plan.run_host(data)
    ref, _ = _oracle(oracle, data, 0, stages).spark_fft(W, S, want_codes=False)
    assert got.shape[0] >= 8
    _check_norms(ref, got, stages, "cascade envelope 8180")
    # 512 * 16 + 200 = 8 392: just past it
    with pytest.raises(engine.QuadrsError) as ei:
        engine.Plan(engine.FMT_CF32, SR, n, stages=[("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 16, 200))], width=W, stride=S)
    assert ei.value.code == engine._ffi.ERR_UNSUPPORTED


@pytest.mark.parametrize("shape", ["LL", "SLSLS", "LS"])
def test_cascade_same_bytes_as_whole_run(engine, shape):
    import torch
    stages, W, S = SHAPES[shape], 128, 32
    n = 2_000_000
    data = _data(0, n, seed=7)
    plan = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S)
    whole = plan.run_host(data)
    nw = plan.n_windows
    assert nw > 1000
    # window sub-ranges from an offset slab
    for w0, cnt in ((1, 7), (333, 501), (nw - 19, 19)):
        s0, sc = plan.src_range(w0, cnt)
        slab = np.frombuffer(data, dtype=np.uint8)[s0 * 8:(s0 + sc) * 8]
        assert plan.run_host(slab, first_window=w0, n_windows=cnt, src_first=s0).tobytes() == whole[w0:w0 + cnt].tobytes()
    # device buffers, twice on the same buffers
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.empty(nw, W, dtype=torch.float32, device="cuda")
    for _ in range(2):
        out.zero_()
        plan.run_device(src, out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == whole.tobytes()
    # the host path in many small chunks
    small = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S, chunk_bytes=1 << 16)
    assert small.run_host(data).tobytes() == whole.tobytes()
    assert small.stats().chunks > 100
    # 2 and 4 shards on one device
    for k in (2, 4):
        sh = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S, shard_devices=[0] * k)
        assert sh.run_sharded_host(data).tobytes() == whole.tobytes()
    # determinism
    assert plan.run_host(data).tobytes() == whole.tobytes()


@pytest.mark.parametrize("n", [20_036, 20_040])
def test_cascade_failing_tail(engine, oracle, n):
    """The probe chain (two lowpasses at 1 MHz, sparkfft -width 4): at 20 036 samples the last window fails read_exact_at
    (LowPass::len over-reports), at 20 040 it does not.  The complete windows are written, bit-exact, then QD_ERR_SHORT."""
    sr = 1_000_000
    data = _data(0, n, seed=13)
    ch = _oracle(oracle, data, 0, PROBE, sr)
    plan = engine.Plan(engine.FMT_CF32, sr, n, stages=PROBE, width=4, stride=4)
    total = plan.n_windows
    done = total
    while done and ch.read_at((done - 1) * 4, 4)[0] != 4:
        done -= 1
    assert plan.complete_windows() == done
    assert (done < total) == (n == 20_036)
    ref, _ = ch.spark_fft(4, 4, max_windows=done, want_codes=False)
    out = np.full((total, 4), np.nan, dtype=np.float32)
    if done < total:
        with pytest.raises(engine.QuadrsError) as ei:
            plan.run_host(data, out=out)
        assert ei.value.code == engine._ffi.ERR_SHORT
        assert np.isnan(out[done:]).all()
        with pytest.raises(RuntimeError):
            ch.spark_fft(4, 4, want_codes=False)      # the oracle fails on the same window
    else:
        plan.run_host(data, out=out)
    assert out[:done].tobytes() == ref.tobytes()


def test_routed_stage_list_is_todays_plan(engine):
    n, W, S = 300_000, 64, 16
    data = _data(0, n, seed=17)
    one = engine.Plan(engine.FMT_CF32, 21_000_000, n, shift_hz=280_000, lowpass=(200_000, 32, 400), width=W, stride=S)
    st = engine.Plan(engine.FMT_CF32, 21_000_000, n, stages=[("shift", 280_000), ("lowpass", (200_000, 32, 400))], width=W, stride=S)
    assert st.kernel_name() == one.kernel_name()
    assert st.run_host(data).tobytes() == one.run_host(data).tobytes()
    assert st.complete_windows() == st.n_windows
    assert st.stage_taps(1).tobytes() == one.taps().tobytes()


def test_cascade_fast_mode_runs_exact(engine):
    stages, n, W = SHAPES["LL"], 200_000, 128
    data = _data(0, n, seed=19)
    exact = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W)
    fast = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, mode=engine.MODE_FAST)
    assert not (fast.info.kernel_flags & (1 << 14))
    assert fast.run_host(data).tobytes() == exact.run_host(data).tobytes()
    taps = engine.lowpass_design(30_000, SR // 4, 64)
    assert fast.stage_taps(1).tobytes() == taps.tobytes()
