"""Cascaded stage lists on the GPU (qd_plan_create_stages, qd_cascade.h) against the oracle's nested Samples.

Shift-free cascades are bit-exact on every bin; with a shift an NCO multiplier component may round the other way where it is
ambiguous, so those chains keep assert_norms_close's default bound AND the NCO rule: norms, glyph cells
and bucket digits may differ only in windows that read an ambiguous multiplier of one of the chain's shifts.  Every sub-range / slab / chunk / shard run
of a cascade plan equals its whole-stream run byte for byte: each NCO sits on absolute rows of its own stage's index."""
import numpy as np
import pytest

from test_gpu_parity import _signal, _to_format, assert_codes_edge_aware, assert_digits_explained, assert_norms_close

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


def _check_norms(ref, got, stages, what, W, S, sr=SR, first_window=0):
    if _has_shift(stages):
        assert_norms_close(ref, got, what, explain=((stages, W, S, sr), first_window))
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
    _check_norms(ref, got, stages, f"cascade {shape} W={W} S={S}", W, S)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_cascade_norms_formats(engine, oracle, shape, fmt):
    stages, W, S, n = SHAPES[shape], 64, 16, 150_000
    data = _data(fmt, n, seed=fmt)
    plan = engine.Plan(fmt, SR, n, stages=stages, width=W, stride=S)
    got = plan.run_host(data)
    ref, _ = _oracle(oracle, data, fmt, stages).spark_fft(W, S, want_codes=False)
    _check_norms(ref, got, stages, f"cascade {shape} fmt={fmt}", W, S)


@pytest.mark.parametrize("shape", ["LL", "SLSLS"])
def test_cascade_glyph_and_bucket(engine, oracle, shape):
    stages, W, S, n = SHAPES[shape], 32, 8, 150_000
    data = _data(0, n, seed=11)
    ch = _oracle(oracle, data, 0, stages)
    rmin, rmax = 0.0005, 0.02
    ref_norms, ref_codes = ch.spark_fft(W, S, rng=(rmin, rmax))
    codes = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_GLYPH_U8, rng=(rmin, rmax)).run_host(data)
    ex = ((stages, W, S, SR), 0) if _has_shift(stages) else None
    assert_codes_edge_aware(ref_codes, codes, ref_norms, rmin, rmax, f"cascade glyph {shape}", explain=ex)
    levels = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_BUCKET2_U8).run_host(data)
    ref_levels = ch.freq_levels(W, S)
    assert levels.shape == ref_levels.shape
    nat = np.roll(ref_norms[: len(ref_levels)].astype(np.float64), W // 2, axis=1)      # fftshift undone: natural bin order
    first, second = nat[:, : W // 2].sum(axis=1), nat[:, W // 2:].sum(axis=1)
    tie = np.abs(first - second) <= 8 * np.spacing(np.maximum(first, second).astype(np.float32)).astype(np.float64)
    diff = levels != ref_levels
    assert not (diff & ~tie).any(), np.nonzero(diff & ~tie)
    if ex:
        assert_digits_explained(ref_levels, levels, ex, f"cascade bucket {shape}")


def test_cascade_envelope(engine, oracle):
    # 512 * 15 + 500 = 8 180 intermediate samples per window: inside the 8 192 envelope
    stages = [("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 15, 500))]
    n, W, S = 400_000, 512, 512
    data = _data(0, n, seed=3)
    plan = engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W, stride=S)
    got = plan.run_host(data)
    ref, _ = _oracle(oracle, data, 0, stages).spark_fft(W, S, want_codes=False)
    assert got.shape[0] >= 8
    _check_norms(ref, got, stages, "cascade envelope 8180", W, S)
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


# ------------------------------------------------------------------ the whole envelope: a seeded fuzzer and its edges

def test_cascade_fuzz_against_oracle(engine, oracle):
    """Seeded random cascades (util.fuzz_cascade_shapes) against the oracle; the draw must reach every FIR class of both stages,
    T % 8 != 0 in both, and a source sub-tile below 512 outputs, so a new seed cannot quietly drop coverage."""
    from test_gpu_parity import record_observed
    from util import fuzz_cascade_shapes
    cov, obs = {}, {}
    checked, bad = fuzz_cascade_shapes(engine, 160, 20261015, oracle, cov=cov, observed=obs)
    frac = obs["exact"] / max(obs["bins"], 1)
    record_observed("cascade fuzz (norms sinks)", bins=obs["bins"], exact_fraction=frac, worst_ulp_of_window_max=obs["worst_ulp"],
                    fir1_classes=sorted(cov["cls1"]), fir2_classes=sorted(cov["cls2"]),
                    halved_sub_tiles=sorted(m for m in cov["M"] if m[0] and m[0] < m[1]),
                    shapes=sorted(cov["shapes"]), failing_tails=cov["short"])
    assert checked >= 150 and not bad, bad
    assert frac >= 0.9999 and obs["worst_ulp"] <= 1.0, (frac, obs["worst_ulp"])
    assert cov["cls1"] >= {0, 2, 4, 8, -1} and cov["cls2"] >= {0, 2, 4, 8, -1}, cov
    assert True in cov["t1_mod8"] and True in cov["t2_mod8"], cov
    assert any(m and m < start for m, start in cov["M"]), cov["M"]        # cascade_init halved the sub-tile (T1 x D1, LDS)


def _sub_tile(plan):
    import re
    return int(re.search(r"M (\d+)\)", plan.kernel_name()).group(1))


def _stream_len(stages, W, S, n_win):
    """a stream of exactly n_win complete windows (the first window's source span, n_win - 1 source steps, a short remainder)"""
    span, step = W, S
    for kind, arg in reversed(stages):
        if kind == "lowpass":
            span, step = span * arg[1] + arg[2], step * arg[1]
    return span + (n_win - 1) * step + 3


def _whole_vs_oracle(engine, oracle, stages, W, S, n_win, fmt=0, sr=SR, seed=23, what="", M_below=None, ratio=None):
    """n_win windows' worth of stream, every window against the oracle's nested chain"""
    n = _stream_len(stages, W, S, n_win)
    data = _data(fmt, n, seed=seed)
    plan = engine.Plan(fmt, sr, n, stages=stages, width=W, stride=S)
    assert "k_cascade" in plan.kernel_name() and plan.complete_windows() == plan.n_windows == n_win
    if M_below is not None:
        assert _sub_tile(plan) < M_below, plan.kernel_name()
    if ratio is not None:
        assert plan.info.ratio == ratio
    got = plan.run_host(data)
    ref, _ = _oracle(oracle, data, fmt, stages, sr).spark_fft(W, S, want_codes=False)
    _check_norms(ref, got, stages, what or f"cascade {stages} W={W} S={S}", W, S, sr)
    return plan


@pytest.mark.parametrize("stages,W", [
    ([("lowpass", (100_000, 16, 4096)), ("lowpass", (5_000, 6, 40))], 64),           # n2 = 424: M = 212
    ([("lowpass", (100_000, 16, 4096)), ("shift", -20_000)], 512),                   # n2 = 512: M = 256
])
def test_cascade_first_stage_4096_taps(engine, oracle, stages, W):
    """T1 = 4096, the largest first stage, with D1 = 16: the sub-tile halves below 512 outputs to stay inside 8192 source samples"""
    _whole_vs_oracle(engine, oracle, stages, W, W, 12, M_below=512, what=f"cascade T1=4096 W={W}")


@pytest.mark.parametrize("stages", [
    [("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 15, 512))],                  # 512 * 15 + 512, D2 odd
    [("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 14, 1024))],                 # 512 * 14 + 1024, D2 even: the most pads
    [("shift", -500_000), ("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 14, 1024)), ("shift", 1_234)],
])
def test_cascade_inter_block_8192(engine, oracle, stages):
    """n2 = 8192 intermediate samples, exactly the envelope"""
    _whole_vs_oracle(engine, oracle, stages, 512, 384, 10, what=f"cascade n2=8192 D2={stages[-1 if stages[-1][0] == 'lowpass' else -2][1][1]}")


@pytest.mark.parametrize("shape,W", [("LL", 1), ("LL", 2), ("LS", 1), ("LS", 2), ("LS", 4096), ("LS", 8192), ("SLS", 4096), ("SLS", 8192)])
def test_cascade_width_edges(engine, oracle, shape, W):
    """W = 1 and 2 (no Radix4 layer; a one-bin half for the bucket) and W = 4096 / 8192 without a second lowpass (n2 = W), every sink"""
    stages = {"LL": SHAPES["LL"], "LS": SHAPES["LS"], "SLS": [("shift", 300_000)] + SHAPES["LS"]}[shape]
    S = max(1, W // 2) if W > 2 else 1
    n_win = 40 if W <= 2 else 6
    _whole_vs_oracle(engine, oracle, stages, W, S, n_win, what=f"cascade {shape} W={W}")
    # glyph codes and bucket digits at the same widths
    n = _stream_len(stages, W, S, n_win)
    data = _data(0, n, seed=W)
    ch = _oracle(oracle, data, 0, stages)
    ref_norms, _ = ch.spark_fft(W, S, want_codes=False)
    rmin, rmax = (float(x) for x in np.percentile(ref_norms, [20, 90]))
    rmax = max(rmax, 1.5 * rmin + 1e-6)
    ref_norms, ref_codes = ch.spark_fft(W, S, rng=(rmin, rmax))
    codes = engine.Plan(0, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_GLYPH_U8, rng=(rmin, rmax)).run_host(data)
    ex = ((stages, W, S, SR), 0) if _has_shift(stages) else None
    assert_codes_edge_aware(ref_codes, codes, ref_norms, rmin, rmax, f"cascade glyph {shape} W={W}", explain=ex)
    levels = engine.Plan(0, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_BUCKET2_U8).run_host(data)
    ref_levels = ch.freq_levels(W, S)
    assert levels.shape == ref_levels.shape
    from util import bucket_digits_ok
    assert bucket_digits_ok(ref_norms[: len(ref_levels)], levels)
    assert _has_shift(stages) or np.array_equal(levels, ref_levels)
    if ex:
        assert_digits_explained(ref_levels, levels, ex, f"cascade bucket {shape} W={W}")


FAR = [("shift", 280_000), ("lowpass", (2_000_000, 4, 40)), ("shift", 15_000), ("lowpass", (200_000, 8, 200)), ("shift", -3_000)]


@pytest.mark.parametrize("fmt,N,at", [(0, 1 << 34, (1 << 34) - (1 << 24)), (1, 1 << 33, (1 << 32) + 777_777)])
def test_cascade_far_offset_slab(engine, oracle, fmt, N, at):
    """SLSLS windows deep in the stream (cf32 near the end of 2^34 samples; cs8 past 2^32 source samples): each NCO's row
    table sits far from 0 on its own stage's index.  Reference: the oracle's primitives at absolute indices, stage by stage."""
    sr, W, S = 21_000_000, 64, 16
    D1, T1, D2, T2 = 4, 40, 8, 200
    p = engine.Plan(fmt, sr, N, stages=FAR, width=W, stride=S)
    w0, nwin = at // (S * D2 * D1), 24
    first, count = p.src_range(w0, nwin)
    assert first > (1 << 32)
    rng = np.random.default_rng(fmt + 41)
    bps = 8 if fmt == 0 else 2
    if fmt == 0:
        raw = (rng.standard_normal((count, 2)) * 0.03).astype(np.float32).tobytes()
    else:
        raw = rng.integers(0, 256, count * bps, dtype=np.uint8).tobytes()
    got = p.run_host(raw, w0, nwin, src_first=first)
    x = oracle.unpack(fmt, raw)
    r = [oracle.shift_ratio(FAR[0][1], sr), oracle.shift_ratio(FAR[2][1], sr // D1), oracle.shift_ratio(FAR[4][1], sr // D1 // D2)]
    h1, h2 = oracle.taps(2_000_000, sr, T1), oracle.taps(200_000, sr // D1, T2)
    n2 = W * D2 + T2
    ref = np.empty_like(got)
    for i in range(nwin):
        o = (w0 + i) * S
        b2, b1 = o * D2, o * D2 * D1
        src = oracle.shift_apply(x[b1 - first:b1 - first + n2 * D1 + T1], b1, r[0])
        k, inter = oracle.lowpass_block(h1, D1, src)
        assert k == n2
        k, outer = oracle.lowpass_block(h2, D2, oracle.shift_apply(inter, b2, r[1]))
        assert k == W
        y = oracle.fft(oracle.shift_apply(outer, o, r[2]))
        ref[i] = oracle.norm(y)[np.r_[W // 2:W, 0:W // 2]]
    assert_norms_close(ref, got, f"cascade far slab fmt={fmt} at {first}", explain=((FAR, W, S, sr), w0))


@pytest.mark.parametrize("edge", [False, True])
def test_cascade_rates_not_divisible(engine, oracle, edge):
    """2 000 003 Hz through /3 and /7: each stage's rate truncates (666 667, 95 238 Hz) and every NCO ratio uses the truncated rate;
    shifts after each filter, ordinary or at +-(rate/2 - 1) of their own stage"""
    sr = 2_000_003
    r1, r2 = sr // 3, sr // 3 // 7
    f1, f2 = (r1 // 2 - 1, -(r2 // 2 - 1)) if edge else (111_111, -12_345)
    stages = [("lowpass", (300_000, 3, 42)), ("shift", f1), ("lowpass", (40_000, 7, 66)), ("shift", f2)]
    plan = _whole_vs_oracle(engine, oracle, stages, 128, 96, 30, sr=sr, what=f"cascade sr={sr} edge={edge}",
                            ratio=oracle.shift_ratio(f1, r1))
    assert plan.info.out_sample_rate == r2


def test_cascade_zero_hz_first_shift(engine, oracle):
    """a 0 Hz first shift: the plan reports ITS ratio (0), not the next shift's, and the bytes are the oracle's"""
    stages = [("shift", 0), ("lowpass", (200_000, 4, 40)), ("shift", 20_000), ("lowpass", (30_000, 4, 64)), ("shift", -3_000)]
    _whole_vs_oracle(engine, oracle, stages, 64, 64, 40, ratio=0.0, what="cascade 0 Hz first shift")
    info, _ = engine.stages_geometry(0, SR, 1 << 20, stages, width=64)
    assert info.ratio == 0.0


@pytest.mark.parametrize("how", ["chunked", "sharded"])
def test_cascade_failing_tail_chunked_and_sharded(engine, oracle, how):
    """The probe chain at 20 036 samples (its last window fails read_exact_at) through 64 KiB host chunks and through 2 shards:
    QD_ERR_SHORT, every complete window bit-exact, the failing window untouched"""
    sr, n = 1_000_000, 20_036
    data = _data(0, n, seed=13)
    ch = _oracle(oracle, data, 0, PROBE, sr)
    kw = dict(chunk_bytes=1 << 16) if how == "chunked" else dict(shard_devices=[0, 0])
    plan = engine.Plan(engine.FMT_CF32, sr, n, stages=PROBE, width=4, stride=4, **kw)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    ref, _ = ch.spark_fft(4, 4, max_windows=done, want_codes=False)
    out = np.full((total, 4), np.nan, dtype=np.float32)
    with pytest.raises(engine.QuadrsError) as ei:
        plan.run_host(data, out=out) if how == "chunked" else plan.run_sharded_host(data, out=out)
    assert ei.value.code == engine._ffi.ERR_SHORT
    assert out[:done].tobytes() == ref.tobytes()
    assert np.isnan(out[done:]).all()
    if how == "chunked":
        assert plan.stats().chunks > 1


def test_cascade_odd_taps_nan(engine, oracle):
    """An odd tap count puts 0/0 in the middle of the reference's windowed sinc: every tap is NaN.  NaN positions, glyph codes and
    bucket digits equal the oracle's."""
    stages = [("lowpass", (200_000, 4, 41)), ("shift", 10_000), ("lowpass", (30_000, 4, 64))]
    W, S = 32, 16
    n = 60_000
    data = _data(0, n, seed=29)
    ch = _oracle(oracle, data, 0, stages)
    assert np.isnan(oracle.taps(200_000, SR, 41)).all()
    rmin, rmax = 0.001, 0.05
    ref_norms, ref_codes = ch.spark_fft(W, S, rng=(rmin, rmax))
    got = engine.Plan(0, SR, n, stages=stages, width=W, stride=S).run_host(data)
    assert got.shape == ref_norms.shape and np.array_equal(np.isnan(got), np.isnan(ref_norms))
    ok = ~np.isnan(ref_norms)
    assert got[ok].tobytes() == ref_norms[ok].tobytes()
    codes = engine.Plan(0, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_GLYPH_U8, rng=(rmin, rmax)).run_host(data)
    assert np.array_equal(codes, ref_codes)
    levels = engine.Plan(0, SR, n, stages=stages, width=W, stride=S, epilogue=engine.EPI_BUCKET2_U8).run_host(data)
    assert np.array_equal(levels, ch.freq_levels(W, S))
