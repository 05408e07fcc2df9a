"""CPU tests of stage lists (qd_plan_create_stages / qd_stages_geometry): validation per stage at its own rate, the qd_stage
layout, and the geometry of cascaded chains against the oracle's nested Samples (no device needed)."""
import ctypes as C

import numpy as np
import pytest

SR = 1_000_000
# the probe chain: lowpass -decimate 4 100000 (40 taps) | lowpass -power 100 -decimate 8 10000 | sparkfft -width 4
PROBE = [("lowpass", (100_000, 4, 40)), ("lowpass", (10_000, 8, 200))]


def _oracle_chain(O, n, stages, sr=SR):
    ch = O.Chain.from_bytes(np.zeros(n * 8, dtype=np.uint8), O.FMT_CF32, sr)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch


def _oracle_complete(O, ch, W, S, n_windows):
    """leading windows whose read_exact_at succeeds: the failures (if any) are the last windows"""
    done = n_windows
    while done > 0 and ch.read_at((done - 1) * S, W)[0] != W:
        done -= 1
    return done


def test_stage_struct_layout(engine):
    from quadrs_amd import _ffi
    assert C.sizeof(_ffi.Stage) == 40 and _ffi.MAX_STAGES == 8
    assert {"qd_plan_create_stages", "qd_plan_get_stage_taps", "qd_plan_complete_windows", "qd_stages_geometry"} <= set(_ffi.SYMBOLS)


@pytest.mark.parametrize("stages,W,S", [
    ([("lowpass", (2_000_000, 4, 40)), ("shift", 20_000)], 128, 128),
    ([("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200))], 128, 128),
    ([("shift", 280_000), ("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200))], 64, 16),
    ([("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200)), ("shift", -5_000)], 32, 64),
    ([("shift", 280_000), ("lowpass", (2_000_000, 4, 40)), ("shift", 1_000), ("lowpass", (200_000, 8, 200)), ("shift", 300)], 16, 16),
    ([("shift", 280_000), ("lowpass", (2_000_000, 16, 400))], 64, 16),          # routed: the one-stage plan's figures
])
def test_geometry_matches_oracle(engine, oracle, stages, W, S):
    n, sr = 3_000_017, 21_000_000
    ch = _oracle_chain(oracle, n, stages, sr)
    info, done = engine.stages_geometry(engine.FMT_CF32, sr, n, stages, width=W, stride=S)
    total = oracle.lib().qo_spark_window_count(ch.len(), W, S)
    assert info.n_windows == total
    assert info.decimated_len == ch.len() and info.out_sample_rate == ch.sample_rate()
    assert done == _oracle_complete(oracle, ch, W, S, total)
    D = int(np.prod([a[1] for k, a in stages if k == "lowpass"]))
    assert info.raw_step == S * D
    # the source span of a window: the innermost read of the nested stages
    span = W
    for kind, arg in reversed(stages):
        if kind == "lowpass":
            span = span * arg[1] + arg[2]
    assert info.raw_per_window == span
    first_shift = next((a for k, a in stages if k == "shift"), None)
    rate = sr
    for kind, arg in stages:
        if kind == "shift":
            break
        rate //= arg[1]
    assert info.ratio == (oracle.shift_ratio(first_shift, rate) if first_shift is not None else 0.0)
    # bucket: freq_levels' trip count (src/fft.rs:86)
    binfo, _ = engine.stages_geometry(engine.FMT_CF32, sr, n, stages, width=W, stride=S, epilogue=engine.EPI_BUCKET2_U8)
    assert binfo.n_windows == (ch.len() - W) // S


def test_probe_tail_sweep(engine, oracle):
    """Two lowpass stages: LowPass::len over-reports by one (src/filter.rs:45-48), so the sink's last window can fail
    read_exact_at.  Over lengths 20 000 ... 20 399 of the probe chain that happens at 12 lengths; the one-stage chain never fails."""
    failing = []
    for n in range(20_000, 20_400):
        ch = _oracle_chain(oracle, n, PROBE)
        total = oracle.lib().qo_spark_window_count(ch.len(), 4, 4)
        info, done = engine.stages_geometry(engine.FMT_CF32, SR, n, PROBE, width=4, stride=4)
        assert info.n_windows == total and done == _oracle_complete(oracle, ch, 4, 4, total), n
        if done < total:
            failing.append(n)
            assert total - done == 1
        one = [PROBE[0]]
        ch1 = _oracle_chain(oracle, n, one)
        info1, done1 = engine.stages_geometry(engine.FMT_CF32, SR, n, one, width=4, stride=4)
        assert done1 == info1.n_windows == oracle.lib().qo_spark_window_count(ch1.len(), 4, 4)
    assert len(failing) == 12 and {20_036, 20_039, 20_164, 20_167} <= set(failing), failing


@pytest.mark.parametrize("stages,code", [
    ([("lowpass", (100_000, 4, 40)), ("shift", 125_000)], 2),            # |f| < rate / 2 at the DECIMATED rate (250 kHz)
    ([("lowpass", (100_000, 4, 40)), ("shift", 124_999)], None),
    ([("lowpass", (100_000, 4, 40)), ("lowpass", (1_000, 0, 40))], 2),   # decimate 0
    ([("lowpass", (100_000, 4, 40)), ("lowpass", (1_000, 8, 1))], 2),    # size < 2
    ([("lowpass", (100_000, 400, 40)), ("lowpass", (1_000, 8, 3000))], 2),   # inner.len() < filter.len() of the second stage
    ([("lowpass", (100_000, 4, 40)), ("lowpass", (1_000, 2100, 40))], 2),    # sink len 125 < width 128
    ([("lowpass", (100_000, 4, 40))] * 3, 5),                            # three lowpasses: not a fused shape
    ([("lowpass", (100_000, 4, 40)), ("shift", 10), ("shift", 20)], 5),  # two shifts in a row
    ([("shift", 10), ("shift", 20)], 5),                                 # shift-only cascade
    ([("lowpass", (100_000, 2, 40)), ("lowpass", (1_000, 16, 200))], None),  # W D2 + T2 = 8 392 ... see below
])
def test_stage_validation(engine, stages, code):
    n = 1 << 20
    W = 512 if stages[-1][0] == "lowpass" and stages[-1][1][1] == 16 else 128
    kw = dict(width=W)
    if code is None and W == 512:
        # 512 * 16 + 200 = 8 392 > 8 192 intermediate samples: past the kernel's envelope
        code = 5
    if code is None:
        engine.stages_geometry(engine.FMT_CF32, SR, n, stages, **kw)
        return
    with pytest.raises(engine.QuadrsError) as ei:
        engine.stages_geometry(engine.FMT_CF32, SR, n, stages, **kw)
    assert ei.value.code == code
    with pytest.raises(engine.QuadrsError) as ei:           # plan creation validates first, before any device call
        engine.Plan(engine.FMT_CF32, SR, n, stages=stages, **kw)
    assert ei.value.code == code


def test_stages_do_not_combine_with_one_stage_fields(engine):
    with pytest.raises(ValueError):
        engine.Plan(engine.FMT_CF32, SR, 1 << 20, shift_hz=10, stages=PROBE)
    from quadrs_amd import _ffi
    d = _ffi.ChainDesc()
    d.struct_size = C.sizeof(d)
    d.sample_rate, d.n_samples, d.width, d.stride, d.has_shift = SR, 1 << 20, 128, 128, 1
    info, done = _ffi.PlanInfo(), C.c_uint64()
    st = engine.engine.stage_array(PROBE)
    assert _ffi.lib().qd_stages_geometry(C.byref(d), st, 2, C.byref(info), C.byref(done)) == _ffi.ERR_INVALID


# ------------------------------------------------------------------ seeded sweep of stage lists against the oracle

ERR_PANIC, ERR_UNSUPPORTED = 2, 5
FUSED = ("LS", "SLS", "LL", "SLL", "LSL", "SLSL", "LLS", "SLLS", "LSLS", "SLSLS")
ROUTED = ("S", "L", "SL")
UNFUSED = ("SS", "LLL", "LSS", "SSL", "LLLS", "LSLSL", "SLLL")


def _sweep_shift(rng, rate):
    """0 Hz, +-1 Hz, +-(rate/2 - 1) at the stage's own input rate, a random value, and now and then the first refused one"""
    lim = rate // 2
    pick = int(rng.integers(0, 8))
    if pick == 0:
        return 0
    if pick == 1:
        return int(rng.choice([-1, 1]))
    if pick == 2:
        return int(rng.choice([-1, 1])) * (lim - 1)
    if pick == 3 and rng.random() < 0.15:
        return int(rng.choice([-1, 1])) * lim                  # |f| == rate / 2: Shift::new panics
    return int(rng.integers(-(lim - 1), lim)) if lim > 1 else 0


def _sweep_list(rng):
    """a random stage list (shape, D, T, shifts), a sample rate the decimations need not divide, W, S and a stream length"""
    r = rng.random()
    shape = str(rng.choice(FUSED if r < 0.75 else (ROUTED if r < 0.9 else UNFUSED)))
    sr = int(rng.integers(50_000, 50_000_000))
    W = 1 << int(rng.integers(0, 11))
    S = int(rng.choice([W, max(1, W // 4), 2 * W, int(rng.integers(1, 2 * W + 1))]))
    n_l = shape.count("L")
    Ds = [int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 24, 32, int(rng.integers(1, 33))])) for _ in range(n_l)]
    Ts = []
    for k in range(n_l):
        t = int(rng.choice([2, 3, 7, 8, 9, 17, 40, 41, 64, 100, 127, 200, 256, 333, int(rng.integers(2, 600))]))
        if k == 0 and rng.random() < 0.05:
            t = int(rng.choice([4095, 4096, 4097]))
        Ts.append(t)
    # keep the oracle's reads of the last windows cheap: outer W T2 + inner n2 T1 products per window
    while True:
        n2 = W * Ds[1] + Ts[1] if n_l >= 2 else W
        if n_l == 0 or n2 * Ts[0] + W * (Ts[1] if n_l >= 2 else 0) <= 4_000_000 or W == 1:
            break
        W //= 2
        S = max(1, min(S, 2 * W))
    stages, rate, li = [], sr, 0
    for c in shape:
        if c == "S":
            stages.append(("shift", _sweep_shift(rng, rate)))
        else:
            D, T = Ds[li], Ts[li]
            li += 1
            stages.append(("lowpass", (int(rng.integers(1, max(2, rate // 2))), D, T)))
            rate //= D
            if rate < 2:
                return None
    # stream length: the source span of the first window, a few strides more, and a remainder that lands the last
    # window anywhere (complete, failing read_exact_at, or - now and then - too short for the sink)
    span, step = W, S
    for kind, arg in reversed(stages):
        if kind == "lowpass":
            span, step = span * arg[1] + arg[2], step * arg[1]
    if rng.random() < 0.04:
        n = int(rng.integers(1, span + 1))
    else:
        n = span + int(rng.integers(0, 24)) * step + int(rng.integers(0, 2 * step + 1))
    return stages, sr, n, W, S


def _expected_code(stages, sr, n, W):
    """the code a stage list must be refused with (None: accepted), from the reference's asserts, stage by stage at each stage's
    own input rate (src/shift.rs:20-24, src/filter.rs:46), the sink's len >= W (src/fft.rs:28,86), then the fused shapes and the
    kernel's envelope (n2 = W D2 + T2 <= 8192, T1 <= 4096)"""
    rate, ln = sr, n
    for kind, arg in stages:
        if kind == "shift":
            if rate == 0 or not abs(arg) < rate // 2:
                return ERR_PANIC
        else:
            if ln < arg[2]:
                return ERR_PANIC
            ln, rate = 1 + (ln - arg[2]) // arg[1], rate // arg[1]
    if ln < W:
        return ERR_PANIC
    shape = "".join(k[0].upper() for k, _ in stages)
    if shape in ("",) + ROUTED:
        return None
    if shape not in FUSED:
        return ERR_UNSUPPORTED
    lps = [a for k, a in stages if k == "lowpass"]
    n2 = W * lps[1][1] + lps[1][2] if len(lps) == 2 else W
    return ERR_UNSUPPORTED if n2 > 8192 or lps[0][2] > 4096 else None


def test_stage_list_sweep_matches_oracle(engine, oracle):
    """Seeded random stage lists (all ten fused shapes, the routed ones, unsupported ones) through qd_stages_geometry against the
    oracle's nested Samples: window counts of both sinks, complete windows, decimated_len, out_sample_rate, the FIRST shift's
    ratio (a 0 Hz first shift included), raw_per_window / raw_step; refused lists carry the reference's code."""
    rng = np.random.default_rng(0x5CA5C)
    seen, checked, refused = set(), 0, {ERR_PANIC: 0, ERR_UNSUPPORTED: 0}
    zero_first = short_tail = 0
    for _ in range(3000):
        drawn = _sweep_list(rng)
        if drawn is None:
            continue
        stages, sr, n, W, S = drawn
        shape = "".join(k[0].upper() for k, _ in stages)
        desc = f"{stages} sr={sr} n={n} W={W} S={S}"
        want = _expected_code(stages, sr, n, W)
        if want is not None:
            with pytest.raises(engine.QuadrsError) as ei:
                engine.stages_geometry(engine.FMT_CF32, sr, n, stages, width=W, stride=S)
            assert ei.value.code == want, desc
            refused[want] += 1
            continue
        info, done = engine.stages_geometry(engine.FMT_CF32, sr, n, stages, width=W, stride=S)
        # the oracle: one nested chain, stage rates read off it before each stage
        ch = oracle.Chain.from_bytes(np.zeros(n * 8, dtype=np.uint8), oracle.FMT_CF32, sr)
        first_ratio = None
        for kind, arg in stages:
            if kind == "shift":
                if first_ratio is None:
                    first_ratio = oracle.shift_ratio(arg, ch.sample_rate())
                ch = ch.shift(arg)
            else:
                ch = ch.lowpass(*arg)
        total = oracle.lib().qo_spark_window_count(ch.len(), W, S)
        assert info.n_windows == total, desc
        assert info.decimated_len == ch.len() and info.out_sample_rate == ch.sample_rate(), desc
        assert info.ratio == (first_ratio if first_ratio is not None else 0.0), f"{desc}: ratio {info.ratio} != {first_ratio}"
        want_done = _oracle_complete(oracle, ch, W, S, total)
        assert done == want_done, desc
        span, step = W, S
        for kind, arg in reversed(stages):
            if kind == "lowpass":
                span, step = span * arg[1] + arg[2], step * arg[1]
        assert info.raw_per_window == span and info.raw_step == step, desc
        binfo, _ = engine.stages_geometry(engine.FMT_CF32, sr, n, stages, width=W, stride=S, epilogue=engine.EPI_BUCKET2_U8)
        assert binfo.n_windows == (ch.len() - W) // S, desc
        seen.add(shape)
        checked += 1
        zero_first += first_ratio == 0.0 and any(k == "shift" and a != 0 for k, a in stages)
        short_tail += want_done < total
    # the draw must keep reaching what it is for: every fused and routed shape, both refusal codes, 0 Hz first shifts
    # followed by another shift, and failing last windows
    assert set(FUSED) | set(ROUTED) <= seen, sorted(set(FUSED) | set(ROUTED) - seen)
    assert checked > 1500 and refused[ERR_PANIC] > 50 and refused[ERR_UNSUPPORTED] > 50, (checked, refused)
    assert zero_first > 20 and short_tail > 20, (zero_first, short_tail)


@pytest.mark.parametrize("stages,W,code", [
    ([("lowpass", (100_000, 16, 4096)), ("shift", 1_000)], 128, None),               # T1 = 4096: the kernel's largest first stage
    ([("lowpass", (100_000, 16, 4097)), ("shift", 1_000)], 128, ERR_UNSUPPORTED),
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 15, 512))], 512, None),    # n2 = 512 * 15 + 512 = 8192, D2 odd
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 15, 513))], 512, ERR_UNSUPPORTED),
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 14, 1024))], 512, None),   # n2 = 512 * 14 + 1024 = 8192, D2 even
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 14, 1025))], 512, ERR_UNSUPPORTED),
    ([("lowpass", (200_000, 2, 40)), ("shift", 1_000)], 8192, None),                 # no second lowpass: n2 = W = 8192
    ([("lowpass", (200_000, 2, 40)), ("shift", 1_000)], 16384, ERR_UNSUPPORTED),
])
def test_stage_validation_envelope(engine, stages, W, code):
    """the kernel's envelope at its edges: intermediate block n2 <= 8192, first stage T1 <= 4096"""
    n = 1 << 21
    if code is None:
        info, _ = engine.stages_geometry(engine.FMT_CF32, SR, n, stages, width=W)
        assert info.n_windows > 0
        return
    with pytest.raises(engine.QuadrsError) as ei:
        engine.stages_geometry(engine.FMT_CF32, SR, n, stages, width=W)
    assert ei.value.code == code
    with pytest.raises(engine.QuadrsError) as ei:           # plan creation validates first, before any device call
        engine.Plan(engine.FMT_CF32, SR, n, stages=stages, width=W)
    assert ei.value.code == code
