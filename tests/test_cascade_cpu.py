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
