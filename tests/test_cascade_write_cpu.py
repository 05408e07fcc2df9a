"""CPU tests of the write sink (QD_EPI_CF32_BLOCKS) behind a cascade: qd_stages_geometry's figures for every fused shape against
the oracle's nested read_at blocks (do_write, src/lib.rs:178-213), and the envelope's edges, refused before any device call."""
import numpy as np
import pytest

SR = 1_000_000
ERR_INVALID, ERR_PANIC, ERR_UNSUPPORTED = 1, 2, 5
FUSED = ("LS", "SLS", "LL", "SLL", "LSL", "SLSL", "LLS", "SLLS", "LSLS", "SLSLS")
# stage parameters by position: the first lowpass (D1, T1), the second (D2, T2), and one shift per rate
LP = [(100_000, 4, 40), (10_000, 3, 25)]
SHIFTS = [40_000, -3_000, 700]


def _stages(shape):
    out, n_lp = [], 0
    for c in shape:
        if c == "S":
            out.append(("shift", SHIFTS[n_lp]))
        else:
            out.append(("lowpass", LP[n_lp]))
            n_lp += 1
    return out


def _oracle_chain(O, n, stages, sr=SR):
    ch = O.Chain.from_bytes(np.zeros(n * 8, dtype=np.uint8), O.FMT_CF32, sr)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch


def _full_blocks(ch, B):
    """leading b whose read_at(b B, B) returns B samples: do_write's full blocks"""
    b = 0
    while ch.read_at(b * B, B)[0] == B:
        b += 1
    return b


def _span(stages, B):
    """source samples of one block: the innermost read of the nested stages"""
    span = B
    for kind, arg in reversed(stages):
        if kind == "lowpass":
            span = span * arg[1] + arg[2]
    return span


def _first_ratio(O, stages, sr=SR):
    rate = sr
    for kind, arg in stages:
        if kind == "shift":
            return O.shift_ratio(arg, rate)
        rate //= arg[1]
    return 0.0


@pytest.mark.parametrize("B", [64, 4096])
@pytest.mark.parametrize("shape", FUSED)
def test_write_geometry_matches_oracle(engine, oracle, shape, B):
    stages = _stages(shape)
    D = int(np.prod([a[1] for k, a in stages if k == "lowpass"]))
    span, step = _span(stages, B), B * D
    rng = np.random.default_rng(B + len(shape) * 7 + sum(map(ord, shape)))
    # lengths around the block boundaries: one short of a block's span, exactly it, and around later blocks' ends
    lengths = {span - 1, span, span + 1, span + step - 1, span + step, span + 2 * step + int(rng.integers(0, step)),
               span + 3 * step - 1, span + 3 * step + int(rng.integers(0, step))}
    lengths |= {int(x) for x in rng.integers(span - step, span + 4 * step, 3)}
    for n in sorted(lengths):
        ch = _oracle_chain(oracle, n, stages)
        info, done = engine.stages_geometry(engine.FMT_CF32, SR, n, stages, width=B, stride=B, epilogue=engine.EPI_CF32_BLOCKS)
        full = _full_blocks(ch, B)
        assert info.n_windows == full, (n, info.n_windows, full)
        assert done == info.n_windows
        assert ch.read_at(full * B, B)[0] < B               # the first block past them is short
        assert info.out_bytes_per_window == 8 * B
        assert info.raw_per_window == span and info.raw_step == step
        assert info.decimated_len == ch.len() and info.out_sample_rate == ch.sample_rate()
        assert info.ratio == _first_ratio(oracle, stages)


def test_write_blocks_ignore_stride(engine):
    """blocks step by B whatever the sink's stride (the one-stage write sink does the same)"""
    stages = _stages("SLL")
    n = 1 << 20
    a, ca = engine.stages_geometry(engine.FMT_CF32, SR, n, stages, width=256, stride=256, epilogue=engine.EPI_CF32_BLOCKS)
    b, cb = engine.stages_geometry(engine.FMT_CF32, SR, n, stages, width=256, stride=7, epilogue=engine.EPI_CF32_BLOCKS)
    assert (a.n_windows, a.raw_step, a.raw_per_window, ca) == (b.n_windows, b.raw_step, b.raw_per_window, cb)


def _refused(engine, stages, B, code, n=1 << 21, stride=None):
    kw = dict(width=B, stride=B if stride is None else stride, epilogue=engine.EPI_CF32_BLOCKS)
    with pytest.raises(engine.QuadrsError) as ei:
        engine.stages_geometry(engine.FMT_CF32, SR, n, stages, **kw)
    assert ei.value.code == code, str(ei.value)
    with pytest.raises(engine.QuadrsError) as ei:           # plan creation validates first, before any device call
        engine.Plan(engine.FMT_CF32, SR, n, stages=stages, **kw)
    assert ei.value.code == code, str(ei.value)


@pytest.mark.parametrize("stages,B,code", [
    ([("lowpass", (100_000, 16, 4096)), ("shift", 1_000)], 4096, None),             # T1 = 4096: the kernel's largest first stage
    ([("lowpass", (100_000, 16, 4097)), ("shift", 1_000)], 4096, ERR_UNSUPPORTED),
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 32, 400))], 4096, None),   # inter block 4096 * 32 + 400: far past 8192
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 2, 4096))], 4096, None),   # T2 = 4096
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 3, 8192))], 64, None),     # T2 = 8192: one sub-block of one output
    ([("lowpass", (200_000, 2, 40)), ("lowpass", (10_000, 3, 8193))], 64, ERR_UNSUPPORTED),
    ([("lowpass", (200_000, 2, 40)), ("shift", 1_000)], 1 << 20, None),              # the one-stage write sink's largest block
    ([("lowpass", (200_000, 2, 40)), ("shift", 1_000)], 1 << 21, ERR_UNSUPPORTED),   # ... and past it (width too large)
    ([("lowpass", (200_000, 2, 40)), ("shift", 1_000)], 100, ERR_PANIC),             # not a power of two (Radix4's contract)
    ([("lowpass", (200_000, 64, 40)), ("lowpass", (1_000, 64, 40))], 1 << 20, ERR_UNSUPPORTED),   # a block's span past 2^31
])
def test_write_envelope(engine, stages, B, code):
    n = 1 << 21
    if code is None:
        info, done = engine.stages_geometry(engine.FMT_CF32, SR, n, stages, width=B, stride=B, epilogue=engine.EPI_CF32_BLOCKS)
        assert info.out_bytes_per_window == 8 * B and done == info.n_windows
        return
    _refused(engine, stages, B, code, n)


def test_write_stride_zero_is_invalid(engine):
    _refused(engine, _stages("LL"), 64, ERR_INVALID, stride=0)


@pytest.mark.parametrize("stages,geo_code,plan_code", [
    ([], ERR_UNSUPPORTED, ERR_INVALID),                      # no lowpass: the write sink needs one
    ([("shift", 1_000)], ERR_UNSUPPORTED, ERR_INVALID),
    ([("lowpass", (100_000, 4, 40))] * 3, ERR_UNSUPPORTED, ERR_UNSUPPORTED),                        # three lowpasses
    ([("lowpass", (100_000, 4, 40)), ("shift", 10), ("shift", 20)], ERR_UNSUPPORTED, ERR_UNSUPPORTED),   # two shifts in a row
    ([("shift", 10), ("shift", 20)], ERR_UNSUPPORTED, ERR_UNSUPPORTED),
    ([("lowpass", (100_000, 4, 40)), ("lowpass", (10_000, 0, 40))], ERR_PANIC, ERR_PANIC),          # decimate 0
])
def test_write_unfused_lists_keep_their_codes(engine, stages, geo_code, plan_code):
    n, B = 1 << 20, 4096
    kw = dict(width=B, stride=B, epilogue=engine.EPI_CF32_BLOCKS)
    with pytest.raises(engine.QuadrsError) as ei:
        engine.stages_geometry(engine.FMT_CF32, SR, n, stages, **kw)
    assert ei.value.code == geo_code
    with pytest.raises(engine.QuadrsError) as ei:
        engine.Plan(engine.FMT_CF32, SR, n, stages=stages, **kw)
    assert ei.value.code == plan_code


@pytest.mark.parametrize("stages", [[("lowpass", (100_000, 4, 40))], [("shift", 1_000), ("lowpass", (100_000, 4, 40))]])
def test_write_routed_lists_stay_one_stage(engine, stages):
    """[shift] lowpass is the one-stage plan's write sink: qd_stages_geometry keeps pointing at qd_plan_get_info"""
    with pytest.raises(engine.QuadrsError) as ei:
        engine.stages_geometry(engine.FMT_CF32, SR, 1 << 20, stages, width=4096, stride=4096, epilogue=engine.EPI_CF32_BLOCKS)
    assert ei.value.code == ERR_UNSUPPORTED
