"""The write sink (QD_EPI_CF32_BLOCKS) behind a cascade on the GPU (qd::k_cascade_write) against the oracle's nested read_at blocks.

do_write (src/lib.rs:178-213) reads read_at(b B, B) of the last stage; every nested lowpass truncates against ITS read of that block.
Shift-free chains are bit for bit; with a shift a block may differ only where it reads an ambiguous NCO multiplier component (the NCO
rule, util.explain_check with S = W = B), and every such block is reproduced by replaying the oracle with the other rounding
(util.replay_window, sink="blocks").  A block's bytes depend only on the block: sub-ranges, slabs, chunks and shards reproduce the
whole run."""
import numpy as np
import pytest

from test_gpu_parity import _signal, _to_format
from util import differing_windows, explain_check, replay_window

pytestmark = pytest.mark.gpu

SR = 2_000_000
L1, L2 = (200_000, 4, 40), (30_000, 4, 64)
SHAPES = {
    "LS": [("lowpass", L1), ("shift", 30_000)],
    "SLS": [("shift", 300_000), ("lowpass", L1), ("shift", 30_000)],
    "LL": [("lowpass", L1), ("lowpass", L2)],
    "SLL": [("shift", 300_000), ("lowpass", L1), ("lowpass", L2)],
    "LSL": [("lowpass", L1), ("shift", 15_000), ("lowpass", L2)],
    "SLSL": [("shift", 300_000), ("lowpass", L1), ("shift", 15_000), ("lowpass", L2)],
    "LLS": [("lowpass", L1), ("lowpass", L2), ("shift", -20_000)],
    "SLLS": [("shift", 300_000), ("lowpass", L1), ("lowpass", L2), ("shift", -20_000)],
    "LSLS": [("lowpass", L1), ("shift", 15_000), ("lowpass", L2), ("shift", 3_000)],
    "SLSLS": [("shift", 300_000), ("lowpass", L1), ("shift", 15_000), ("lowpass", L2), ("shift", 3_000)],
}


def _oracle(O, data, fmt, stages, sr=SR):
    ch = O.Chain.from_bytes(data, fmt, sr)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch


def _span_step(stages, B):
    span, D = B, 1
    for kind, arg in reversed(stages):
        if kind == "lowpass":
            span, D = span * arg[1] + arg[2], D * arg[1]
    return span, B * D


def _data(fmt, n, seed=5):
    return _to_format(_signal(np.random.default_rng(seed), n), fmt)


def _plan(engine, fmt, n, stages, B, sr=SR, **kw):
    return engine.Plan(fmt, sr, n, stages=stages, width=B, stride=B, epilogue=engine.EPI_CF32_BLOCKS, **kw)


def _ref_blocks(ch, B, blocks):
    """the oracle's read_at blocks, one row each (the blocks asked for are all full)"""
    rows = []
    for b in blocks:
        got, out = ch.read_at(int(b) * B, B)
        assert got == B, (b, got)
        rows.append(out.reshape(-1))
    return np.stack(rows) if rows else np.zeros((0, 2 * B), np.float32)


def _check_blocks(ch, stages, B, ref, got, sr=SR, first_block=0, what=""):
    """ref / got: one row per block (absolute blocks first_block ...)"""
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(ref.shape[0], -1)
    if not any(k == "shift" for k, _ in stages):
        assert got.tobytes() == ref.tobytes(), f"{what}: blocks {differing_windows(ref, got)[:8]} differ"
        return
    detail = {}
    assert explain_check((stages, B, B, sr), ref, got, first_block, detail) == [], what
    for r in differing_windows(ref, got):
        w = first_block + int(r)
        assert replay_window(ch, w, detail[w], got[r], B, sink="blocks") is not None, f"{what}: block {w} is not reproduced"


def _whole_vs_oracle(engine, oracle, stages, B, fmt=0, sr=SR, seed=5, what=""):
    """a stream of three full blocks plus a ragged tail, run on the host path, against the oracle"""
    span, step = _span_step(stages, B)
    n = span + 2 * step + step // 2 + 3
    data = _data(fmt, n, seed)
    plan = _plan(engine, fmt, n, stages, B, sr)
    assert plan.n_windows == 3 and plan.complete_windows() == 3
    assert plan.kernel_name().startswith(f"qd::k_cascade_write<{fmt}>")
    got = plan.run_host(data)
    assert got.shape == (3 * B, 2)
    ch = _oracle(oracle, data, fmt, stages, sr)
    assert ch.read_at(3 * B, B)[0] < B                     # the ragged tail is the iterator's
    _check_blocks(ch, stages, B, _ref_blocks(ch, B, range(3)), got, sr, what=what or f"{stages} B={B}")
    return plan, data, got, ch


@pytest.mark.parametrize("B", [64, 1024, 4096])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_write_blocks_cf32(engine, oracle, shape, B):
    _whole_vs_oracle(engine, oracle, SHAPES[shape], B, what=f"{shape} B={B}")


@pytest.mark.parametrize("fmt", [1, 2, 3])
@pytest.mark.parametrize("shape", ["LL", "SLSLS", "LS"])
def test_write_blocks_formats(engine, oracle, shape, fmt):
    _whole_vs_oracle(engine, oracle, SHAPES[shape], 1024, fmt=fmt, what=f"{shape} fmt={fmt}")


@pytest.mark.parametrize("stages,B", [
    ([("lowpass", (200_000, 3, 37)), ("lowpass", (30_000, 2, 45))], 256),                     # D1 odd, D2 = 2
    ([("lowpass", (300_000, 2, 29)), ("shift", 10_000), ("lowpass", (40_000, 4, 51))], 1024),  # D1 = 2, D2 = 4
    ([("lowpass", (200_000, 4, 43)), ("lowpass", (20_000, 8, 101)), ("shift", 1_000)], 512),  # D2 a multiple of 8
    ([("lowpass", (150_000, 6, 35)), ("lowpass", (20_000, 6, 77))], 256),                     # D = 6: per-tap pads
    ([("shift", 100_000), ("lowpass", (60_000, 16, 53)), ("lowpass", (5_000, 3, 33))], 128),  # D1 a multiple of 8, D2 odd
    ([("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 32, 400))], 4096),                  # inter block 131 472: far past 8192
    ([("lowpass", (60_000, 16, 4096)), ("shift", 2_000)], 1024),                              # T1 = 4096, no second lowpass
    ([("lowpass", (60_000, 16, 4096)), ("lowpass", (5_000, 2, 99))], 64),                     # T1 = 4096 with one
    ([("lowpass", (400_000, 2, 40)), ("lowpass", (20_000, 3, 8192))], 64),                    # T2 = 8192: sub-blocks of one output
])
def test_write_geometry(engine, oracle, stages, B):
    plan, *_ = _whole_vs_oracle(engine, oracle, stages, B, seed=11)
    assert "k_cascade_write" in plan.kernel_name()


def test_write_truncation_is_real(engine, oracle):
    """the last outputs of a block are truncated against THAT block's reads: they differ from the untruncated continuation"""
    stages, B = SHAPES["LL"], 1024
    _, _, got, ch = _whole_vs_oracle(engine, oracle, stages, B, seed=3)
    got = got.reshape(3, B, 2)
    n, cont = ch.read_at(B - 8, 16)
    assert n == 16
    # outer outputs 1017 ... 1023 read past the block's inter samples (k D2 + c2 + T2 > B D2 + T2), 1016 reads truncated inter samples
    assert (got[0, B - 8:] != cont[:8]).any(axis=1).sum() >= 7


@pytest.mark.parametrize("shape", ["LL", "SLSLS", "LS"])
def test_write_same_bytes_as_whole_run(engine, shape):
    import torch
    stages, B = SHAPES[shape], 1024
    span, step = _span_step(stages, B)
    n = span + 40 * step + 777
    data = _data(0, n, seed=7)
    plan = _plan(engine, 0, n, stages, B)
    nw = plan.n_windows
    assert nw == 41
    whole = plan.run_host(data).reshape(nw, -1)
    raw = np.frombuffer(data, dtype=np.uint8)
    # block sub-ranges from a slab that starts at the range's first sample, and one a sample earlier (an odd slab start)
    for w0, cnt in ((1, 7), (13, 11), (nw - 3, 3), (0, 1)):
        s0, sc = plan.src_range(w0, cnt)
        slab = raw[s0 * 8:(s0 + sc) * 8]
        assert plan.run_host(slab, first_window=w0, n_windows=cnt, src_first=s0).tobytes() == whole[w0:w0 + cnt].tobytes()
        a = s0 - 1 if s0 % 2 == 0 and s0 > 0 else s0
        slab = raw[a * 8:(s0 + sc) * 8]
        assert a % 2 == 1 or s0 == 0
        assert plan.run_host(slab, first_window=w0, n_windows=cnt, src_first=a).tobytes() == whole[w0:w0 + cnt].tobytes()
    # device buffers, whole and a sub-range from an odd device slab, twice on the same buffers
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.empty(nw * B, 2, dtype=torch.float32, device="cuda")
    for _ in range(2):
        out.zero_()
        plan.run_device(src, out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == whole.tobytes()
    s0, sc = plan.src_range(5, 9)
    sub = torch.empty(9 * B, 2, dtype=torch.float32, device="cuda")
    plan.run_device(src[(s0 - 1) * 8:(s0 + sc) * 8], sub, 5, 9, src_first=s0 - 1, src_count=sc + 1)
    torch.cuda.synchronize()
    assert sub.cpu().numpy().tobytes() == whole[5:14].tobytes()
    # the host path in small chunks (whole blocks each)
    small = _plan(engine, 0, n, stages, B, chunk_bytes=1 << 16)
    assert small.run_host(data).tobytes() == whole.tobytes()
    assert small.stats().chunks >= 10
    # pinned source and sink
    pin_in, pin_out = engine.PinnedBuffer(raw.size), engine.PinnedBuffer(whole.nbytes)
    pin_in.array[:] = raw
    assert plan.run_host(pin_in.array, pinned=True, out=pin_out.array).tobytes() == whole.tobytes()
    assert plan.run_host(pin_in.array, pinned=True).tobytes() == whole.tobytes()
    pin_in.close(); pin_out.close()
    # 2 and 3 shards on one device
    for k in (2, 3):
        sh = _plan(engine, 0, n, stages, B, shard_devices=[0] * k)
        assert sh.run_sharded_host(data).tobytes() == whole.tobytes()
    # determinism
    assert plan.run_host(data).tobytes() == whole.tobytes()


def test_write_long_stream(engine, oracle):
    """2^25 device-resident samples (bench.synth_slab): the whole run against sub-ranges, the first, middle and last full blocks
    against the oracle"""
    import torch
    import bench
    stages, B, n = [("shift", 280_000), ("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200))], 4096, 1 << 25
    sr = 21_000_000
    plan = _plan(engine, 0, n, stages, B, sr=sr)
    nw = plan.n_windows
    span, step = _span_step(stages, B)
    assert nw == (n - span) // step + 1 and nw > 200
    src = bench.synth_slab(torch, 0, 0, n, bench.STREAM_SEED, torch.device("cuda"))
    out = torch.empty(nw * B, 2, dtype=torch.float32, device="cuda")
    plan.run_device(src, out)
    torch.cuda.synchronize()
    whole = out.cpu().numpy().reshape(nw, -1)
    for w0, cnt in ((0, 5), (nw // 2 - 2, 17), (nw - 4, 4)):
        s0, sc = plan.src_range(w0, cnt)
        sub = torch.empty(cnt * B, 2, dtype=torch.float32, device="cuda")
        plan.run_device(src.view(torch.uint8).reshape(-1)[s0 * 8:(s0 + sc) * 8], sub, w0, cnt, src_first=s0, src_count=sc)
        torch.cuda.synchronize()
        assert sub.cpu().numpy().tobytes() == whole[w0:w0 + cnt].tobytes(), (w0, cnt)
    blocks = [0, nw // 2, nw - 1]
    lo, cnt = plan.src_range(nw - 1, 1)
    data = src.view(torch.uint8).reshape(-1).cpu().numpy().tobytes()
    ch = _oracle(oracle, data, 0, stages, sr)
    assert ch.read_at(nw * B, B)[0] < B
    ref = _ref_blocks(ch, B, blocks)
    _check_blocks(ch, stages, B, ref, whole[blocks], sr=sr, what="long stream")


def test_write_plan_behaviour(engine, oracle):
    stages, B = SHAPES["SLL"], 1024
    span, step = _span_step(stages, B)
    n = span + 4 * step + 5
    data = _data(0, n, seed=29)
    plan = _plan(engine, 0, n, stages, B)
    fast = _plan(engine, 0, n, stages, B, mode=engine.MODE_FAST)
    whole = plan.run_host(data)
    assert fast.run_host(data).tobytes() == whole.tobytes()           # a cascade runs the exact arithmetic in either mode
    info, done = engine.stages_geometry(engine.FMT_CF32, SR, n, stages, width=B, stride=B, epilogue=engine.EPI_CF32_BLOCKS)
    for f in ("n_windows", "decimated_len", "out_sample_rate", "out_bytes_per_window", "raw_per_window", "raw_step", "ratio"):
        assert getattr(plan.info, f) == getattr(info, f), f
    assert done == plan.complete_windows() == plan.n_windows == 5
    with pytest.raises(engine.QuadrsError) as ei:
        plan.run_host(data, first_window=3, n_windows=3)
    assert ei.value.code == engine._ffi.ERR_SHORT
    with pytest.raises(engine.QuadrsError) as ei:                     # no pre-split device path for cascades
        plan.run_sharded_device([0], [0])
    assert ei.value.code == engine._ffi.ERR_UNSUPPORTED
    name = plan.kernel_name()
    assert name.startswith("qd::k_cascade_write<0>(D1 4, T1 40, D2 4, T2 64, B 1024, K 512"), name
