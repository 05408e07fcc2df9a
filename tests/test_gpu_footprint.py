"""Footprint tests (-m gpu): which memory a run touches.  Windows [w0, w0 + n) may read source samples src_range(w0, n) and
nothing else, and write n * out_bytes_per_window bytes and nothing else (include/quadrs_hip.h; DESIGN section 8 partitions a
stream over GPUs on exactly that).  Every run here gets its slab and its output INSIDE one allocation each, between frames the
test owns (util.framed / util.framed_out): an over-read or over-write lands in the test's own memory, never outside it.

Each case runs once per poison pattern.  cf32 frames hold quiet NaNs (0x7FC00000: survives a multiplication by a zero tap) and
then 0x7F7FFFFF; cs8 / cu8 / cs16 frames hold 0x80 and then 0x7F bytes — the integer formats have no NaN, so there an influence
of the frames shows ONLY as a difference between the two runs.  util.footprint_violations then asks: both fills give the same
payload bytes; the payload obeys the chain's rule against the ORACLE on the true stream (bit for bit without a shift, the NCO
rule with one, codes_edge_ok / bucket_digits_ok for the quantising sinks); no output element kept its 0xA5 pre-fill where the
oracle says otherwise; both output guards still hold 0xA5; device and pinned source buffers are byte for byte what was uploaded.
Frame sizes are conditions (util.src_frame_bytes / out_guard_bytes), not measurements.  Reads whose values are discarded
cannot be seen by this method.  The positive controls put a NaN on the first and the last sample INSIDE the slab and see it in
the first and the last window: the frames sit flush against samples the kernels consume.

Every case asserts the kernel family it is named for; plans that follow the harness environment (no explicit policy) are
skipped under QD_NO_FIXED=1 like the family tests of test_gpu_robustness.py."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_parity import _signal, _to_format
from util import (FMT_BYTES, POISON_WORDS, FootprintRun, Framed, complex_ulp_err, footprint_reference, footprint_violations, framed,
                  framed_out, out_guard_bytes, poison, src_frame_bytes)

pytestmark = pytest.mark.gpu

SR = 21_000_000
NAN_WORD = 0x7FC00000


# ------------------------------------------------------------------ cases

class Case:
    """one chain + plan options + the family its plan must come out as"""

    def __init__(self, name, fmt, n, W, S=None, shift=None, lp=None, stages=None, sr=SR, epi=0, rng=None, family=None, follows_env=False,
                 **plan_kw):
        self.name, self.fmt, self.n, self.W, self.S, self.sr, self.epi, self.rng = name, fmt, n, W, W if S is None else S, sr, epi, rng
        self.shift, self.lp, self.stages_arg, self.family, self.follows_env, self.plan_kw = shift, lp, stages, family, follows_env, plan_kw
        self.stages = list(stages) if stages is not None else \
            ([("shift", shift)] if shift is not None else []) + ([("lowpass", tuple(lp))] if lp is not None else [])

    def __repr__(self):
        return self.name

    def with_sink(self, epi, rng=None):
        c = Case(f"{self.name}-epi{epi}", self.fmt, self.n, self.W, self.S, self.shift, self.lp, self.stages_arg, self.sr, epi, rng,
                 self.family, self.follows_env, **self.plan_kw)
        return c

    def longer(self, k):
        return Case(f"{self.name}-x{k}", self.fmt, self.n * k, self.W, self.S, self.shift, self.lp, self.stages_arg, self.sr, self.epi, self.rng,
                    self.family, self.follows_env, **self.plan_kw)

    def data(self):
        return np.frombuffer(_to_format(_signal(np.random.default_rng(self.n + self.W), self.n), self.fmt), dtype=np.uint8)

    def plan(self, engine, **kw):
        if self.follows_env and os.environ.get("QD_NO_FIXED"):
            pytest.skip("QD_NO_FIXED=1 runs the generic kernels only")
        args = dict(width=self.W, stride=self.S, epilogue=self.epi, rng=self.rng)
        if self.stages_arg is not None:
            args["stages"] = self.stages_arg
        else:
            args.update(shift_hz=self.shift, lowpass=self.lp)
        p = engine.Plan(self.fmt, self.sr, self.n, **args, **self.plan_kw, **kw)
        name = p.kernel_name()
        if self.family is not None:
            assert self.family(p, name), (self.name, name, int(p.info.kernel_kind), int(p.info.kernel_flags))
        return p

    def oracle_chain(self, oracle, data):
        ch = oracle.Chain.from_bytes(data, self.fmt, self.sr)
        for kind, arg in self.stages:
            ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
        return ch


def builtin(kernel):
    return lambda p, name: p.info.kernel_kind == 1 and name.startswith(f"qd::{kernel}<") and name.endswith("built-in")


def plan_time(kernel, flags=0, no_flags=0):
    return lambda p, name: (p.info.kernel_kind == 2 and name.startswith(f"qd::{kernel}<") and name.endswith("plan-time build")
                            and (p.info.kernel_flags & flags) == flags and not (p.info.kernel_flags & no_flags))


def generic(p, name):
    return p.info.kernel_kind == 0 and "DynGeo" in name and name.endswith("generic")


def named(part, then=""):
    return lambda p, name: part in name and then in name


FSK = dict(shift=280000, lp=(200_000, 32, 400), W=64, S=16)
CFG2 = dict(shift=280000, lp=(2_000_000, 16, 40), W=128, S=128)
CFG3P = dict(shift=280000, lp=(200_000, 32, 200), W=128, S=128)
CFG4 = dict(shift=None, lp=(5_000_000, 8, 512), W=1024, S=1024, sr=100_000_000)
L1, L2 = ("lowpass", (200_000, 4, 40)), ("lowpass", (30_000, 4, 64))
CASC = {"LL": [L1, L2], "LS": [L1, ("shift", 30_000)],
        "SLSLS": [("shift", 300_000), L1, ("shift", 15_000), L2, ("shift", 3_000)]}

# row 1: the built-in kernels of cfg2, cfg3', cfg4; two-window and half-window tiles through a tile hint
ROW1 = [
    Case("cfg2", 0, 300_000, family=builtin("k_chain"), follows_env=True, **CFG2),
    Case("cfg3p", 0, 400_000, family=builtin("k_chain"), follows_env=True, **CFG3P),
    Case("cfg4", 0, 150_000, family=builtin("k_chain"), follows_env=True, **CFG4),
    Case("cfg2-two-window-tiles", 0, 300_000, family=plan_time("k_chain", 264), follows_env=True, tile_hint=[2, 256, 1, 8, 4, 1, 1 | (264 << 8), 0], **CFG2),
    Case("cfg4-half-window-tiles", 0, 150_000, family=plan_time("k_chain", 8192), follows_env=True, tile_hint=[1, 512, 2, 4, 4, 2, 2 | (8392 << 8), 0], **CFG4),
]
# row 2: the three-stage kernel and its streaming form; long streams give every workgroup a run of many steps and switch the
# tile queue on (more tiles than workgroups), short ones leave it off
BIG = (1 << 25) - 40_000
ROW2 = [
    Case("pipe3s-cs8-builtin-long", 1, BIG, family=lambda p, n: p.info.kernel_flags == 164128 and n.startswith("qd::k_chain_pipe3s<"), follows_env=True, **FSK),
    Case("pipe3s-cf32-long", 0, BIG, family=plan_time("k_chain_pipe3s", 32768 | 131072), follows_env=True,
         tile_hint=[14, 512, 1, 8, 4, 2, 1 | (164128 << 8), 0], **FSK),
    Case("pipe3s-cs8-short", 1, 300_000, family=lambda p, n: p.info.kernel_flags == 164128 and n.startswith("qd::k_chain_pipe3s<"), follows_env=True, **FSK),
    Case("pipe3-cs8-tile-queue", 1, BIG, family=plan_time("k_chain_pipe3", 32768, 131072), follows_env=True,
         tile_hint=[12, 512, 1, 8, 4, 2, 1 | (32800 << 8), 0], **FSK),
    Case("pipe3-cf32-no-queue", 0, 300_000, family=plan_time("k_chain_pipe3", 32768, 131072), follows_env=True,
         tile_hint=[12, 512, 1, 8, 4, 2, 1 | (33056 << 8), 0], **FSK),
]
# row 3: the generic DynGeo kernels: all four formats, odd D, stride 1, T/2 < D, decimate 1
GEN = dict(family=generic, kernel_policy=1)
ROW3 = [
    Case("generic-cf32-odd-D-stride-1", 0, 50_000, 4, 1, 5_000, (300_000, 3, 10), **GEN),
    Case("generic-cs8", 1, 200_000, **FSK, **GEN),
    Case("generic-cu8", 2, 100_000, 32, 8, -500_000, (1_000_000, 8, 40), **GEN),
    Case("generic-cs16-D10", 3, 100_000, 16, 5, 123_456, (700_000, 10, 24), **GEN),
    Case("generic-decimate-1", 0, 30_000, 256, 256, 280000, (2_000_000, 1, 6), **GEN),
    Case("generic-half-T-below-D", 0, 70_000, 8, 2, 280000, (2_000_000, 64, 30), **GEN),
]
# row 4: plan-time specialised builds; the write sink's streaming kernel (flag 262144) and the generic write sink
ROW4 = [
    Case("specialised-D12", 0, 300_000, 256, 256, -1_250_000, (1_500_000, 12, 48), family=plan_time("k_chain"), kernel_policy=2),
    Case("specialised-cs16-overlap", 3, 300_000, 64, 32, 99_000, (300_000, 16, 100), family=lambda p, n: p.info.kernel_kind == 2, kernel_policy=2),
    Case("write-sink-streaming", 0, 9 * 4096 * 8 + 40 + 4096 * 4, 4096, 4096, 280000, (500_000, 8, 40), epi=3,
         family=lambda p, n: p.info.kernel_kind == 2 and p.info.kernel_flags & 262144, kernel_policy=2),
    Case("write-sink-generic", 0, 40 * 64 * 3 + 10 + 96, 64, 64, None, (500_000, 3, 10), epi=3, family=lambda p, n: p.info.kernel_kind == 0, kernel_policy=1),
]
# row 5: the wave-local family (no lowpass): k_spark2, k_spark, k_spark0, the interleaved-phase launches
NF = 24 * 1024 + 5
ROW5 = [
    Case("spark2-cf32-shift", 0, NF + 384, 128, 128, 280000, family=plan_time("k_spark2", 524288 | 1048576), kernel_policy=2),
    Case("spark-cs8", 1, NF + 192, 64, 64, family=plan_time("k_spark", 524288, 1048576 | 2097152), kernel_policy=2),
    Case("spark-builtin-cs16-shift", 3, NF + 96, 32, 32, 280000, family=builtin("k_spark"), kernel_policy=3),
    Case("spark0-cf32-W4-S2", 0, NF + 12, 4, 2, family=plan_time("k_spark0", 524288 | 2097152), kernel_policy=2),
    Case("phases-cf32-W64-S16", 0, NF + 192, 64, 16, family=plan_time("k_spark", 524288, 1048576 | 2097152), kernel_policy=2),
    Case("phases-cf32-W64-S16-shift", 0, NF + 192, 64, 16, 280000, family=plan_time("k_spark", 524288, 1048576 | 2097152), kernel_policy=2),
    Case("phases-cs16-W16-S4-shift", 3, NF + 48, 16, 4, -1_234_567, family=plan_time("k_spark", 524288, 1048576 | 2097152), kernel_policy=2),
    Case("phases-cs8-W8-S4", 1, NF + 24, 8, 4, family=plan_time("k_spark0", 524288 | 2097152), kernel_policy=2),
]
# row 7: two-stage plans (a window larger than one workgroup's LDS)
TWO = named("two stages:")
ROW7 = [
    Case("two-stage-cf32-W1024-D32", 0, 7 * 1024 * 32 + 200 + 3 * 32 + 5, 1024, 1024, 280000, (150_000, 32, 200), family=TWO),
    Case("two-stage-cs8-W256-D128", 1, 7 * 256 * 128 + 400 + 3 * 128 + 5, 256, 256, 280000, (150_000, 128, 400), family=TWO),
]
# row 8: cascades
ROW8 = [Case(f"cascade-{k}", 0, 200_000, 128, 32, stages=CASC[k], sr=2_000_000, family=named("qd::k_cascade<0>")) for k in ("LL", "LS", "SLSLS")] + \
       [Case("cascade-LL-cs8", 1, 150_000, 64, 16, stages=CASC["LL"], sr=2_000_000, family=named("qd::k_cascade<1>"))] + \
       [Case(f"cascade-write-{k}", 0, 9 * 1024 * 16 + 5000, 1024, 1024, stages=CASC[k], sr=2_000_000, epi=3, family=named("qd::k_cascade_write<0>"))
        for k in ("LL", "LS", "SLSLS")] + \
       [Case("cascade-write-LL-cs8", 1, 9 * 1024 * 16 + 5000, 1024, 1024, stages=CASC["LL"], sr=2_000_000, epi=3, family=named("qd::k_cascade_write<1>"))]
# the shape of each crossed row that goes through every run path
CROSS = [ROW1[0], ROW3[2], ROW5[5], ROW8[2]]
CROSS_SHARD_DEVICE = [ROW1[0], ROW1[1], ROW5[4], ROW5[5]]


# ------------------------------------------------------------------ the framed run

def _ranges(p, nw):
    """the whole stream (poison flush against sample 0 and behind the last sample: the tail-truncation reads), an interior
    sub-range that starts and ends off tile boundaries, and the last windows only"""
    G = max(int(p.info.tile_windows), 1)
    out = [(0, nw)]
    w0 = min(G + 1 if G > 1 else 1, nw - 1)
    cnt = max(1, min(nw - w0 - 1, 3 * G + (2 if G > 1 else 1)))
    if (w0 + cnt) % G == 0 and G > 1 and cnt > 1:
        cnt -= 1
    out.append((w0, cnt))
    out.append((nw - min(nw, 3), min(nw, 3)))
    return out


def _one_run(engine, p, case, path, data, w0, n, which, lead=0, twice=False):
    """windows [w0, w0 + n) of `data` (the true stream) from a framed slab of exactly src_range(w0, n) (+ `lead` leading samples,
    declared through src_first) into a framed output; returns the FootprintRun"""
    bps = FMT_BYTES[case.fmt]
    first, count = p.src_range(w0, n)
    first, count = first - lead, count + lead
    fb, gb = src_frame_bytes(p.info, case.fmt), out_guard_bytes(p.info)
    assert fb >= 1 << 20 and gb >= 64 << 10
    kind = {"device": "device", "pinned": "pinned"}.get(path, "host")
    src = framed(kind, case.fmt, which, fb, data[first * bps:(first + count) * bps], fb, engine)
    out = framed_out(kind, gb, n * int(p.info.out_bytes_per_window), engine)
    assert src.body.numel() == count * bps if kind == "device" else src.body.size == count * bps
    for _ in range(2 if twice else 1):
        if path == "device":
            p.run_device(src.body, out.body, w0, n, src_first=first, src_count=count)
        else:
            p.run_host(src.body, w0, n, src_first=first, pinned=(path == "pinned"), out=out.body)
    run = FootprintRun(out, src)
    src.close(); out.close()
    return run


def _check(engine, p, case, path, data, expect, w0, n, **kw):
    runs = [_one_run(engine, p, case, path, data, w0, n, which, **kw) for which in range(len(POISON_WORDS))]
    ref, rule, unit = expect(w0, n)
    bad = footprint_violations(runs, ref, rule, unit)
    assert not bad, (case.name, path, w0, n, kw, bad)


def _expect(case, oracle, data, nw):
    return footprint_reference(case.oracle_chain(oracle, data), case.stages, case.sr, case.W, case.S, case.epi, case.rng, nw)


def _usable_windows(p):
    return min(int(p.n_windows), int(p.complete_windows()))


def _three_ranges(engine, oracle, case, path="device", twice=False, **plan_kw):
    p = case.plan(engine, **plan_kw)
    data = case.data()
    nw = _usable_windows(p)
    assert nw >= 5, (case.name, nw)
    expect = _expect(case, oracle, data, nw)
    for w0, n in _ranges(p, nw):
        _check(engine, p, case, path, data, expect, w0, n, twice=twice)
    p.close()


@pytest.mark.parametrize("case", ROW1 + ROW3 + ROW4 + ROW5 + ROW8, ids=repr)
def test_device_runs_stay_inside_their_slab_and_windows(engine, oracle, case):
    """rows 1, 3, 4, 5, 8 on the device path: whole stream, an interior sub-range off the tile grid, the last windows"""
    _three_ranges(engine, oracle, case)


@pytest.mark.parametrize("case", ROW2, ids=repr)
def test_three_stage_and_streaming_kernels(engine, oracle, case):
    """row 2: k_chain_pipe3 / k_chain_pipe3s, runs of many steps per workgroup and the tile queue on the long streams"""
    _three_ranges(engine, oracle, case)


@pytest.mark.parametrize("case", ROW7, ids=repr)
def test_two_stage_plans(engine, oracle, case):
    """row 7: the device path twice per run (the carrier between the stages is reused), then the host path"""
    _three_ranges(engine, oracle, case, twice=True)
    _three_ranges(engine, oracle, case, path="host")


def _sink_range(oracle, case, data):
    norms, _ = case.oracle_chain(oracle, data).spark_fft(case.W, case.S, max_windows=400, want_codes=False)
    return float(np.percentile(norms, 20)), float(np.percentile(norms, 99))


@pytest.mark.parametrize("case,epi", [(ROW1[0], 1), (ROW1[0], 2), (ROW5[4], 1), (ROW5[1], 2), (ROW8[0], 1), (ROW8[0], 2)], ids=repr)
def test_glyph_and_bucket_sinks(engine, oracle, case, epi):
    """row 9: one-byte outputs behind vector stores: the output guards matter most here"""
    rng = _sink_range(oracle, case, case.data()) if epi == 1 else None
    _three_ranges(engine, oracle, case.with_sink(epi, rng))


# ------------------------------------------------------------------ row 6: the per-sample kernel

def test_per_sample_kernel_on_odd_and_ragged_device_slabs(engine, oracle):
    """A device slab that starts on an odd sample (one extra leading sample, declared through src_first) sends every window to
    the per-sample kernel; a slab that ends inside a load vector sends the last windows there."""
    case = Case("fsk-wide-tiles", 0, 400_000, family=None, **FSK)
    p = case.plan(engine)
    if not os.environ.get("QD_NO_FIXED"):
        assert p.info.threads != 256
    data = case.data()
    expect = _expect(case, oracle, data, p.n_windows)
    first, _ = p.src_range(11, 50)
    assert (first - 1) % 2 == 1
    _check(engine, p, case, "device", data, expect, 11, 50, lead=1)
    _check(engine, p, case, "device", data, expect, 0, 200)
    _check(engine, p, case, "device", data, expect, p.n_windows - 37, 37, lead=1)
    # slabs whose sample count is odd: the last load vector straddles the slab's end
    for c in (Case("ragged-generic", 0, 50_000, 4, 1, 5_000, (300_000, 3, 10), family=generic, kernel_policy=1),
              Case("ragged-spark-S7", 0, 20_000, 64, 7, 280000, family=None, kernel_policy=2),
              Case("ragged-cs8-S3", 1, 20_000, 16, 3, None, family=None, kernel_policy=2)):
        q = c.plan(engine)
        d = c.data()
        ex = _expect(c, oracle, d, q.n_windows)
        spl = {0: 2, 1: 4}[c.fmt]
        for w0, n in ((0, 100), (33, 58), (q.n_windows - 8, 8)):
            a, cnt = q.src_range(w0, n)
            if cnt % spl == 0:
                n -= 1
                a, cnt = q.src_range(w0, n)
            assert cnt % spl != 0, (c.name, w0, n, cnt)
            _check(engine, q, c, "device", d, ex, w0, n)
            if a > 0 and a % spl == 0:                   # ... and with an odd start on top (other ranges start off the vector grid anyway)
                _check(engine, q, c, "device", d, ex, w0, n, lead=1)
        q.close()


# ------------------------------------------------------------------ run paths

@pytest.mark.parametrize("case", CROSS, ids=repr)
@pytest.mark.parametrize("path", ["host", "pinned", "chunked"])
def test_host_paths(engine, oracle, case, path):
    """run_host from pageable memory, from pinned memory in and out (the slab at an interior offset of a larger PinnedBuffer), and
    with 64 KiB chunks so that the range crosses many chunk seams"""
    if path != "chunked":
        return _three_ranges(engine, oracle, case, path=path)
    case = case.longer(8)
    _three_ranges(engine, oracle, case, path="host", chunk_bytes=1 << 16)
    p = case.plan(engine, chunk_bytes=1 << 16)
    p.run_host(case.data())
    assert p.stats().chunks > 8, p.stats().chunks
    p.close()


@pytest.mark.parametrize("case", CROSS, ids=repr)
def test_sharded_host_run(engine, oracle, case):
    """qd_plan_run_sharded over three shards on device 0: the whole stream framed, the whole output framed"""
    p = case.plan(engine, shard_devices=[0, 0, 0])
    data = case.data()
    nw = int(p.n_windows)
    assert _usable_windows(p) == nw
    ref, rule, unit = _expect(case, oracle, data, nw)(0, nw)
    fb, gb = src_frame_bytes(p.info, case.fmt), out_guard_bytes(p.info)
    runs = []
    for which in range(len(POISON_WORDS)):
        src = framed("host", case.fmt, which, fb, data, fb)
        out = framed_out("host", gb, nw * int(p.info.out_bytes_per_window))
        p.run_sharded_host(src.body, out=out.body)
        runs.append(FootprintRun(out, src))
    bad = footprint_violations(runs, ref, rule, unit)
    assert not bad, (case.name, bad)
    p.close()


def _sharded_device(engine, p, case, data, n_shards, which):
    """every shard's slab is its OWN framed buffer: [frame | owned samples | halo room, poisoned | frame]; every shard's output
    its own framed buffer.  Returns (shard infos, FootprintRuns of the outputs, complaints about the slabs)."""
    import torch
    bps = FMT_BYTES[case.fmt]
    infos = [p.shard_info(g) for g in range(n_shards)]
    fb, gb = src_frame_bytes(p.info, case.fmt), out_guard_bytes(p.info)
    slabs, outs = [], []
    for si in infos:
        own = data[si.own_first * bps:(si.own_first + si.own_count) * bps]
        room = _round4(si.halo * bps)
        slabs.append(Framed("device", poison(case.fmt, fb, which), own, poison(case.fmt, room + fb, which)))
        outs.append(framed_out("device", gb, max(int(si.w1 - si.w0), 1) * int(p.info.out_bytes_per_window)))
    torch.cuda.synchronize()
    p.run_sharded_device([s.body.data_ptr() for s in slabs], [o.body.data_ptr() for o in outs], sync=True)
    bad = []
    for g, (si, s) in enumerate(zip(infos, slabs)):
        now, was = s.snapshot(), s.uploaded
        end = s.hi + si.halo * bps
        if not np.array_equal(now[:s.hi], was[:s.hi]):
            bad.append(f"shard {g}: the front frame or the owned samples changed")
        if not np.array_equal(now[end:], was[end:]):
            bad.append(f"shard {g}: bytes behind slab + halo changed")
        if si.halo and not np.array_equal(now[s.hi:end], data[(si.own_first + si.own_count) * bps:(si.own_first + si.own_count + si.halo) * bps]):
            bad.append(f"shard {g}: the halo is not the next shard's first samples")
    return infos, [FootprintRun(o) for o in outs], bad


def _round4(x):
    return (int(x) + 3) // 4 * 4


@pytest.mark.parametrize("case", CROSS_SHARD_DEVICE, ids=repr)
@pytest.mark.parametrize("n_shards", [2, 4])
def test_sharded_device_run(engine, oracle, case, n_shards):
    """qd_plan_run_sharded_device on device 0: a shard's slab is all the memory it may read: what it owns and the halo fetched
    behind it.  Outputs obey the rule, the bytes behind slab + halo are intact, the owned samples unchanged."""
    p = case.plan(engine, shard_devices=[0] * n_shards, chunk_bytes=1 << 20)
    data = case.data()
    nw = int(p.n_windows)
    expect = _expect(case, oracle, data, nw)
    per_fill = []
    for which in range(len(POISON_WORDS)):
        infos, runs, bad = _sharded_device(engine, p, case, data, n_shards, which)
        assert not bad, (case.name, which, bad)
        per_fill.append(runs)
    assert infos[0].w0 == 0 and infos[-1].w1 == nw
    obw = int(p.info.out_bytes_per_window)
    for g, si in enumerate(infos):
        n = int(si.w1 - si.w0)
        if n == 0:
            continue
        runs = [per_fill[k][g] for k in range(len(POISON_WORDS))]
        assert runs[0].payload.size == n * obw
        ref, rule, unit = expect(int(si.w0), n)
        bad = footprint_violations(runs, ref, rule, unit)
        assert not bad, (case.name, g, bad)
    p.close()


# ------------------------------------------------------------------ positive controls

def _nan_at(data, sample):
    d = data.copy()
    d.view("<u4")[2 * sample:2 * sample + 2] = NAN_WORD
    return d


@pytest.mark.parametrize("path", ["device", "host", "pinned", "chunked"])
def test_positive_control_edge_samples_reach_edge_windows(engine, path):
    """A NaN on the LAST sample inside the slab shows in the last window, one on the FIRST sample in the first window (cf32,
    overlapping windows without a lowpass: every sample of a window is consumed).  Behind a lowpass the first T - T/2 samples
    of a window feed no output (src/filter.rs:68-83 keeps outputs from the convolution's centre on), so there the first CONSUMED
    sample stands in for the first one."""
    for case, skip in ((ROW5[4], 0), (ROW1[0], 20)):
        p = case.plan(engine, **(dict(chunk_bytes=1 << 16) if path == "chunked" else {}))
        data = case.data()
        run_path = "host" if path == "chunked" else path
        W = case.W
        for w0, n in _ranges(p, _usable_windows(p))[:2]:
            first, count = p.src_range(w0, n)
            clean = _one_run(engine, p, case, run_path, data, w0, n, 0).payload.view(np.float32).reshape(n, W)
            assert not np.isnan(clean).any()
            last = _one_run(engine, p, case, run_path, _nan_at(data, first + count - 1), w0, n, 0).payload.view(np.float32).reshape(n, W)
            assert np.isnan(last[-1]).all() and (n == 1 or not np.isnan(last[0]).any()), (case.name, path, w0, n)
            head = _one_run(engine, p, case, run_path, _nan_at(data, first + skip), w0, n, 0).payload.view(np.float32).reshape(n, W)
            assert np.isnan(head[0]).all() and (n == 1 or not np.isnan(head[-1]).any()), (case.name, path, w0, n)
        p.close()


def test_positive_control_sharded_runs(engine):
    """the same through qd_plan_run_sharded (whole stream) and qd_plan_run_sharded_device (per-shard slabs)"""
    case = ROW5[4]
    data = case.data()
    p = case.plan(engine, shard_devices=[0, 0, 0])
    nw, W, S = int(p.n_windows), case.W, case.S
    last_sample = (nw - 1) * S + W - 1
    for sample, row in ((0, 0), (last_sample, nw - 1)):
        got = p.run_sharded_host(_nan_at(data, sample)).reshape(nw, W)
        assert np.isnan(got[row]).all() and not np.isnan(got[nw // 2]).any()
    p.close()
    p = case.plan(engine, shard_devices=[0, 0], chunk_bytes=1 << 20)
    for sample, g, row in ((0, 0, 0), (last_sample, 1, -1)):
        infos, runs, bad = _sharded_device(engine, p, case, _nan_at(data, sample), 2, 0)
        rows = runs[g].payload.view(np.float32).reshape(-1, W)
        assert np.isnan(rows[row]).all() and not np.isnan(runs[1 - g].payload.view(np.float32)).any()
    p.close()


# ------------------------------------------------------------------ stale workspaces

@pytest.mark.parametrize("case", [ROW1[0], ROW5[4], ROW7[0], ROW8[2]], ids=repr)
def test_stale_workspaces_do_not_leak(engine, oracle, case):
    """A whole stream MADE of NaN goes through the plan first (host path: the staging ring, the carrier and every intermediate
    buffer then hold NaN), then a short interior sub-range of the true stream runs on the same plan."""
    p = case.plan(engine)
    data = case.data()
    nw = _usable_windows(p)
    expect = _expect(case, oracle, data, nw)
    w0, n = _ranges(p, nw)[1]
    nan_stream = poison(0, data.size, 0)
    out = p.run_host(nan_stream)
    assert np.isnan(out).all()
    _check(engine, p, case, "host", data, expect, w0, n)
    if case is ROW7[0]:
        import torch
        src = torch.from_numpy(nan_stream.copy()).cuda()
        sink = torch.empty(p.n_windows, case.W, dtype=torch.float32, device="cuda")
        p.run_device(src, sink)
        torch.cuda.synchronize()
        assert torch.isnan(sink).all()
        _check(engine, p, case, "device", data, expect, w0, n)
    p.close()


# ------------------------------------------------------------------ row 10: fine-grained calls on device memory

def _fine(engine, fmt_in, inputs, out_bytes, call, ref, rule=None, in_place=False):
    """a fine-grained call with framed device input(s) and a framed device output, once per poison pattern.  inputs: the input
    bytes; in_place: the input buffer is the output (its frames are guards and poison at once)."""
    import torch
    runs = []
    for which in range(len(POISON_WORDS)):
        src = framed("device", fmt_in, which, 1 << 20, inputs, 1 << 20)
        out = src if in_place else framed_out("device", 64 << 10, out_bytes)
        call(C.c_void_p(src.body.data_ptr()), C.c_void_p(out.body.data_ptr()))
        torch.cuda.synchronize()
        if in_place:
            snap = src.snapshot()
            assert np.array_equal(snap[:src.lo], src.uploaded[:src.lo]) and np.array_equal(snap[src.hi:], src.uploaded[src.hi:]), "frames of an in-place call changed"
            r = FootprintRun(framed_out("host", 64, out_bytes))
            r.payload = snap[src.lo:src.hi]
            runs.append(r)
        else:
            runs.append(FootprintRun(out, src))
    bad = footprint_violations(runs, ref, rule)
    assert not bad, bad


def test_fine_grained_calls_on_framed_device_memory(engine, oracle, fsk):
    from quadrs_amd import _ffi
    L, DEV, chk = _ffi.lib(), _ffi.MEM_DEVICE, _ffi.check
    rng = np.random.default_rng(3)
    # unpack: cs8 and cs16, a sample count that is no multiple of any vector
    for fmt, bps in ((1, 2), (3, 4)):
        raw = rng.integers(0, 256, bps * 5003, dtype=np.uint8)
        _fine(engine, fmt, raw, 5003 * 8, lambda s, o: chk(L.qd_unpack(fmt, s, 5003, o, DEV)), oracle.unpack(fmt, raw.tobytes()))
    # shift, in place
    x = (rng.standard_normal((30_001, 2)) * 0.1).astype(np.float32)
    ratio = engine.shift_ratio(-123_456, 2_000_000)
    want = oracle.shift_apply(x, 777_777_777, ratio)
    _fine(engine, 0, x, x.nbytes, lambda s, o: chk(L.qd_shift(s, 30_001, 777_777_777, ratio, DEV)), want, in_place=True,
          rule=lambda pl: [] if complex_ulp_err(want, pl.view(np.float32).reshape(-1, 2)).max() <= 1.0 else ["shift further than 1 ulp"])
    # lowpass block: a full block, and a short read (valid < raw: the samples behind `valid` are frame)
    taps = oracle.taps(1000, 16000, 64)
    raw = rng.standard_normal((200 * 8 + 64, 2)).astype(np.float32)
    for valid in (raw.shape[0], raw.shape[0] - 7):
        n_ref, ref = oracle.lowpass_block(taps, 8, raw, valid=valid)
        produced = C.c_size_t(0)
        _fine(engine, 0, raw[:valid], n_ref * 8,
              lambda s, o: chk(L.qd_lowpass_block(taps.ctypes.data_as(C.c_void_p), 64, 8, s, valid, o, n_ref, C.byref(produced), DEV)), ref[:n_ref])
        assert produced.value == n_ref
    # fft + norm, windows that overlap (in_stride != W)
    W, n_fft, stride = 256, 5, 129
    xin = rng.standard_normal(((n_fft - 1) * stride + W, 2)).astype(np.float32)
    ref = np.stack([oracle.norm(oracle.fft(xin[i * stride:i * stride + W]))[np.r_[W // 2:W, 0:W // 2]] for i in range(n_fft)])
    _fine(engine, 0, xin, ref.nbytes, lambda s, o: chk(L.qd_fft_norm_batch(s, W, n_fft, stride, o, DEV)), ref)
    # take_fft: a power of two (bit for bit) and a Bluestein width (the bound of test_take_fft_any_width_against_f64_dft)
    xs = np.frombuffer(fsk, dtype=np.float32).reshape(-1, 2)
    for W, out_len in ((256, 32), (100, 48)):
        rc, ref, offs = oracle.Chain.from_bytes(fsk, oracle.FMT_CF32, SR).take_fft(W, out_len, None, 1)
        assert rc == 0
        lo, hi = int(offs.min()), int(offs.max()) + W
        rule = None
        if W == 100:
            l1 = np.array([np.abs(xs[int(o):int(o) + W].astype(np.float64)).sum() for o in offs])[:, None]
            allowed = 2.0 * np.spacing(ref).astype(np.float64) + 1e-12 * l1
            rule = lambda pl, ref=ref, allowed=allowed: [] if (np.abs(pl.view(np.float32).reshape(ref.shape).astype(np.float64) - ref) <= allowed).all() \
                else ["take_fft rows outside 2 ulp + 1e-12 l1"]
        _fine(engine, 0, xs[lo:hi], ref.nbytes,
              lambda s, o: chk(L.qd_take_fft(s, lo, hi - lo, xs.shape[0], 1, 0, xs.shape[0] - W, W, 1, out_len, o, DEV)), ref, rule=rule)
    # gen: an output only
    cos = np.array([1000, -2500], dtype=np.int64)
    want_g = oracle.Chain.gen([1000, -2500], 48000).read_at(1 << 20, 1001)[1]
    _fine(engine, 0, np.zeros(8, np.uint8), 1001 * 8, lambda s, o: chk(L.qd_gen(cos.ctypes.data_as(C.c_void_p), 2, 48000, 1 << 20, 1001, o, DEV)), want_g,
          rule=lambda pl: [] if complex_ulp_err(want_g, pl.view(np.float32).reshape(-1, 2)).max() <= 1.0 else ["gen further than 1 ulp"])
