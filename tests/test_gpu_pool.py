"""qd_plan_pool on the GPU: bit for bit against qd_pool_fold of the same plan's qd_plan_run norms, which are held to the oracle (exactly
without a shift, by the NCO rule behind one), at every width where k_pool's geometry changes and over every plan kind; independent of
batches, memory kinds and call order; values, the short cascade and the refusals.  Golden files only."""
import math

import numpy as np
import pytest

from test_gpu_cascade import PROBE, _data
from test_gpu_parity import assert_norms_close
from test_gpu_summary import quantised
from test_pool_cpu import F32, INF, np_pool, same

pytestmark = pytest.mark.gpu

SR = 21_000_000


# name -> (format, sample rate, stream, plan keywords, oracle stages)
def _cases(cupboard, fsk):
    cf32 = fsk * 4                                   # 262 144 samples
    c = {f"cf32_w{W}": (0, SR, cf32, dict(width=W), []) for W in (1, 2, 4, 128, 256, 2048)}
    c.update({
        "nofir_w4_s2": (0, 400, cupboard, dict(width=4, stride=2), []),
        "cs8_fir_w64_s16": (1, SR, quantised(fsk, 1), dict(lowpass=(200000, 32, 400), width=64, stride=16), [("lowpass", (200000, 32, 400))]),
        "shift_fir_w128": (0, SR, cf32, dict(shift_hz=280000, lowpass=(2_000_000, 16, 40), width=128),
                           [("shift", 280000), ("lowpass", (2_000_000, 16, 40))]),
        "cascade_w16_s8": (0, SR, fsk, dict(stages=[("lowpass", (2_000_000, 4, 40)), ("lowpass", (500_000, 4, 40))], width=16, stride=8),
                           [("lowpass", (2_000_000, 4, 40)), ("lowpass", (500_000, 4, 40))]),
        "two_stage_w1024": (1, SR, quantised(fsk, 1, reps=4), dict(lowpass=(200000, 32, 40), width=1024), [("lowpass", (200000, 32, 40))]),
    })
    return c


WIDTHS = [f"cf32_w{W}" for W in (1, 2, 4, 128, 256, 2048)]
FAMILIES = ["nofir_w4_s2", "cs8_fir_w64_s16", "shift_fir_w128", "cascade_w16_s8", "two_stage_w1024"]


@pytest.fixture(scope="module")
def world(engine, oracle, cupboard, fsk):
    """per case, made once: the plan, the stream (host bytes and a device tensor), its complete windows and their qd_plan_run norms,
    held to the oracle here"""
    import torch
    cache, cases = {}, _cases(cupboard, fsk)

    def get(name):
        if name not in cache:
            fmt, rate, data, kw, stages = cases[name]
            n_samples = len(data) // {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
            plan = engine.Plan(fmt, rate, n_samples, **kw)
            dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            n = plan.complete_windows()
            assert n >= 6
            norms = plan.run_host(data, n_windows=n)
            ch = oracle.Chain.from_bytes(data, fmt, rate)
            for kind, arg in stages:
                ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
            ref = ch.spark_fft(kw["width"], kw.get("stride"), max_windows=n, want_codes=False)[0]
            if any(kind == "shift" for kind, _ in stages):
                assert_norms_close(ref, norms, name, explain=(plan, 0))
            else:
                assert_norms_close(ref, norms, name, min_exact=1.0, max_ulp=0)
            norms.setflags(write=False)
            cache[name] = (plan, data, dev, norms, n, (fmt, rate, n_samples, kw))
        return cache[name]
    return get


def pools_of(plan, n):
    G = max(int(plan.info.tile_windows), 1)
    odd = next(p for p in range(5, 10_000) if math.gcd(p, G) == 1 and p not in (1, 3, n, n + 5))
    return [1, 3, odd, n, n + 5]


def host(pair):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in pair)


@pytest.mark.parametrize("name", WIDTHS + FAMILIES)
def test_matches_the_fold_of_the_plans_norms(engine, world, name):
    plan, data, dev, norms, n, spec = world(name)
    if name == "two_stage_w1024":
        assert plan.info.raw_per_window * 8 > 160 * 1024          # the window's cf32 samples do not fit the LDS tile: stage A + stage B
    for pool in pools_of(plan, n):
        got = host(plan.pool(dev, pool, n_windows=n))
        ref = engine.pool_fold(norms, pool)
        assert got[0].shape == (-(-n // min(pool, n)), spec[3]["width"])
        assert same(got, ref), pool
        assert same(ref, np_pool(norms, pool))
        if pool == 1:
            keep = ~np.isnan(norms)
            assert got[0][keep].tobytes() == norms[keep].tobytes() and got[1][keep].tobytes() == norms[keep].tobytes()
        if pool >= n:
            s = plan.summarize(dev, n_windows=n)
            assert got[0][0].tobytes() == s.peak.tobytes() and got[1][0].tobytes() == s.floor.tobytes()


@pytest.mark.parametrize("name", ["cf32_w128", "cf32_w4", "shift_fir_w128", "cascade_w16_s8"])
def test_batch_seams_and_sources(engine, world, name):
    """chunk_bytes = 64 KiB: batches end inside rows; pageable, pinned and device sources; host and device outputs; twice on a plan"""
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    small = engine.Plan(fmt, rate, n_samples, chunk_bytes=1 << 16, **kw)
    if name == "cf32_w128":
        assert n * kw["width"] * 4 >= 3 * (1 << 16)
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    for pool in (3, 7, 1000, n):
        whole = engine.pool_fold(norms, pool)
        for p in (plan, small):
            assert same(host(p.pool(dev, pool, n_windows=n)), whole), pool                          # device -> device
            assert same(p.pool(dev, pool, n_windows=n, device_out=False), whole), pool              # device -> host
            assert same(p.pool(data, pool, n_windows=n), whole), pool                               # pageable -> host
            assert same(host(p.pool(data, pool, n_windows=n, device_out=True)), whole), pool        # pageable -> device
            assert same(p.pool(pin.array, pool, n_windows=n, pinned=True), whole), pool             # pinned -> host
    # a second call on the same plan reuses the workspace: a smaller result after a larger one, and the first again
    a = plan.pool(data, 1, n_windows=n)
    b = plan.pool(data, n, n_windows=n)
    c = plan.pool(data, 1, n_windows=n)
    assert same(a, engine.pool_fold(norms, 1)) and same(b, engine.pool_fold(norms, n)) and same(c, a)
    pin.close()


@pytest.mark.parametrize("name", ["cf32_w128", "cs8_fir_w64_s16", "cascade_w16_s8"])
def test_sub_range_from_a_slab(engine, world, name):
    import torch
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    bps = {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
    first, count = 2, n - 3
    a, cnt = plan.src_range(first, count)
    slab = data[a * bps:(a + cnt) * bps]
    for pool in (1, 3, 5, count):
        ref = engine.pool_fold(norms[first:first + count], pool)        # rows count from the range's first window
        assert same(plan.pool(slab, pool, first, count, src_first=a), ref), pool
        sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
        assert same(host(plan.pool(sd, pool, first, count, src_first=a)), ref), pool


def test_one_output_only(engine, world):
    import ctypes as C
    import torch
    from quadrs_amd import _ffi
    plan, data, dev, norms, n, _ = world("cf32_w128")
    ref = engine.pool_fold(norms, 5)
    R = ref[0].shape[0]
    buf = np.frombuffer(data, dtype=np.uint8)
    for which in (0, 1):
        out = np.full((R + 2, 128), F32(-7.5))                   # a guard row on either side
        ptrs = [None, None]
        ptrs[which] = C.c_void_p(out.ctypes.data + 128 * 4)
        _ffi.check(_ffi.lib().qd_plan_pool(plan._h, buf.ctypes.data_as(C.c_void_p), _ffi.MEM_HOST, 0, buf.size // 8, 0, n, 5, ptrs[0], ptrs[1],
                                           _ffi.MEM_HOST, None))
        assert out[1:R + 1].tobytes() == ref[which].tobytes() and (out[0] == F32(-7.5)).all() and (out[R + 1] == F32(-7.5)).all()
        # device memory at an address that is not a multiple of 16
        t = torch.full(((R + 2) * 128 + 1,), -7.5, dtype=torch.float32, device="cuda")
        ptrs[which] = C.c_void_p(t.data_ptr() + 4 * (128 + 1))
        _ffi.check(_ffi.lib().qd_plan_pool(plan._h, C.c_void_p(dev.data_ptr()), _ffi.MEM_DEVICE, 0, buf.size // 8, 0, n, 5, ptrs[0], ptrs[1],
                                           _ffi.MEM_DEVICE, None))
        torch.cuda.synchronize()
        h = t.cpu().numpy()
        assert h[129:129 + R * 128].tobytes() == ref[which].tobytes() and (h[:129] == F32(-7.5)).all() and (h[129 + R * 128:] == F32(-7.5)).all()


@pytest.mark.parametrize("W", [2, 64])
def test_planted_nan_and_inf(engine, fsk, W):
    x = np.frombuffer(fsk, dtype=F32).reshape(-1, 2)[:8192].copy()
    x[3 * W] = (np.nan, 0.25)                      # window 3
    x[5 * W + 1] = (np.inf, 0.0)                   # window 5
    x[9 * W] = (0.5, -np.nan)
    plan = engine.Plan(engine.FMT_CF32, SR, x.shape[0], width=W)
    norms = plan.run_host(x)
    nan = np.isnan(norms)
    assert nan[3].all() and nan[9].all() and nan.sum() >= 2 * W and not np.isfinite(norms[5]).all()
    for pool in (1, 2, 3, 4, norms.shape[0]):
        got = plan.pool(x, pool)
        assert same(got, engine.pool_fold(norms, pool)) and same(got, np_pool(norms, pool)), pool
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
        # the identities stand exactly where a whole group is NaN
        R = got[0].shape[0]
        all_nan = np.stack([nan[r * pool:(r + 1) * pool].all(axis=0) for r in range(R)])
        assert (all_nan == ((got[0] == 0) & (got[1] == INF))).all(), pool
    assert plan.pool(x, 1)[0][3].tobytes() == np.zeros(W, F32).tobytes() and (plan.pool(x, 1)[1][9] == INF).all()


def test_short_cascade_folds_its_complete_windows(engine):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    for pool, first in ((1, 0), (3, 0), (total, 0), (1, done - 1), (2, done)):
        with pytest.raises(engine.QuadrsError) as e:
            plan.pool(data, pool, first_window=first)
        assert e.value.code == engine._ffi.ERR_SHORT
        count = total - first
        ref = engine.pool_init(4, -(-count // min(pool, count)))
        if done > first:
            engine.pool_fold(norms[first:done], pool, into=ref)
        assert same(e.value.partial, ref), (pool, first)
    last = e.value.partial                          # pool 2 from the first incomplete window on: nothing but the identities
    assert not last[0].any() and (last[1] == INF).all()


def test_refusals(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8

    def code(plan, *a, **k):
        with pytest.raises(engine.QuadrsError) as e:
            plan.pool(fsk, *a, **k)
        return e.value.code
    for epi in (engine.EPI_GLYPH_U8, engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
        assert code(engine.Plan(0, SR, n, width=64, epilogue=epi), 3) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, SR, n, width=64, stride=1, epilogue=engine.EPI_ROWS_F32), 3, n_windows=1) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, SR, n, width=64, shard_devices=[0, 0]), 3) == _ffi.ERR_UNSUPPORTED
    plan = engine.Plan(0, SR, n, width=64)
    assert code(plan, 0) == _ffi.ERR_INVALID
    assert code(plan, 3, 0, plan.n_windows + 1) == _ffi.ERR_SHORT
    assert code(plan, 3, plan.n_windows, 1) == _ffi.ERR_SHORT
    import ctypes as C
    buf = np.frombuffer(fsk, dtype=np.uint8)
    out = np.full(64, F32(-7.5))
    L, src, dst = _ffi.lib(), buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.qd_plan_pool(plan._h, src, _ffi.MEM_HOST, 0, n, 0, 4, 2, None, None, _ffi.MEM_HOST, None) == _ffi.ERR_INVALID
    assert L.qd_plan_pool(plan._h, src, 9, 0, n, 0, 4, 2, dst, None, _ffi.MEM_HOST, None) == _ffi.ERR_INVALID
    assert L.qd_plan_pool(plan._h, src, _ffi.MEM_HOST, 0, n, 0, 4, 2, dst, None, 9, None) == _ffi.ERR_INVALID
    assert L.qd_plan_pool(plan._h, src, _ffi.MEM_HOST, 0, n, 5, 0, 2, dst, None, _ffi.MEM_HOST, None) == 0      # no windows: nothing is touched
    assert (out == F32(-7.5)).all()
    peak, floor = plan.pool(fsk, 3, 5, 0)
    assert peak.shape == floor.shape == (0, 64)
