"""qd_plan_spread on the GPU: byte for byte against qd_spread_finish(qd_spread_fold) of the same plan's qd_plan_run norms, which
test_gpu_pool's `world` holds to the oracle, and against the integer referee of test_spread_cpu; at every width where the fold kernel's
geometry changes and over every plan kind; its mean and rms rows against Plan.mean and Plan.power of the same call; independent of
batches, memory kinds and call order — both endings of a row (rounded in the fold kernel, or through the limb accumulator) and the
accumulator's moves included; std <= rms, std <= peak, std == +0 where peak == floor; each output alone; planted values, the short cascade
and the refusals.  Golden files only."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cascade import PROBE, _data
from test_gpu_pool import FAMILIES, SR, WIDTHS, pools_of, world  # noqa: F401  (world: the module-scoped fixture)
from test_spread_cpu import NAMES, NAN64_BITS, NAN_BITS, ref_spread, same
from test_pool_cpu import F32

pytestmark = pytest.mark.gpu

DTYPES = (F32, np.float64, np.uint32, F32, F32)


def host(five):
    import torch
    torch.cuda.synchronize()
    out = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in five]
    if out[2] is not None:
        out[2] = out[2].view(np.uint32)
    return tuple(out)


def twin(engine, norms, pool, at=0, into=None):
    return engine.spread_finish(engine.spread_fold(norms, pool, at=at, into=into))


def identity_ref(norms):
    """pool == 1 restated without a sum: std +0 and ssd 0.0 where there is a finite value, NaNs where there is an infinity, the value
    itself as mean and rms, and whether it is there"""
    keep, inf = ~np.isnan(norms), np.isinf(norms)
    mag = np.where(keep, np.abs(norms).view(np.uint32), np.uint32(NAN_BITS)).astype(np.uint32).view(F32)
    std = np.where(keep & ~inf, np.uint32(0), np.uint32(NAN_BITS)).astype(np.uint32).view(F32)
    ssd = np.where(inf, np.uint64(NAN64_BITS), np.uint64(0)).astype(np.uint64).view(np.float64)
    return std, ssd, keep.astype(np.uint32), mag, mag


@pytest.mark.parametrize("name", WIDTHS + FAMILIES)
def test_matches_the_fold_of_the_plans_norms(engine, world, name):
    plan, data, dev, norms, n, spec = world(name)
    for pool in pools_of(plan, n):
        got = host(plan.spread(dev, pool, n_windows=n))
        ref = twin(engine, norms, pool)
        assert got[0].shape == (-(-n // min(pool, n)), spec[3]["width"])
        assert same(got, ref), pool
        if pool == 1:
            assert same(got, identity_ref(norms))
        elif name in ("cf32_w4", "shift_fir_w128"):
            assert same(ref[:3], ref_spread(norms, min(pool, n))), pool
        # the halves of the cell are the other two sinks' results of the same call
        mean = host(plan.mean(dev, pool, n_windows=n))
        power = host(plan.power(dev, pool, n_windows=n))
        assert same(got, (None, None, mean[2], mean[0], power[0])), pool
        if not np.isnan(norms).any():
            # the deviation is at most the root mean square and at most the largest value, and +0 where the group never moved
            peak, floor = (t.cpu().numpy() for t in plan.pool(dev, pool, n_windows=n))
            assert (got[0] <= got[4]).all() and (got[0] <= peak).all(), pool
            assert not got[0].view(np.uint32)[peak == floor].any(), pool


@pytest.mark.parametrize("name", ["cf32_w128", "cf32_w4", "shift_fir_w128", "cascade_w16_s8"])
def test_batch_seams_and_sources(engine, world, name):
    """chunk_bytes = 64 KiB: batches end inside rows of the large pools and on row boundaries of the small ones, and pool 37 opens more
    rows than the limb accumulator holds; pageable, pinned and device sources; host and device outputs; twice and thrice on a plan"""
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    small = engine.Plan(fmt, rate, n_samples, chunk_bytes=1 << 16, **kw)
    if name == "cf32_w128":
        cw = (1 << 16) // (128 * 4)                              # windows a batch holds
        assert n >= 3 * cw and 1000 > cw and n > cw              # pools 1000 and n: a row spans a seam (through the accumulator)
        assert 3 <= cw and 7 <= cw                               # pools 3 and 7: seams fall between rows (rounded in the fold kernel)
        assert -(-n // 37) > 2 * (1 << 16) // (128 * 224)         # pool 37: more rows than the accumulator of 2 chunk_bytes holds
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    for pool in (3, 7, 37, 1000, n):
        whole = twin(engine, norms, pool)
        for p in (plan, small):
            assert same(host(p.spread(dev, pool, n_windows=n)), whole), pool                          # device -> device
            assert same(p.spread(dev, pool, n_windows=n, device_out=False), whole), pool              # device -> host
            assert same(p.spread(data, pool, n_windows=n), whole), pool                               # pageable -> host
            assert same(host(p.spread(data, pool, n_windows=n, device_out=True)), whole), pool        # pageable -> device
            assert same(p.spread(pin.array, pool, n_windows=n, pinned=True), whole), pool             # pinned -> host
    # further calls on the same plan reuse the workspace: a smaller result after a larger one, and the first again
    a = plan.spread(data, 1, n_windows=n)
    b = plan.spread(data, n, n_windows=n)
    c = plan.spread(data, 1, n_windows=n)
    assert same(a, twin(engine, norms, 1)) and same(b, twin(engine, norms, n)) and same(c, a)
    a = small.spread(dev, 1, n_windows=n, device_out=False)
    b = small.spread(dev, n, n_windows=n, device_out=False)
    assert same(a, twin(engine, norms, 1)) and same(b, twin(engine, norms, n))
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
        ref = twin(engine, norms[first:first + count], pool)          # rows count from the range's first window
        assert same(plan.spread(slab, pool, first, count, src_first=a), ref), pool
        sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
        assert same(host(plan.spread(sd, pool, first, count, src_first=a)), ref), pool


def test_each_output_alone(engine, world):
    import torch
    from quadrs_amd import _ffi
    plan, data, dev, norms, n, _ = world("cf32_w128")
    buf = np.frombuffer(data, dtype=np.uint8)
    tdts = (torch.float32, torch.float64, torch.int32, torch.float32, torch.float32)
    for pool in (5, 1000):                                       # rows rounded in the fold kernel; rows through the accumulator
        ref = twin(engine, norms, pool)
        R = ref[0].shape[0]
        for which, (dt, tdt) in enumerate(zip(DTYPES, tdts)):
            fill = 77 if dt is np.uint32 else -7.5
            out = np.full((R + 2, 128), fill, dtype=dt)             # a guard row on either side
            ptrs = [None] * 5
            ptrs[which] = out.ctypes.data + 128 * out.itemsize
            rows = _ffi.SpreadRows(*ptrs)
            _ffi.check(_ffi.lib().qd_plan_spread(plan._h, buf.ctypes.data_as(C.c_void_p), _ffi.MEM_HOST, 0, buf.size // 8, 0, n, pool, C.byref(rows),
                                                _ffi.MEM_HOST, None))
            assert out[1:R + 1].tobytes() == ref[which].tobytes(), (pool, NAMES[which])
            assert (out[0] == dt(fill)).all() and (out[R + 1] == dt(fill)).all()
            # device memory at an address that is not a multiple of 16
            t = torch.full(((R + 2) * 128 + 1,), fill, dtype=tdt, device="cuda")
            ptrs[which] = t.data_ptr() + out.itemsize * (128 + 1)
            assert ptrs[which] % 16 != 0
            rows = _ffi.SpreadRows(*ptrs)
            _ffi.check(_ffi.lib().qd_plan_spread(plan._h, C.c_void_p(dev.data_ptr()), _ffi.MEM_DEVICE, 0, buf.size // 8, 0, n, pool, C.byref(rows),
                                                _ffi.MEM_DEVICE, None))
            torch.cuda.synchronize()
            h = t.cpu().numpy().view(dt)
            assert h[129:129 + R * 128].tobytes() == ref[which].tobytes(), (pool, NAMES[which])
            assert (h[:129] == dt(fill)).all() and (h[129 + R * 128:] == dt(fill)).all()
        # through the Python view: a subset leaves the others None
        got = plan.spread(data, pool, n_windows=n, outputs=("std", "mean"))
        assert same(got, (ref[0], None, None, ref[3], None)) and got[1] is None and got[2] is None and got[4] is None


@pytest.mark.parametrize("W", [2, 64])
def test_planted_values(engine, fsk, W):
    x = np.frombuffer(fsk, dtype=F32).reshape(-1, 2)[:8192].copy()
    x[3 * W:4 * W] = (np.nan, 0.25)                # window 3 is NaN throughout
    x[5 * W + 1] = (np.inf, 0.0)                   # window 5
    x[9 * W] = (0.5, -np.nan)
    x[20 * W:24 * W] *= F32(1e30)                  # windows 20 .. 23: norms near the top of the range, squares past the f32 range
    x[30 * W:34 * W] *= F32(1e-42)                 # windows 30 .. 33: subnormal samples, subnormal norms, squares far below the f32 range
    plan = engine.Plan(engine.FMT_CF32, SR, x.shape[0], width=W)
    norms = plan.run_host(x)
    nan = np.isnan(norms)
    assert nan[3].all() and nan[9].all() and np.isinf(norms[5]).any()
    assert (norms < F32(1.2e-38)).any() and (norms > F32(1e30)).any()
    n = norms.shape[0]
    for pool in (1, 2, 3, 4, 16, n):
        got = plan.spread(x, pool)
        assert same(got, twin(engine, norms, pool)), pool
        assert same(got[:3], ref_spread(norms, pool)) if pool > 1 else same(got, identity_ref(norms)), pool
        R = got[0].shape[0]
        live = np.stack([(~nan[r * pool:(r + 1) * pool]).sum(axis=0) for r in range(R)])
        infs = np.stack([np.isinf(norms[r * pool:(r + 1) * pool]).any(axis=0) for r in range(R)])
        assert (got[2] == live).all(), pool
        none = live == 0
        assert (got[0].view(np.uint32)[none | infs] == NAN_BITS).all() and not np.isnan(got[0][~none & ~infs]).any()
        assert not got[1].view(np.uint64)[none].any() and (got[1].view(np.uint64)[infs] == NAN64_BITS).all()
    assert plan.spread(x, 1)[2][3].sum() == 0


def test_short_cascade_folds_its_complete_windows(engine):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    for pool, first in ((1, 0), (3, 0), (total, 0), (1, done - 1), (2, done)):
        with pytest.raises(engine.QuadrsError) as e:
            plan.spread(data, pool, first_window=first)
        assert e.value.code == engine._ffi.ERR_SHORT
        count = total - first
        acc = engine.spread_init(4, -(-count // min(pool, count)))
        if done > first:
            engine.spread_fold(norms[first:done], pool, into=acc)
        assert same(e.value.partial, engine.spread_finish(acc)), (pool, first)
    last = e.value.partial                          # pool 2 from the first incomplete window on: no values anywhere
    assert not last[1].view(np.uint64).any() and not last[2].any()
    assert all((last[i].view(np.uint32) == NAN_BITS).all() for i in (0, 3, 4))


def test_refusals(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8

    def code(plan, *a, **k):
        with pytest.raises(engine.QuadrsError) as e:
            plan.spread(fsk, *a, **k)
        return e.value.code
    for epi in (engine.EPI_GLYPH_U8, engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
        assert code(engine.Plan(0, SR, n, width=64, epilogue=epi), 3) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, SR, n, width=64, stride=1, epilogue=engine.EPI_ROWS_F32), 3, n_windows=1) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, SR, n, width=64, shard_devices=[0, 0]), 3) == _ffi.ERR_UNSUPPORTED
    plan = engine.Plan(0, SR, n, width=64)
    assert code(plan, 0) == _ffi.ERR_INVALID
    assert code(plan, 3, 0, plan.n_windows + 1) == _ffi.ERR_SHORT
    assert code(plan, 3, plan.n_windows, 1) == _ffi.ERR_SHORT
    buf = np.frombuffer(fsk, dtype=np.uint8)
    out = np.full(64, F32(-7.5))
    L, src = _ffi.lib(), buf.ctypes.data_as(C.c_void_p)
    dst, none = C.byref(_ffi.SpreadRows(out.ctypes.data, None, None, None, None)), C.byref(_ffi.SpreadRows(None, None, None, None, None))
    assert L.qd_plan_spread(plan._h, src, _ffi.MEM_HOST, 0, n, 0, 4, 2, none, _ffi.MEM_HOST, None) == _ffi.ERR_INVALID
    assert L.qd_plan_spread(plan._h, src, _ffi.MEM_HOST, 0, n, 0, 4, 2, None, _ffi.MEM_HOST, None) == _ffi.ERR_INVALID
    assert L.qd_plan_spread(plan._h, src, 9, 0, n, 0, 4, 2, dst, _ffi.MEM_HOST, None) == _ffi.ERR_INVALID
    assert L.qd_plan_spread(plan._h, src, _ffi.MEM_HOST, 0, n, 0, 4, 2, dst, 9, None) == _ffi.ERR_INVALID
    assert L.qd_plan_spread(plan._h, src, _ffi.MEM_HOST, 0, n, plan.n_windows, 1, 2, dst, _ffi.MEM_HOST, None) == _ffi.ERR_SHORT
    assert L.qd_plan_spread(plan._h, src, _ffi.MEM_HOST, 0, n, 5, 0, 2, dst, _ffi.MEM_HOST, None) == 0   # no windows: nothing is touched
    assert (out == F32(-7.5)).all()
    got = plan.spread(fsk, 3, 5, 0)
    assert all(g.shape == (0, 64) for g in got)
