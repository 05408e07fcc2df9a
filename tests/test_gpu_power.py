"""qd_plan_power on the GPU: byte for byte against qd_power_finish(qd_power_fold) of the same plan's qd_plan_run norms, which test_gpu_pool's
`world` holds to the oracle, and against the integer referee of test_power_cpu; at every width where the fold kernel's geometry changes
and over every plan kind; independent of batches, memory kinds and call order — both endings of a row
(rounded in the fold kernel, or through the limb accumulator) and the accumulator's moves included; floor <= mean <= rms <= peak; planted
values, the short cascade and the refusals.  Golden files only."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cascade import PROBE, _data
from test_gpu_pool import FAMILIES, SR, WIDTHS, pools_of, world  # noqa: F401  (world: the module-scoped fixture)
from test_power_cpu import NAN_BITS, ref_power, same3
from test_pool_cpu import F32

pytestmark = pytest.mark.gpu


def host(three):
    import torch
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in three)
    return out[0], out[1], out[2].view(np.uint32)


def twin(engine, norms, pool, at=0, into=None):
    return engine.power_finish(engine.power_fold(norms, pool, at=at, into=into))


def identity_ref(norms):
    """pool == 1 restated without a sum: the value, the square of its double (a 48-bit product: exact), and whether it is there"""
    keep = ~np.isnan(norms)
    rms = np.where(keep, np.abs(norms).view(np.uint32), np.uint32(NAN_BITS)).astype(np.uint32).view(F32)
    d = np.abs(norms).astype(np.float64)
    return rms, np.where(keep, d * d, 0.0), keep.astype(np.uint32)


@pytest.mark.parametrize("name", WIDTHS + FAMILIES)
def test_matches_the_fold_of_the_plans_norms(engine, world, name):
    plan, data, dev, norms, n, spec = world(name)
    for pool in pools_of(plan, n):
        got = host(plan.power(dev, pool, n_windows=n))
        ref = twin(engine, norms, pool)
        assert got[0].shape == (-(-n // min(pool, n)), spec[3]["width"])
        assert same3(got, ref), pool
        if pool == 1:
            assert same3(got, identity_ref(norms))
        elif name in ("cf32_w4", "shift_fir_w128"):
            assert same3(ref, ref_power(norms, min(pool, n))), pool
        if not np.isnan(norms).any():
            # the traces of one plan and pool order cell by cell (equal values: equal traces, every one rounded to nearest)
            peak, floor = (t.cpu().numpy() for t in plan.pool(dev, pool, n_windows=n))
            mean = host(plan.mean(dev, pool, n_windows=n))[0]
            assert (floor <= mean).all() and (mean <= got[0]).all() and (got[0] <= peak).all(), pool


@pytest.mark.parametrize("name", ["cf32_w128", "cf32_w4", "shift_fir_w128", "cascade_w16_s8"])
def test_batch_seams_and_sources(engine, world, name):
    """chunk_bytes = 64 KiB: batches end inside rows of the large pools and on row boundaries of the small ones, and pool 37 opens more
    rows than the limb accumulator holds; pageable, pinned and device sources; host and device outputs; twice on a plan"""
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    small = engine.Plan(fmt, rate, n_samples, chunk_bytes=1 << 16, **kw)
    if name == "cf32_w128":
        cw = (1 << 16) // (128 * 4)                              # windows a batch holds
        assert n >= 3 * cw and 1000 > cw and n > cw              # pools 1000 and n: a row spans a seam
        assert 3 <= cw and 7 <= cw                               # pools 3 and 7: seams fall between rows
        assert -(-n // 37) > 2 * (1 << 16) // (128 * 152)         # pool 37: more rows than the accumulator of 2 chunk_bytes holds
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    for pool in (3, 7, 37, 1000, n):
        whole = twin(engine, norms, pool)
        for p in (plan, small):
            assert same3(host(p.power(dev, pool, n_windows=n)), whole), pool                          # device -> device
            assert same3(p.power(dev, pool, n_windows=n, device_out=False), whole), pool              # device -> host
            assert same3(p.power(data, pool, n_windows=n), whole), pool                               # pageable -> host
            assert same3(host(p.power(data, pool, n_windows=n, device_out=True)), whole), pool        # pageable -> device
            assert same3(p.power(pin.array, pool, n_windows=n, pinned=True), whole), pool             # pinned -> host
    # a second call on the same plan reuses the workspace: a smaller result after a larger one, and the first again
    a = plan.power(data, 1, n_windows=n)
    b = plan.power(data, n, n_windows=n)
    c = plan.power(data, 1, n_windows=n)
    assert same3(a, twin(engine, norms, 1)) and same3(b, twin(engine, norms, n)) and same3(c, a)
    a = small.power(dev, 1, n_windows=n, device_out=False)
    b = small.power(dev, n, n_windows=n, device_out=False)
    assert same3(a, twin(engine, norms, 1)) and same3(b, twin(engine, norms, n))
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
        assert same3(plan.power(slab, pool, first, count, src_first=a), ref), pool
        sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
        assert same3(host(plan.power(sd, pool, first, count, src_first=a)), ref), pool


def test_one_output_only(engine, world):
    import torch
    from quadrs_amd import _ffi
    plan, data, dev, norms, n, _ = world("cf32_w128")
    buf = np.frombuffer(data, dtype=np.uint8)
    for pool in (5, 1000):                                       # rows rounded in the fold kernel; rows through the accumulator
        ref = twin(engine, norms, pool)
        R = ref[0].shape[0]
        for which, (dt, tdt, fill) in enumerate(((F32, torch.float32, -7.5), (np.float64, torch.float64, -7.5), (np.uint32, torch.int32, 77))):
            out = np.full((R + 2, 128), fill, dtype=dt)             # a guard row on either side
            ptrs = [None, None, None]
            ptrs[which] = C.c_void_p(out.ctypes.data + 128 * out.itemsize)
            _ffi.check(_ffi.lib().qd_plan_power(plan._h, buf.ctypes.data_as(C.c_void_p), _ffi.MEM_HOST, 0, buf.size // 8, 0, n, pool, *ptrs,
                                               _ffi.MEM_HOST, None))
            assert out[1:R + 1].tobytes() == ref[which].tobytes() and (out[0] == dt(fill)).all() and (out[R + 1] == dt(fill)).all()
            # device memory at an address that is not a multiple of 16
            t = torch.full(((R + 2) * 128 + 1,), fill, dtype=tdt, device="cuda")
            ptrs[which] = C.c_void_p(t.data_ptr() + out.itemsize * (128 + 1))
            assert (t.data_ptr() + out.itemsize * (128 + 1)) % 16 != 0
            _ffi.check(_ffi.lib().qd_plan_power(plan._h, C.c_void_p(dev.data_ptr()), _ffi.MEM_DEVICE, 0, buf.size // 8, 0, n, pool, *ptrs,
                                               _ffi.MEM_DEVICE, None))
            torch.cuda.synchronize()
            h = t.cpu().numpy().view(dt)
            assert h[129:129 + R * 128].tobytes() == ref[which].tobytes() and (h[:129] == dt(fill)).all() and (h[129 + R * 128:] == dt(fill)).all()


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
        got = plan.power(x, pool)
        assert same3(got, twin(engine, norms, pool)), pool
        assert same3(got, ref_power(norms, pool) if pool > 1 else identity_ref(norms)), pool
        R = got[0].shape[0]
        live = np.stack([(~nan[r * pool:(r + 1) * pool]).sum(axis=0) for r in range(R)])
        assert (got[2] == live).all(), pool
        none = live == 0
        assert (got[0].view(np.uint32)[none] == NAN_BITS).all() and not got[1][none].any() and not np.isnan(got[0][~none]).any()
    assert plan.power(x, 1)[2][3].sum() == 0


def test_short_cascade_folds_its_complete_windows(engine):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    for pool, first in ((1, 0), (3, 0), (total, 0), (1, done - 1), (2, done)):
        with pytest.raises(engine.QuadrsError) as e:
            plan.power(data, pool, first_window=first)
        assert e.value.code == engine._ffi.ERR_SHORT
        count = total - first
        acc = engine.power_init(4, -(-count // min(pool, count)))
        if done > first:
            engine.power_fold(norms[first:done], pool, into=acc)
        assert same3(e.value.partial, engine.power_finish(acc)), (pool, first)
    last = e.value.partial                          # pool 2 from the first incomplete window on: no values anywhere
    assert (last[0].view(np.uint32) == NAN_BITS).all() and not last[1].any() and not last[2].any()


def test_refusals(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8

    def code(plan, *a, **k):
        with pytest.raises(engine.QuadrsError) as e:
            plan.power(fsk, *a, **k)
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
    L, src, dst = _ffi.lib(), buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.qd_plan_power(plan._h, src, _ffi.MEM_HOST, 0, n, 0, 4, 2, None, None, None, _ffi.MEM_HOST, None) == _ffi.ERR_INVALID
    assert L.qd_plan_power(plan._h, src, 9, 0, n, 0, 4, 2, dst, None, None, _ffi.MEM_HOST, None) == _ffi.ERR_INVALID
    assert L.qd_plan_power(plan._h, src, _ffi.MEM_HOST, 0, n, 0, 4, 2, dst, None, None, 9, None) == _ffi.ERR_INVALID
    assert L.qd_plan_power(plan._h, src, _ffi.MEM_HOST, 0, n, plan.n_windows, 1, 2, dst, None, None, _ffi.MEM_HOST, None) == _ffi.ERR_SHORT
    assert L.qd_plan_power(plan._h, src, _ffi.MEM_HOST, 0, n, 5, 0, 2, dst, None, None, _ffi.MEM_HOST, None) == 0   # no windows: nothing is touched
    assert (out == F32(-7.5)).all()
    got = plan.power(fsk, 3, 5, 0)
    assert all(g.shape == (0, 64) for g in got)
