"""qd_plan_density on the GPU: byte for byte, counts and traces, against qd_density_fold / qd_density_quantile of the same plan's
qd_plan_run norms (held to the oracle by test_gpu_pool and test_gpu_parity), on the committed 65 536-sample head: at every width and
level count where k_density's geometry changes, over every pool kind, with batch seams that cut rows and rows split over workgroups,
every memory kind, either output alone between guards, a sub-range, planted NaN / +inf / zero values, every plan kind, the short cascade
and the refusals.  Golden files only."""
import ctypes as C

import numpy as np
import pytest

from test_density_cpu import BUCKETS, INF_BITS, NAN_BITS, ref_counts
from test_gpu_cascade import PROBE, _data
from test_gpu_footprint import FootprintRun, framed_out
from util import GUARD_BYTE, zero_runs

pytestmark = pytest.mark.gpu

F32 = np.float32
SR = 21_000_000
QS = (0.0, 0.5, 0.9, 1.0)
# the column count of the workgroup histogram is 256 for L <= 64, 128 for L <= 128, 64 above: one L on each side of both switches
LEVELS = [1, 8, 64, 65, 128, 129, 256]
# W < 64: several pieces a wave; 64; below, at and above the 256 columns; 2048: more than one column slab at every L
WIDTHS = [4, 32, 64, 128, 256, 512, 2048]
FIR = dict(shift_hz=280000, lowpass=(2_000_000, 16, 40), width=64)


def grid_for(norms, L):
    """level0 so that the median bucket of the norms sits in the middle of L levels"""
    k = (norms.view(np.uint32) & np.uint32(0x7FFFFFFF)) >> 20
    return int(np.clip(int(np.median(k[k <= 2040])) - L // 2, 0, BUCKETS - L))


def pools_of(n):
    return [1, 3, 16, n, n + 5]


@pytest.fixture(scope="module")
def world(engine, fsk):
    """per case, made once: the plan, the stream (host bytes, a device tensor), its complete windows and their qd_plan_run norms"""
    import torch
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            if name == "w2048_s64":
                data, spec = fsk, dict(width=2048, stride=64)
            elif name == "fir":
                data, spec = fsk, dict(FIR)
            elif name.startswith("f"):                               # the whole head
                data, spec = fsk, dict(width=int(name[1:]))
            elif name.startswith("w"):                               # at most 1024 windows of the head
                W = int(name[1:])
                data = fsk[:8 * min(65536, 1024 * W)]                # at most 1024 windows
                spec = dict(width=W)
            else:
                raise KeyError(name)
            spec.update(kw)
            plan = engine.Plan(engine.FMT_CF32, SR, len(data) // 8, **spec)
            n = plan.complete_windows()
            norms = plan.run_host(data, n_windows=n)
            norms.setflags(write=False)
            dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            cache[key] = (plan, data, dev, norms, n, spec)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def twin(engine):
    """the host twin's (counts, traces) of a norms array, computed once per (array, pool, level0, L) and left unchanged"""
    cache = {}

    def get(norms, pool, level0, L, rows=None):
        key = (id(norms), norms.shape, pool, level0, L, rows)
        if key not in cache:
            n, W = norms.shape
            p = min(pool, n) if rows is None else pool            # rows given: the caller has clamped the pool to the range asked
            R = -(-n // p) if rows is None else rows
            counts = engine.density_init(W, L, R)
            if n:
                engine.density_fold(norms, p, level0, L, into=counts)
            traces = np.stack([engine.density_quantile(counts, level0, q)[0] for q in QS]) if R else np.zeros((len(QS), 0, W), F32)
            counts.setflags(write=False)
            traces.setflags(write=False)
            cache[key] = (counts, traces, norms)                     # the array stays alive: its id stays its own
        return cache[key][:2]
    return get


def host(pair):
    import torch
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in pair)
    return (None if out[0] is None else out[0].view(np.uint32)), out[1]


def same2(got, ref):
    got = host(got)
    return all(g.shape == r.shape and g.dtype == r.dtype and g.tobytes() == r.tobytes() for g, r in zip(got, ref)) and len(got) == 2


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("W", WIDTHS)
def test_matches_the_twin_on_the_plans_norms(engine, world, twin, W, L):
    plan, data, dev, norms, n, _ = world(f"w{W}")
    assert n == min(1024, 65536 // W) - 1
    level0 = grid_for(norms, L)
    for pool in pools_of(n):
        got = plan.density(dev, pool, level0, L, q=QS, n_windows=n)
        ref = twin(norms, pool, level0, L)
        assert got[0].shape == (-(-n // min(pool, n)), W, L) and got[1].shape == (len(QS), ref[0].shape[0], W)
        assert same2(got, ref), pool
    if L == 8:
        ref = twin(norms, 3, level0, L)
        assert ref[0].tobytes() == ref_counts(norms, 3, level0, L).tobytes()
        assert (ref[0].sum(axis=2) == np.minimum(3, n - 3 * np.arange(ref[0].shape[0]))[:, None]).all()       # no NaN here: every window counted
        if W <= 256:
            assert len(np.unique(ref[1][1])) > 1                      # the median trace is a picture, not a constant


@pytest.mark.parametrize("name,L", [("f4", 8), ("f4", 256), ("f128", 64), ("f128", 129), ("f256", 64), ("w2048_s64", 8), ("w2048_s64", 256)])
def test_cut_rows_batch_seams_and_rows_split_over_workgroups(engine, world, twin, name, L):
    """chunk_bytes = 64 KiB, the least: batches end inside rows of the large pools; pool = n: one row, cut into pieces of at least 128 windows over
    several workgroups even within one batch; small pools: whole rows, stored"""
    plan, data, dev, norms, n, spec = world(name)
    small = world(name, chunk_bytes=1 << 16)[0]
    W = spec["width"]
    assert n > 128 and n * W * 4 >= 3 * (1 << 16)                   # two pieces a row at pool = n; three batches
    level0 = grid_for(norms, L)
    for pool in ((16, 300, n) if name == "w2048_s64" else (3, 16, 300, n)):
        ref = twin(norms, pool, level0, L)
        for p in (plan, small):
            assert same2(p.density(dev, pool, level0, L, q=QS, n_windows=n), ref), pool


@pytest.mark.parametrize("name", ["f128", "f4", "fir"])
def test_memory_kinds(engine, world, twin, name):
    """pageable, pinned and device sources; host and device outputs (the device accumulator is the caller's array); twice on a plan"""
    plan, data, dev, norms, n, spec = world(name)
    small = world(name, chunk_bytes=1 << 16)[0]
    L = 64
    level0 = grid_for(norms, L)
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    for pool in (3, 7, n):
        ref = twin(norms, pool, level0, L)
        for p in (plan, small):
            kw = dict(q=QS, n_windows=n)
            assert same2(p.density(dev, pool, level0, L, **kw), ref), pool                               # device -> device
            assert same2(p.density(dev, pool, level0, L, device_out=False, **kw), ref), pool             # device -> host
            assert same2(p.density(data, pool, level0, L, **kw), ref), pool                              # pageable -> host
            assert same2(p.density(data, pool, level0, L, device_out=True, **kw), ref), pool             # pageable -> device
            assert same2(p.density(pin.array, pool, level0, L, pinned=True, **kw), ref), pool            # pinned -> host
            assert same2(p.density(pin.array, pool, level0, L, pinned=True, device_out=True, **kw), ref), pool
    # a second call on the same plan reuses the workspace: a smaller result after a larger one, and the first again
    a = plan.density(data, 1, level0, L, q=QS, n_windows=n)
    b = plan.density(data, n, level0, L, q=QS, n_windows=n)
    c = plan.density(data, 1, level0, L, q=QS, n_windows=n)
    assert same2(a, twin(norms, 1, level0, L)) and same2(b, twin(norms, n, level0, L)) and same2(c, twin(norms, 1, level0, L))
    pin.close()


@pytest.mark.parametrize("kind", ["host", "device"])
def test_one_output_only_between_guards(engine, world, twin, kind):
    from quadrs_amd import _ffi
    plan, data, dev, norms, n, _ = world("w128")
    buf = np.frombuffer(data, dtype=np.uint8)
    L = 8
    level0 = grid_for(norms, L)
    qa = (C.c_double * len(QS))(*QS)
    src, smem = (C.c_void_p(dev.data_ptr()), _ffi.MEM_DEVICE) if kind == "device" else (buf.ctypes.data_as(C.c_void_p), _ffi.MEM_HOST)
    omem = _ffi.MEM_DEVICE if kind == "device" else _ffi.MEM_HOST

    def ptr(f):
        return C.c_void_p(f.body.data_ptr() if kind == "device" else f.body.ctypes.data)
    for pool in (5, n):                                              # stored rows; a row through the atomics
        counts, traces = twin(norms, pool, level0, L)
        co, to = framed_out(kind, 64 << 10, counts.nbytes), framed_out(kind, 64 << 10, traces.nbytes)
        _ffi.check(_ffi.lib().qd_plan_density(plan._h, src, smem, 0, buf.size // 8, 0, n, pool, level0, L, ptr(co), None, 0, None, omem, None))
        _ffi.check(_ffi.lib().qd_plan_density(plan._h, src, smem, 0, buf.size // 8, 0, n, pool, level0, L, None, qa, len(QS), ptr(to), omem, None))
        for f, ref in ((co, counts), (to, traces)):
            r = FootprintRun(f)
            assert r.payload.tobytes() == ref.tobytes(), pool
            assert (r.front == GUARD_BYTE).all() and (r.back == GUARD_BYTE).all(), pool
            f.close()


@pytest.mark.parametrize("name", ["w128", "fir"])
def test_sub_range_from_a_slab(engine, world, twin, name):
    import torch
    plan, data, dev, norms, n, _ = world(name)
    first, count = 2, n - 3
    a, cnt = plan.src_range(first, count)
    slab = data[a * 8:(a + cnt) * 8]
    part = norms[first:first + count]
    level0 = grid_for(norms, 64)
    sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
    for pool in (1, 5, count):
        ref = twin(part, pool, level0, 64)                           # rows count from the range's first window
        assert same2(plan.density(slab, pool, level0, 64, QS, first, count, src_first=a), ref), pool
        assert same2(plan.density(sd, pool, level0, 64, QS, first, count, src_first=a), ref), pool


@pytest.mark.parametrize("W", [2, 64])
def test_planted_values(engine, fsk, twin, W):
    """util.zero_runs' stream (runs of zeros of every sign) with NaN and +inf samples, huge and subnormal windows planted"""
    x = np.frombuffer(fsk, dtype=F32).reshape(-1, 2)[:8192].copy()
    x, _ = zero_runs(x, 5 * W, W, seed=3)
    x[3 * W:4 * W] = (np.nan, 0.25)                # window 3 is NaN throughout
    x[5 * W + 1] = (np.inf, 0.0)                   # window 5
    x[9 * W] = (0.5, -np.nan)
    x[20 * W:24 * W] *= F32(1e30)                  # windows 20 .. 23: norms near the top of the range
    x[30 * W:34 * W] *= F32(1e-42)                 # windows 30 .. 33: subnormal samples, subnormal norms
    plan = engine.Plan(engine.FMT_CF32, SR, x.shape[0], width=W)
    norms = plan.run_host(x)
    nan = np.isnan(norms)
    assert nan[3].all() and nan[9].all() and np.isinf(norms[5]).any() and (norms == 0).any()
    assert (norms < F32(1.2e-38)).any() and (norms > F32(1e30)).any()
    n = norms.shape[0]
    for L, level0 in ((64, grid_for(norms, 64)), (256, 0), (256, BUCKETS - 256), (1, 7)):
        for pool in (1, 4, n):
            got = plan.density(x, pool, level0, L, q=QS)
            assert same2(got, twin(norms, pool, level0, L)), (L, level0, pool)
            assert got[0].tobytes() == ref_counts(norms, pool, level0, L).tobytes()
            R = got[0].shape[0]
            live = np.stack([(~nan[r * pool:(r + 1) * pool]).sum(axis=0) for r in range(R)])
            assert (got[0].sum(axis=2) == live).all()
            assert ((got[1].view(np.uint32) == NAN_BITS) == (live == 0)[None]).all()
    top = plan.density(x, n, BUCKETS - 256, 256, q=(1.0,))
    assert top[0][0, :, 255].sum() >= 1 and (top[1].view(np.uint32)[0, 0] == INF_BITS).any()       # +inf: the top level, whose lo is bucket 2040


def test_short_cascade_counts_its_complete_windows(engine, twin):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    level0 = grid_for(norms, 8)
    # whole, without the incomplete window: QD_OK
    assert same2(plan.density(data, 3, level0, 8, q=QS, n_windows=done), twin(norms, 3, level0, 8))
    for pool, first in ((1, 0), (3, 0), (total, 0), (1, done - 1), (2, done)):
        with pytest.raises(engine.QuadrsError) as e:
            plan.density(data, pool, level0, 8, q=QS, first_window=first)
        assert e.value.code == engine._ffi.ERR_SHORT
        count = total - first
        ref = twin(norms[first:done], min(pool, count), level0, 8, rows=-(-count // min(pool, count)))
        assert same2(e.value.partial, ref), (pool, first)
    last = host(e.value.partial)                    # pool 2 from the first incomplete window on: no values anywhere
    assert not last[0].any() and (last[1].view(np.uint32) == NAN_BITS).all()


def test_refusals(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8

    def code(plan, *a, **k):
        with pytest.raises(engine.QuadrsError) as e:
            plan.density(fsk, *a, **k)
        return e.value.code
    for epi in (engine.EPI_GLYPH_U8, engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
        assert code(engine.Plan(0, SR, n, width=64, epilogue=epi), 3, 1000, 8) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, SR, n, width=64, stride=1, epilogue=engine.EPI_ROWS_F32), 3, 1000, 8, n_windows=1) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, SR, n, width=64, shard_devices=[0, 0]), 3, 1000, 8) == _ffi.ERR_UNSUPPORTED
    plan = engine.Plan(0, SR, n, width=64)
    assert code(plan, 0, 1000, 8) == _ffi.ERR_INVALID
    for level0, L in ((1000, 0), (1000, 257), (BUCKETS - 7, 8), (0xFFFFFFFF, 2), (BUCKETS, 1)):
        assert code(plan, 3, level0, L) == _ffi.ERR_INVALID
    for q in (-1e-9, 1.0000001, float("nan")):
        assert code(plan, 3, 1000, 8, q=(0.5, q)) == _ffi.ERR_INVALID
    assert code(plan, 3, 1000, 8, q=(0.5,) * 9) == _ffi.ERR_INVALID
    assert code(plan, 3, 1000, 8, (), 0, plan.n_windows + 1) == _ffi.ERR_SHORT
    assert code(plan, 3, 1000, 8, (), plan.n_windows, 1) == _ffi.ERR_SHORT
    buf = np.frombuffer(fsk, dtype=np.uint8)
    out = np.full(2 * 64 * 8, 77, dtype=np.uint32)
    Lib, src, dst = _ffi.lib(), buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    qa = (C.c_double * 1)(0.5)
    H = _ffi.MEM_HOST
    assert Lib.qd_plan_density(plan._h, src, H, 0, n, 0, 4, 2, 1000, 8, None, None, 0, None, H, None) == _ffi.ERR_INVALID        # no output
    assert Lib.qd_plan_density(plan._h, src, H, 0, n, 0, 4, 2, 1000, 8, None, qa, 0, dst, H, None) == _ffi.ERR_INVALID           # no output asked
    assert Lib.qd_plan_density(plan._h, src, H, 0, n, 0, 4, 2, 1000, 8, dst, qa, 1, None, H, None) == _ffi.ERR_INVALID           # a q without its trace
    assert Lib.qd_plan_density(plan._h, src, H, 0, n, 0, 4, 2, 1000, 8, dst, None, 1, dst, H, None) == _ffi.ERR_INVALID
    assert Lib.qd_plan_density(plan._h, src, 9, 0, n, 0, 4, 2, 1000, 8, dst, None, 0, None, H, None) == _ffi.ERR_INVALID
    assert Lib.qd_plan_density(plan._h, src, H, 0, n, 0, 4, 2, 1000, 8, dst, None, 0, None, 9, None) == _ffi.ERR_INVALID
    assert Lib.qd_plan_density(plan._h, src, H, 0, n, plan.n_windows, 1, 2, 1000, 8, dst, None, 0, None, H, None) == _ffi.ERR_SHORT
    assert Lib.qd_plan_density(plan._h, src, H, 0, n, 5, 0, 2, 1000, 8, dst, None, 0, None, H, None) == 0      # no windows: nothing is touched
    assert (out == 77).all()
    got = plan.density(fsk, 3, 1000, 8, (0.5,), 5, 0)
    assert got[0].shape == (0, 64, 8) and got[1].shape == (1, 0, 64)
    # counts that need more than 1 GiB of workspace: refused before anything runs, and the message says what to do
    wide = engine.Plan(0, SR, 1 << 22, width=64, stride=1)
    assert wide.n_windows * 64 * 256 * 4 > 1 << 30
    rc = Lib.qd_plan_density(wide._h, src, H, 0, 1 << 22, 0, wide.n_windows, 1, 1000, 256, None, qa, 1, dst, H, None)
    assert rc == _ffi.ERR_UNSUPPORTED and b"spans of rows" in Lib.qd_last_error()
    assert (out == 77).all()
