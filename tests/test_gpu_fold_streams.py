"""The fold sinks on a caller's stream and from several threads (-m gpu).  Every fold takes a `stream`: accumulator initialisation,
band-table uploads, the planes' copies home and the workspace hand-over are ordered on it, and the results are complete on return.
Here that stream is a non-default torch.cuda.Stream whose producer is still pending when the fold is called, and the plan mutex and the
workspace pool are used from concurrent threads.  Every result is byte for byte the CPU twin's over the plan's own norms, which
test_gpu_fold_footprint's `world` holds to the oracle."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_gpu_bands import band_sets
from test_gpu_fold_footprint import SINKS, _lib, _plane_bytes, world  # noqa: F401  (world: the module-scoped fixture)
from test_gpu_picture import pages
from util import GUARD_BYTE, poison

pytestmark = pytest.mark.gpu

BALLAST_BYTES = 1 << 30
COPIES = 8
JOIN_SECONDS = 120


def param_of(sink, w, k=0):
    """one variant per sink (k picks another pool / grid / band set / page)"""
    pool = (16, 25, 3, w.n)[k % 4]
    sets = band_sets(w.W)
    return {"summarize": None, "pool": pool, "mean": pool, "power": pool, "spread": (pool, tuple(SINKS["spread"].dtypes) if k % 2 == 0 else ("std",)),
            "density": (pool, *((1000, 64), (1500, 1))[k % 2]),
            "bands": [("ragged", tuple(sets["ragged"])), ("k255", tuple(sets["k255"]))][k % 2],
            "picture": [(t, pages(w.engine, w.W, w.n)[t]) for t in ("clipped", "invisible")][k % 2]}[sink]


@pytest.fixture(scope="module")
def ballast():
    """two large device tensors: copies between them are the delay in front of the producer"""
    import torch
    pair = [torch.zeros(BALLAST_BYTES, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    yield pair
    del pair[:]
    torch.cuda.empty_cache()


def fold_on(w, sink, param, src, stream, device_out, reader=None):
    """the fold of the whole stream through the C entry point on `stream` (a torch stream or None) into exact-size planes pre-filled
    with 0xA5; returns the planes' bytes as they are ON RETURN: host planes as they stand, device planes read back on `reader`, a
    stream of its own that waits for nothing"""
    import torch
    ffi, _ = _lib()
    is_dev = hasattr(src, "data_ptr")
    specs = sink.planes(param, w.W, w.n)
    on_dev = device_out and not sink.host_only
    if on_dev:
        outs = {sp[0]: torch.full((_plane_bytes(sp),), GUARD_BYTE, dtype=torch.uint8, device="cuda") for sp in specs}
        ptr = {n: t.data_ptr() for n, t in outs.items()}
    else:
        outs = {sp[0]: np.full(_plane_bytes(sp), GUARD_BYTE, dtype=np.uint8) for sp in specs}
        ptr = {n: a.ctypes.data for n, a in outs.items()}
    sptr = C.c_void_p(src.data_ptr() if is_dev else src.ctypes.data)
    st = C.c_void_p(stream.cuda_stream) if stream is not None else None
    rc = sink.call(w.plan, (sptr, ffi.MEM_DEVICE if is_dev else ffi.MEM_HOST, 0, w.n_samples, 0, w.n), param, ptr,
                   ffi.MEM_DEVICE if on_dev else ffi.MEM_HOST, st)
    assert rc == 0, (sink.name, ffi.lib().qd_last_error())
    if not on_dev:
        return {n: a.copy() for n, a in outs.items()}
    with torch.cuda.stream(reader):
        got = {n: t.cpu().numpy() for n, t in outs.items()}
    return got


def same(got, ref, what):
    assert set(got) == set(ref), what
    for n in ref:
        assert got[n].tobytes() == np.ascontiguousarray(ref[n]).tobytes(), (what, n)
    return True


@pytest.mark.parametrize("chain", ["cf32_w128", "cascade_w16_s8"])
@pytest.mark.parametrize("sink", list(SINKS))
def test_fold_behind_a_pending_producer_on_a_side_stream(world, ballast, sink, chain):
    """The device source holds the 0x7FC00000 poison; on one non-default stream go COPIES device-to-device copies of 1 GiB, the copy
    of the true stream into the source, and an event.  The fold is called on that stream while the event is still pending (asserted:
    a producer that has finished proves nothing) and must give the twin of the TRUE stream, complete on return: the planes are read
    back on a third stream that waits for nothing.  Then a host source -> device planes on the same side stream.
    COPIES = 8 was the first count tried and it holds: on the MI355X the queued producer (the eight copies and the source's) takes
    3.56 ... 3.68 ms by the events, over all sixteen cases, against microseconds between the record and the query."""
    import torch
    w, s = world(chain), SINKS[sink]
    param = param_of(sink, w)
    ref = s.twin(w.engine, w.norms[:s.looked_at(param, w.W, w.n)], param)
    side, reader = torch.cuda.Stream(), torch.cuda.Stream()
    src = torch.from_numpy(poison(0, w.data.size, 0).copy()).cuda()
    true_dev = torch.from_numpy(w.data.copy()).cuda()
    t0, t1, ready = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t0.record(side)
        for _ in range(COPIES):
            ballast[1].copy_(ballast[0])
        src.copy_(true_dev)
        t1.record(side)
        ready.record(side)
        pending = not ready.query()
        got = fold_on(w, s, param, src, side, True, reader)
    assert pending, "the producer had finished before the fold was called: the case proves nothing"
    assert same(got, ref, (sink, chain, "device source"))
    side.synchronize()
    print("producer: %d copies of %d MiB, %.2f ms queued in front of the fold" % (COPIES, BALLAST_BYTES >> 20, t0.elapsed_time(t1)))
    assert t0.elapsed_time(t1) < 1000.0
    # host source -> device planes on the same side stream: the copies home and the ring's hand-back are complete on return
    with torch.cuda.stream(side):
        got = fold_on(w, s, param, w.data, side, True, reader)
    assert same(got, ref, (sink, chain, "host source"))
    with torch.cuda.stream(side):
        got = fold_on(w, s, param, w.data, side, False)
    assert same(got, ref, (sink, chain, "host source, host planes"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ concurrency

def _threads(jobs):
    """run the jobs (callables) on one thread each; join with a timeout and fail on it or on the first error; never retry"""
    errors = []

    def guarded(job):
        try:
            job()
        except BaseException as e:          # noqa: B036  (reported in the main thread)
            errors.append(repr(e))
    ts = [threading.Thread(target=guarded, args=(j,), daemon=True) for j in jobs]
    assert len(ts) <= 4
    for t in ts:
        t.start()
    for t in ts:
        t.join(JOIN_SECONDS)
    assert not any(t.is_alive() for t in ts), "a fold thread did not finish"
    assert not errors, errors


def _loop(w, dev, order, rounds, refs, k=0):
    """a thread's work: `rounds` times over the sinks of `order` on a side stream of its own"""
    import torch
    side, reader = torch.cuda.Stream(), torch.cuda.Stream()

    def job():
        with torch.cuda.stream(side):
            for r in range(rounds):
                for name in order:
                    param = param_of(name, w, k)
                    same(fold_on(w, SINKS[name], param, dev, side, True, reader), refs[(w.name, name, k)], (w.name, name, r))
                    if r == 0:
                        same(fold_on(w, SINKS[name], param, w.data, side, True, reader), refs[(w.name, name, k)], (w.name, name, "host"))
        side.synchronize()
    return job


def _refs(w, k):
    out = {}
    for name, s in SINKS.items():
        param = param_of(name, w, k)
        out[(w.name, name, k)] = s.twin(w.engine, w.norms[:s.looked_at(param, w.W, w.n)], param)
    return out


def test_two_threads_two_plans_two_streams(world):
    """the workspace pool's leases: each thread folds on its own plan and side stream, three times over all eight sinks"""
    import torch
    ws = [world("cf32_w128"), world("cs8_fir_w64_s16")]
    refs = {}
    for w in ws:
        refs.update(_refs(w, 0))
    devs = [torch.from_numpy(w.data.copy()).cuda() for w in ws]
    torch.cuda.synchronize()
    _threads([_loop(w, d, list(SINKS), 3, refs) for w, d in zip(ws, devs)])
    torch.cuda.synchronize()


def test_two_threads_one_plan_then_released_workspaces(world):
    """the plan mutex and the accumulators' re-initialisation between calls: two threads on ONE plan, the sinks in opposite orders and
    with different pools, grids, band sets and pages; then qd_release_workspaces and one fold of every sink again"""
    import torch
    w = world("cf32_w128")
    refs = {**_refs(w, 0), **_refs(w, 1)}
    dev = torch.from_numpy(w.data.copy()).cuda()
    torch.cuda.synchronize()
    _threads([_loop(w, dev, list(SINKS), 3, refs, 0), _loop(w, dev, list(SINKS)[::-1], 3, refs, 1)])
    torch.cuda.synchronize()
    ffi, L = _lib()
    ffi.check(L.qd_release_workspaces())
    side, reader = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        for name in SINKS:
            same(fold_on(w, SINKS[name], param_of(name, w, 1), dev, side, True, reader), refs[(w.name, name, 1)], (name, "after the release"))
    torch.cuda.synchronize()
