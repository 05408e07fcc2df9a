"""qd_plan_bursts on the GPU: the list, found and on_counts byte for byte against engine.bursts_of (the CPU twin) of the same plan's
qd_plan_run norms, which test_gpu_pool's `world` holds to the oracle; at every width where the walker's layout changes (several pieces in
a wave, a piece over several waves, column slabs) and in every kernel family; independent of batches, memory kinds, cap and call order;
planted streams against the integer referee of test_bursts_cpu; the short cascade, the refusals, the caller's stream, and the relation
to the mark sink.  Golden files only."""
import ctypes as C

import numpy as np
import pytest

import util
from test_bursts_cpu import BURST, ref_bursts
from test_gpu_cascade import PROBE, _data
from test_gpu_pool import FAMILIES, SR, WIDTHS, world  # noqa: F401  (world: the module-scoped fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32


def host(got):
    """(list BURST, found, on_counts uint64) of a Plan.bursts result of either kind"""
    import torch
    torch.cuda.synchronize()
    lst, found, counts = got
    if hasattr(lst, "cpu"):
        lst = np.ascontiguousarray(lst.cpu().numpy()).reshape(-1).view(BURST)
    if hasattr(counts, "cpu"):
        counts = counts.cpu().numpy().view(np.uint64)                     # a torch on_counts is int64: the same bits
    return lst, found, counts


def same(got, ref, what=None):
    assert got[1] == ref[1], (what, got[1], ref[1])
    assert got[0].dtype == BURST and got[0].tobytes() == ref[0].tobytes(), what
    assert got[2].dtype == np.uint64 and got[2].tobytes() == ref[2].tobytes(), what
    return True


def threshold_sets(norms):
    """the per-bin median (about half the cells on, many short runs) and the 0.9 quantile over all cells as one level (sparse, longer
    runs): taken from the norms themselves"""
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            median = np.nanmedian(norms, axis=0).astype(F32)              # a bin without a value: NaN, which masks it
    level = F32(np.nanquantile(norms.astype(np.float64), 0.9))
    return {"median": median, "q90": np.full(norms.shape[1], level, F32)}


@pytest.mark.parametrize("name", WIDTHS + FAMILIES)
def test_matches_the_twin_on_the_plans_norms(engine, world, name):
    plan, data, dev, norms, n, spec = world(name)
    W = spec[3]["width"]
    longest = 0
    for tag, thr in threshold_sets(norms).items():
        for min_len in (1, 3):
            ref = engine.bursts_of(norms, thr, min_len, cap=n * W)         # cannot overflow: a bin holds at most ceil(n / 2) bursts
            got = host(plan.bursts(dev, thr, min_len, cap=n * W, n_windows=n))
            assert same(got, ref, (tag, min_len))
            assert ref[1] > 0, (tag, min_len)
            longest = max(longest, int(ref[0]["length"].max()))
    assert longest >= 2                                                    # teeth


@pytest.mark.parametrize("name", ["cf32_w128", "cf32_w4", "shift_fir_w128", "cascade_w16_s8"])
def test_batch_seams_and_sources(engine, world, name):
    """chunk_bytes = 64 KiB: several batches, the last one ragged, on the host ring over its two streams; pageable, pinned and device
    sources; host and device outputs; twice on a plan.  That a run is open across the small plan's batch seams is asserted for cf32_w128
    only, whose 128 bins make it certain; the other cases take what their data holds, and test_planted_streams crosses every batch and
    piece seam by construction."""
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    W = kw["width"]
    small = engine.Plan(fmt, rate, n_samples, chunk_bytes=1 << 16, **kw)
    if name in ("cf32_w128", "cf32_w4"):
        cw = (1 << 16) // (W * 4)                                       # windows a batch holds
        assert n >= 3 * cw + 5
        n = 3 * cw + 5
        norms = norms[:n]
    if name == "cf32_w128":                                             # a run crosses every batch seam of the small plan
        on = np.abs(norms) >= threshold_sets(norms)["median"]
        assert all((on[k - 1] & on[k]).any() for k in (cw, 2 * cw, 3 * cw))
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    sets = threshold_sets(norms)
    refs = {}
    for tag, thr in sets.items():
        for min_len in (1, 3):
            refs[tag, min_len] = whole = engine.bursts_of(norms, thr, min_len, cap=n * W)
            kwargs = dict(min_len=min_len, cap=n * W, n_windows=n)
            for p in (plan, small):
                assert same(host(p.bursts(dev, thr, **kwargs)), whole, tag)                              # device -> device
                assert same(p.bursts(dev, thr, device_out=False, **kwargs), whole, tag)                  # device -> host
                assert same(p.bursts(data, thr, **kwargs), whole, tag)                                   # pageable -> host
                assert same(host(p.bursts(data, thr, device_out=True, **kwargs)), whole, tag)            # pageable -> device
                assert same(p.bursts(pin.array, thr, pinned=True, **kwargs), whole, tag)                 # pinned -> host
    # a second call on the same plan reuses the workspace: a larger result, a smaller one, and the first again
    a = small.bursts(data, sets["median"], 1, cap=n * W, n_windows=n)
    b = small.bursts(data, sets["q90"], 3, cap=n * W, n_windows=7)
    c = small.bursts(data, sets["median"], 1, cap=n * W, n_windows=n)
    assert a[1] > b[1] and same(a, refs["median", 1]) and same(b, engine.bursts_of(norms[:7], sets["q90"], 3)) and same(c, a)
    a = host(small.bursts(dev, sets["median"], 1, cap=n * W, n_windows=n))
    b = host(small.bursts(dev, sets["q90"], 3, cap=n * W, n_windows=7))
    assert same(a, refs["median", 1]) and same(b, engine.bursts_of(norms[:7], sets["q90"], 3))
    pin.close()


@pytest.mark.parametrize("name", ["cf32_w128", "cs8_fir_w64_s16", "cascade_w16_s8"])
def test_sub_range_from_a_slab(engine, world, name):
    import torch
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    bps = {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
    first, count = 2, n - 3
    a, cnt = plan.src_range(first, count)
    slab = data[a * bps:(a + cnt) * bps]
    part = norms[first:first + count]
    for tag, thr in threshold_sets(part).items():
        ref = engine.bursts_of(part, thr, 1, cap=count * kw["width"])     # records count from the range's first window
        assert ref[1] > 0 and int(ref[0]["first"].min()) == 0
        assert same(plan.bursts(slab, thr, 1, count * kw["width"], first, count, src_first=a), ref, tag)
        sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
        assert same(host(plan.bursts(sd, thr, 1, count * kw["width"], first, count, src_first=a)), ref, tag)


def planted_levels(n):
    """levels 1 ... 8 by window: runs of odd lengths co-prime to any power-of-two piece, then alternating windows, equal peaks inside a
    run, a +inf window and a NaN window; the lowest level is 1, so a bin with threshold 1 is on from end to end but for the NaN"""
    lengths = [1, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41]
    rng = np.random.default_rng(2024)
    v = np.empty(n, dtype=np.float64)
    i = k = 0
    while i < n:
        ln = min(lengths[k % len(lengths)], n - i)
        v[i:i + ln] = 1 + rng.integers(0, 8)
        if k % 3 == 0:                                                     # a run with a shape: its peak twice, the first one wins
            v[i:i + ln] = np.resize([3, 6, 4, 6, 2], ln)
        i += ln
        k += 1
    v[40:72] = np.resize([8, 1], 32)                                       # alternating cells, across a multiple of 16
    return v.astype(F32)


@pytest.mark.parametrize("W", [1, 4, 128, 2048])
def test_planted_streams(engine, W):
    """window i holds level v_i in every bin and bin b's threshold is 1 + b % 8 (the last bin of a wide window is masked), so bin b's
    runs are the runs of v >= 1 + b % 8: different in every bin, across every batch seam of the small plan and, bin 0 being on from end to
    end, across every piece seam of every launch.  Against the integer referee."""
    import torch
    cw = max((1 << 16) // (W * 4), 1)
    n = max(min(3 * cw + 5, 12_293), 120) if W > 1 else 20_000
    vals = planted_levels(n)
    bits = vals.view(np.uint32).copy()
    bits[n // 2] = util.PLANT_INF
    if W > 1:
        bits[n // 3] = util.PLANT_NAN                                      # W = 1 keeps its run over the whole range
    data = util.impulse_stream(bits, W)
    thr = (1 + np.arange(W) % 8).astype(F32)
    if W >= 128:
        thr[W - 1] = np.nan
    nb = np.broadcast_to(bits[:, None], (n, W))
    refs = {min_len: ref_bursts(nb, thr, min_len) for min_len in (1, 2)}
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    for chunk in (0, 1 << 16):
        plan = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, len(data) // 8, width=W, chunk_bytes=chunk)
        assert plan.complete_windows() >= n
        norms = plan.run_host(data, n_windows=n)
        keep = bits != util.PLANT_NAN
        assert (norms.view(np.uint32)[keep] == nb[keep]).all() and np.isnan(norms[~keep]).all()
        for min_len in (1, 2):
            ref = refs[min_len]
            assert same(plan.bursts(data, thr, min_len, cap=n * W, n_windows=n), ref, (chunk, min_len))
            assert same(host(plan.bursts(dev, thr, min_len, cap=n * W, n_windows=n)), ref, (chunk, min_len, "device"))
    ref = refs[1]
    lst = ref[0]
    if W == 1:
        assert ref[1] == 1 and lst[0]["first"] == 0 and lst[0]["length"] == n and lst[0]["peak"] == np.inf and lst[0]["peak_at"] == n // 2
    else:
        whole = lst[lst["bin"] == 0]
        assert whole["length"].tolist() == [n // 3, n - n // 3 - 1]                          # bin 0: the range, split by the NaN window
        twice = 0
        for r in lst[lst["bin"] == 1]:                                                       # equal peaks: the first window wins
            run = bits[int(r["first"]):int(r["first"] + r["length"])]
            assert int(r["peak_at"]) == int(r["first"]) + int(np.argmax(run)) and r["peak"].view(np.uint32) == run.max()
            twice += int((run == run.max()).sum() >= 2)
        assert twice > 0
        alt = lst[(lst["bin"] == min(7, W - 1)) & (lst["first"] >= 42) & (lst["first"] < 70)]
        assert alt.size == 14 and (alt["length"] == 1).all()                                 # alternating cells


def test_overflow_keeps_the_prefix_and_the_guards(engine, world):
    import torch
    plan, data, dev, norms, n, spec = world("shift_fir_w128")
    W = 128
    thr = threshold_sets(norms)["median"]
    full, found, counts = engine.bursts_of(norms, thr, 1, cap=n * W)
    assert found > 8
    got = plan.bursts(data, thr, 1, cap=0, n_windows=n)                                      # cap 0 and no list: counts only
    assert got[0].size == 0 and got[1] == found and got[2].tobytes() == counts.tobytes()
    got = host(plan.bursts(dev, thr, 1, cap=0, n_windows=n))
    assert got[0].size == 0 and got[1] == found and got[2].tobytes() == counts.tobytes()
    for cap in (1, found - 1):
        k = min(cap, found)
        buf = np.full((cap + 3) * 32, util.GUARD_BYTE, dtype=np.uint8)
        cbuf = np.full(W + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        got = plan.bursts(data, thr, 1, cap=cap, n_windows=n, out=buf[32:32 + cap * 32].view(BURST), counts_out=cbuf[1:W + 1])
        assert got[1] == found and buf[32:32 + k * 32].tobytes() == full[:k].tobytes()
        assert (buf[:32] == util.GUARD_BYTE).all() and (buf[32 + k * 32:] == util.GUARD_BYTE).all()
        assert cbuf[1:W + 1].tobytes() == counts.tobytes() and cbuf[0] == cbuf[W + 1] == 0xA5A5A5A5A5A5A5A5
        # a list that is given sets cap when none is, and bounds the one that is
        buf[:] = util.GUARD_BYTE
        got = plan.bursts(data, thr, 1, n_windows=n, out=buf[32:32 + cap * 32].view(BURST))
        assert got[1] == found and got[0].size == k and buf[32:32 + k * 32].tobytes() == full[:k].tobytes()
        assert (buf[:32] == util.GUARD_BYTE).all() and (buf[32 + k * 32:] == util.GUARD_BYTE).all()
        with pytest.raises(ValueError):
            plan.bursts(data, thr, 1, cap=cap + 1, n_windows=n, out=buf[32:32 + cap * 32].view(BURST))
        with pytest.raises(ValueError):
            plan.bursts(data, thr, 1, cap=cap, n_windows=n, out=buf[32:32 + cap * 32].view(BURST), counts_out=cbuf[1:W])
        assert (buf == util.GUARD_BYTE).sum() >= 32 + 64
        for lead in (32, 40):                                                                # device lists at and off a multiple of 16
            t = torch.full((lead + (cap + 2) * 32,), util.GUARD_BYTE, dtype=torch.uint8, device="cuda")
            ct = torch.full((W + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            got = plan.bursts(dev, thr, 1, cap=cap, n_windows=n, out=t[lead:lead + cap * 32], counts_out=ct[1:W + 1])
            torch.cuda.synchronize()
            h, hc = t.cpu().numpy(), ct.cpu().numpy().view(np.uint64)
            assert got[1] == found and h[lead:lead + k * 32].tobytes() == full[:k].tobytes()
            assert (h[:lead] == util.GUARD_BYTE).all() and (h[lead + k * 32:] == util.GUARD_BYTE).all()
            assert hc[1:W + 1].tobytes() == counts.tobytes() and hc[0] == hc[W + 1] == 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("name", ["cf32_w4", "cf32_w128"])
def test_cap_ladder(engine, world, name):
    """cap at the wave, round and off-by-one boundaries of the ballot rank (63 ... 65, 255 ... 257), at found and past it; at W = 4
    several pieces share a wave.  The list is the twin's first min(found, cap) records byte for byte, found is the twin's, and the guard
    bytes in front of and behind the list are intact.  A host source into a host list and a device source into a device list, where
    the kernels store."""
    import torch
    plan, data, dev, norms, n, spec = world(name)
    W = spec[3]["width"]
    thr = threshold_sets(norms)["median"]
    full, found, _ = engine.bursts_of(norms, thr, 1, cap=n * W)
    assert found > 257 and full.size == found                              # every cap of the ladder cuts the list
    for cap in (63, 64, 65, 255, 256, 257, found, found + 1):
        k = min(cap, found)
        buf = np.full((cap + 2) * 32, util.GUARD_BYTE, dtype=np.uint8)
        got = plan.bursts(data, thr, 1, cap=cap, n_windows=n, out=buf[32:32 + cap * 32].view(BURST))
        t = torch.full(((cap + 2) * 32,), util.GUARD_BYTE, dtype=torch.uint8, device="cuda")
        got_d = plan.bursts(dev, thr, 1, cap=cap, n_windows=n, out=t[32:32 + cap * 32])
        torch.cuda.synchronize()
        for g, h in ((got, buf), (got_d, t.cpu().numpy())):
            assert g[1] == found and g[0].shape[0] == k, cap
            assert h[32:32 + k * 32].tobytes() == full[:k].tobytes(), cap
            assert (h[:32] == util.GUARD_BYTE).all() and (h[32 + k * 32:] == util.GUARD_BYTE).all(), cap


def test_covered_windows_are_the_mark_sinks(engine, cupboard):
    """nofir_w4_s2 on the OOK file, which has no NaN: with every threshold 0.001 and min_len 1 a window is covered by a burst iff one of
    its norms is >= 0.001, which is when the mark sink under -range 0.001:0.01 writes 1"""
    n_samples = len(cupboard) // 8
    kw = dict(width=4, stride=2)
    plan = engine.Plan(0, 400, n_samples, **kw)
    marks = engine.Plan(0, 400, n_samples, epilogue=engine.EPI_MARK_U8, rng=(0.001, 0.01), **kw).run_host(cupboard).reshape(-1)
    n = plan.complete_windows()
    assert not np.isnan(plan.run_host(cupboard, n_windows=n)).any()
    lst, found, counts = plan.bursts(cupboard, F32(0.001), 1, cap=n * 4, n_windows=n)
    assert found == lst.size > 0
    covered = np.zeros(n, dtype=np.uint8)
    for r in lst:
        covered[int(r["first"]):int(r["first"] + r["length"])] = 1
    assert 0 < covered.sum() < n and covered.tobytes() == (marks[:n] != 0).astype(np.uint8).tobytes()


def test_short_cascade_lists_its_complete_windows(engine):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    thr = threshold_sets(norms)["median"]
    thr[0] = 0                                                                               # bin 0 is on to the end: a run to close there
    assert not np.isnan(norms).any()
    for first in (0, done - 1, done):
        with pytest.raises(engine.QuadrsError) as e:
            plan.bursts(data, thr, first_window=first, cap=total * 4)
        assert e.value.code == engine._ffi.ERR_SHORT
        if first < done:
            ref = engine.bursts_of(norms[first:done], thr, 1, cap=total * 4)                 # the open runs close at the last complete window
        else:
            ref = (np.zeros(0, BURST), 0, np.zeros(4, np.uint64))
        assert same(e.value.partial, ref, first)
    ref = engine.bursts_of(norms, thr, 1)
    assert (ref[0]["first"] + ref[0]["length"] == done).any()                                # a run was open at the end


def test_refusals_leave_the_outputs_untouched(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8
    L = _ffi.lib()
    buf = np.frombuffer(fsk, dtype=np.uint8)
    src = buf.ctypes.data_as(C.c_void_p)
    W = 64
    lst = np.full(8 * 32, 0x5A, np.uint8)
    counts = np.full(W, 77, np.uint64)
    found = C.c_uint64(99)
    ok = np.zeros(W, F32)                                                                    # every cell is on

    def call(plan, thr=ok, min_len=1, lp=lst.ctypes.data_as(C.c_void_p), cap=8, fp=C.byref(found), first=0, count=4, src_mem=_ffi.MEM_HOST,
             out_mem=_ffi.MEM_HOST):
        t = None if thr is None else np.ascontiguousarray(thr, F32)
        return L.qd_plan_bursts(plan._h, src, src_mem, 0, n, first, count, None if t is None else t.ctypes.data_as(C.c_void_p), min_len, lp, cap, fp,
                                counts.ctypes.data_as(C.c_void_p), out_mem, None)
    for epi in (engine.EPI_GLYPH_U8, engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
        assert call(engine.Plan(0, SR, n, width=W, epilogue=epi)) == _ffi.ERR_INVALID
    assert call(engine.Plan(0, SR, n, width=W, shard_devices=[0, 0])) == _ffi.ERR_UNSUPPORTED
    assert b"seam" in L.qd_last_error()
    plan = engine.Plan(0, SR, n, width=W)
    for bad in (-1.0, -0.0, -np.inf):
        t = ok.copy()
        t[W - 1] = bad
        assert call(plan, thr=t) == _ffi.ERR_INVALID, bad
    assert call(plan, thr=None) == _ffi.ERR_INVALID and call(plan, fp=None) == _ffi.ERR_INVALID
    assert call(plan, min_len=0) == _ffi.ERR_INVALID and call(plan, lp=None) == _ffi.ERR_INVALID
    assert call(plan, src_mem=9) == _ffi.ERR_INVALID and call(plan, out_mem=9) == _ffi.ERR_INVALID
    assert call(plan, first=0, count=plan.n_windows + 1) == _ffi.ERR_SHORT
    assert call(plan, first=plan.n_windows, count=1) == _ffi.ERR_SHORT
    assert call(plan, cap=(1 << 25) + 1) == _ffi.ERR_UNSUPPORTED                             # a list workspace above 1 GiB
    assert (lst == 0x5A).all() and (counts == 77).all() and found.value == 99
    assert call(plan, first=5, count=0) == 0                                                 # no windows: nothing found, the list untouched
    assert (lst == 0x5A).all() and not counts.any() and found.value == 0
    counts[:] = 77
    assert call(plan) == 0 and found.value == W and (counts == 4).all()                      # every bin's run closes at the range's end
    assert lst.view(BURST)["bin"].tolist() == list(range(8)) and (lst.view(BURST)["length"] == 4).all()
    with pytest.raises(ValueError):
        plan.bursts(fsk, np.zeros(W + 1, F32))
    with pytest.raises(engine.QuadrsError) as e:
        plan.bursts(fsk, -1.0)
    assert e.value.code == _ffi.ERR_INVALID


def test_stats_are_unchanged_by_a_fold(engine, fsk):
    n = len(fsk) // 8
    plan = engine.Plan(0, SR, n, width=64)
    plan.run_host(fsk)
    before = plan.stats()
    fields = [f for f, _ in before._fields_]
    assert before.chunks >= 1 and before.bytes_h2d > 0
    assert plan.bursts(fsk, 0.0)[1] > 0
    after = plan.stats()
    assert [getattr(after, f) for f in fields] == [getattr(before, f) for f in fields]


def test_on_the_callers_stream_behind_a_pending_producer(engine, world):
    """The device source holds NaN poison; on a non-default stream go copies of 1 GiB, then the copy of the true stream into the source.
    The call runs on that stream while the producer is still pending (asserted) and must list the bursts of the TRUE stream, complete on
    return; then a host source on the same side stream."""
    import torch
    plan, data, dev, norms, n, spec = world("cf32_w128")
    thr = threshold_sets(norms)["median"]
    ref = engine.bursts_of(norms, thr, 1, cap=n * 128)
    side = torch.cuda.Stream()
    ballast = [torch.zeros(1 << 30, dtype=torch.uint8, device="cuda") for _ in range(2)]
    src = torch.from_numpy(util.poison(0, len(data), 0).copy()).cuda()
    ready = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            ballast[1].copy_(ballast[0])
        src.copy_(dev)
        ready.record(side)
        pending = not ready.query()
        got = plan.bursts(src, thr, 1, cap=n * 128, n_windows=n, device_out=False)
        assert pending, "the producer had finished before the call: the case proves nothing"
        assert same(got, ref, "device source")
        assert same(plan.bursts(data, thr, 1, cap=n * 128, n_windows=n), ref, "host source")
        lst, found, counts = plan.bursts(src, thr, 1, cap=n * 128, n_windows=n)
    side.synchronize()
    assert same(host((lst, found, counts)), ref, "device list")
    del ballast
    torch.cuda.empty_cache()
