"""qd_plan_emissions on the GPU: the list and found byte for byte against engine.emissions_of (the CPU twin, which test_emissions_cpu
holds to a flood fill) of the same plan's qd_plan_run norms, which test_gpu_pool's `world` holds to the oracle; at every width where a
tile's layout changes and in every kernel family; independent of batches, spans, memory kinds, cap and call order; planted streams
against the flood-fill referee of test_emissions_cpu; a stream longer than one span; the relation to the burst list; the short
cascade, the refusals and the caller's stream.  Golden files only."""
import ctypes as C

import numpy as np
import pytest

import util
from test_emissions_cpu import EMISSION, ref_emissions
from test_gpu_cascade import PROBE, _data
from test_gpu_pool import FAMILIES, SR, WIDTHS, world  # noqa: F401  (world: the module-scoped fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
SPAN_CELLS = 1 << 20                                                       # kEmissionsSpanCells: a span holds at most this many cells


def host(got):
    """(list EMISSION, found) of a Plan.emissions result of either kind"""
    import torch
    torch.cuda.synchronize()
    lst, found = got
    if hasattr(lst, "cpu"):
        lst = np.ascontiguousarray(lst.cpu().numpy()).reshape(-1).view(EMISSION)
    return lst, found


def same(got, ref, what=None):
    assert got[1] == ref[1], (what, got[1], ref[1])
    assert got[0].dtype == EMISSION
    if got[0].tobytes() != ref[0].tobytes():
        k = next(i for i in range(len(ref[0])) if got[0][i:i + 1].tobytes() != ref[0][i:i + 1].tobytes())
        raise AssertionError("%s: record %d: got %s, expected %s" % (what, k, got[0][k], ref[0][k]))
    return True


def threshold_sets(norms):
    """the per-bin median (about half the cells on: the labelling's hard case) and the 0.9 quantile over all cells as one level"""
    import warnings
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        median = np.nanmedian(norms, axis=0).astype(F32)                   # a bin without a value: NaN, which masks it
    level = F32(np.nanquantile(norms.astype(np.float64), 0.9))
    return {"median": median, "q90": np.full(norms.shape[1], level, F32)}


FILTERS = ((1, 1), (3, 1), (1, 4))


@pytest.mark.parametrize("name", WIDTHS + FAMILIES)
def test_matches_the_twin_on_the_plans_norms(engine, world, name):
    plan, data, dev, norms, n, spec = world(name)
    W = spec[3]["width"]
    wide = False
    for tag, thr in threshold_sets(norms).items():
        for min_len, min_cells in FILTERS:
            ref = engine.emissions_of(norms, thr, min_len, min_cells, cap=n * W)
            got = host(plan.emissions(dev, thr, min_len, min_cells, cap=n * W, n_windows=n))
            assert same(got, ref, (tag, min_len, min_cells))
            assert ref[1] > 0, (tag, min_len, min_cells)
            wide = wide or bool(((ref[0]["hi"] > ref[0]["lo"]) & (ref[0]["last"] > ref[0]["first"])).any())
    assert wide or W < 4                                                   # teeth: an emission over several bins and several windows


@pytest.mark.parametrize("name", ["cf32_w128", "cf32_w4", "shift_fir_w128", "cascade_w16_s8"])
def test_batch_seams_and_sources(engine, world, name):
    """chunk_bytes = 64 KiB: several batches, the last one ragged, on the host ring over its two streams; pageable, pinned and device
    sources; host and device lists; twice and three times on a plan.  That an emission crosses every batch seam of the small plan is
    asserted for cf32_w128, whose 128 bins make it certain."""
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    W = kw["width"]
    small = engine.Plan(fmt, rate, n_samples, chunk_bytes=1 << 16, **kw)
    if name in ("cf32_w128", "cf32_w4"):
        cw = (1 << 16) // (W * 4)                                       # windows a batch holds
        assert n >= 3 * cw + 5
        n = 3 * cw + 5
        norms = norms[:n]
    if name == "cf32_w128":
        on = np.abs(norms) >= threshold_sets(norms)["median"]
        assert all((on[k - 1] & on[k]).any() for k in (cw, 2 * cw, 3 * cw))
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    sets = threshold_sets(norms)
    refs = {}
    for tag, thr in sets.items():
        for min_len, min_cells in ((1, 1), (3, 2)):
            refs[tag, min_len] = whole = engine.emissions_of(norms, thr, min_len, min_cells, cap=n * W)
            kwargs = dict(min_len=min_len, min_cells=min_cells, cap=n * W, n_windows=n)
            for p in (plan, small):
                assert same(host(p.emissions(dev, thr, **kwargs)), whole, tag)                              # device -> device
                assert same(p.emissions(dev, thr, device_out=False, **kwargs), whole, tag)                  # device -> host
                assert same(p.emissions(data, thr, **kwargs), whole, tag)                                   # pageable -> host
                assert same(host(p.emissions(data, thr, device_out=True, **kwargs)), whole, tag)            # pageable -> device
                assert same(p.emissions(pin.array, thr, pinned=True, **kwargs), whole, tag)                 # pinned -> host
    # a second and a third call on the same plan reuse the workspace: a larger result, a smaller one, and the first again
    a = small.emissions(data, sets["median"], cap=n * W, n_windows=n)
    b = small.emissions(data, sets["q90"], 3, 2, cap=n * W, n_windows=7)
    c = small.emissions(data, sets["median"], cap=n * W, n_windows=n)
    assert a[1] > b[1] and same(a, refs["median", 1]) and same(b, engine.emissions_of(norms[:7], sets["q90"], 3, 2)) and same(c, a)
    a = host(small.emissions(dev, sets["median"], cap=n * W, n_windows=n))
    b = host(small.emissions(dev, sets["q90"], 3, 2, cap=n * W, n_windows=7))
    assert same(a, refs["median", 1]) and same(b, engine.emissions_of(norms[:7], sets["q90"], 3, 2))
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
        ref = engine.emissions_of(part, thr, cap=count * kw["width"])      # records count from the range's first window
        assert ref[1] > 0 and int(ref[0]["first"].min()) == 0
        assert same(plan.emissions(slab, thr, 1, 1, count * kw["width"], first, count, src_first=a), ref, tag)
        sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
        assert same(host(plan.emissions(sd, thr, 1, 1, count * kw["width"], first, count, src_first=a)), ref, tag)


PLANTED_THRESHOLDS = np.array([1, 5, 2, 8, 1, 5, 2, 9], F32)


def planted_bits(n, with_inf=True):
    """levels 1 ... 7 by window in runs of odd lengths, equal peaks twice inside every third run; a single 8 at window 2n/3, a NaN window
    at n/3 and (with_inf) +inf at n/2; windows 4 ... 6 hold 1, 2, 1"""
    lengths = [1, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41]
    rng = np.random.default_rng(2025)
    v = np.empty(n, dtype=np.float64)
    i = k = 0
    while i < n:
        ln = min(lengths[k % len(lengths)], n - i)
        v[i:i + ln] = 1 + rng.integers(0, 7)
        if k % 3 == 0:                                                     # a run with a shape: its peak twice, the first one wins
            v[i:i + ln] = np.resize([3, 6, 4, 6, 2], ln)
        i += ln
        k += 1
    v[4:7] = [1, 2, 1]                                                     # the bins of threshold 2 alone for one window: single cells
    bits = v.astype(F32).view(np.uint32).copy()
    bits[2 * n // 3] = F32(8).view(np.uint32)
    bits[n // 3] = util.PLANT_NAN
    if with_inf:
        bits[n // 2] = util.PLANT_INF
    return bits


def planted_case(n, W, with_inf=True):
    bits = planted_bits(n, with_inf)
    thr = PLANTED_THRESHOLDS[np.arange(W) % 8].copy()
    return bits, thr, np.broadcast_to(bits[:, None], (n, W))


def planted_teeth(lst, bits, thr, n, W, cw, with_inf):
    """what the planted design holds by construction, asserted on the referee's list"""
    nan_at, inf_at, eight_at = n // 3, n // 2, 2 * n // 3
    # bins of threshold 1 are on in every window but the NaN's: open from the window behind it to the range's end, cut there
    tail = lst[(lst["first"] == nan_at + 1) & (lst["last"] == n - 1)]
    assert tail.size >= 1 and (tail["flags"] & 2).all()
    seams = [k for k in range(cw, n, cw) if nan_at + 1 < k <= n - 1]
    assert len(seams) >= 2                                                 # ... across batch seams of the small plan
    # the emissions that the NaN window ends: all in the window before it, in the list's order by end_bin
    ended = lst[lst["last"] == nan_at - 1]
    at = np.flatnonzero(lst["last"] == nan_at - 1)
    assert (np.diff(at) == 1).all() and (np.diff(ended["end_bin"].astype(np.int64)) > 0).all()
    assert ended.size >= max(1, (W + 3) // 4)                              # every bin of threshold 1 ends an emission of its own there
    if W >= 8:
        # the columns of threshold 1 are apart until a window turns the bins between them on: the whole row at +inf, or bins 0 ... 6 of
        # every eight at the level 8, where pairs that were open since the NaN window, over at least two batch seams, merge
        merge_at = inf_at if with_inf else eight_at
        assert len([k for k in seams if k <= merge_at]) >= (1 if with_inf else 2)
        merged = lst[(lst["first"] == nan_at + 1) & (lst["last"] >= merge_at)]
        assert merged.size >= 1 and (merged["hi"] - merged["lo"] >= 4).all()
        if not with_inf:
            assert merged.size == (W + 7) // 8 and (merged["lo"] % 8 == 0).all()      # bin 7 of every eight (threshold 9) keeps the groups apart
        before = lst[(lst["first"] == 0) & (lst["last"] == nan_at - 1) & (lst["lo"] % 4 == 0)]
        assert (before["hi"] - before["lo"] < 4).all() and before.size >= W // 4       # before that, no two of those columns had met
    if W > 1:
        assert (lst["cells"] == 1).any()                                   # single-cell emissions
    if with_inf:
        # the +inf window is a whole row of equal peaks: the earliest (window, bin) wins
        top = lst[lst["peak"] == np.inf]
        assert top.size == 1 and int(top["peak_at"][0]) == inf_at and int(top["peak_bin"][0]) == int(top["lo"][0]) == 0 and int(top["hi"][0]) == W - 1
    # equal peaks inside an emission whose lowest bin has threshold 1 (on at every level): the first window that attains the peak wins,
    # at the emission's lowest bin
    tied = 0
    for r in lst[(lst["lo"] % 4 == 0) & (lst["last"] > lst["first"])][:200]:
        run = bits[int(r["first"]):int(r["last"]) + 1]
        assert int(r["peak_at"]) == int(r["first"]) + int(np.argmax(run)) and r["peak"].view(np.uint32) == run.max() and r["peak_bin"] == r["lo"]
        tied += int((run == run.max()).sum() >= 2)
    assert tied > 0


@pytest.mark.parametrize("W,with_inf", [(1, True), (4, True), (128, True), (128, False), (2048, True)])
def test_planted_streams(engine, W, with_inf):
    """window i holds level v_i in every bin and the thresholds repeat [1, 5, 2, 8, 1, 5, 2, 9] over the bins.  Against the flood-fill
    referee, with the batch seams of a 64 KiB plan and in one batch.  With the +inf window in front of the 8 window the whole row is on
    there, so that is where the open columns merge; the case without +inf is the one where they merge at the 8 window."""
    import torch
    cw = max((1 << 16) // (W * 4), 1)
    n = max(6 * cw + 5, 120)
    bits, thr, nb = planted_case(n, W, with_inf)
    data = util.impulse_stream(bits, W)
    ref = ref_emissions(nb, thr)[:2]
    planted_teeth(ref[0], bits, thr, n, W, cw, with_inf)
    refs = {(1, 1): ref, (2, 3): ref_emissions(nb, thr, 2, 3)[:2]}
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    for chunk in (0, 1 << 16):
        plan = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, len(data) // 8, width=W, chunk_bytes=chunk)
        assert plan.complete_windows() >= n
        norms = plan.run_host(data, n_windows=n)
        keep = bits != util.PLANT_NAN
        assert (norms.view(np.uint32)[keep] == nb[keep]).all() and np.isnan(norms[~keep]).all()
        for (min_len, min_cells), r in refs.items():
            assert same(plan.emissions(data, thr, min_len, min_cells, cap=n * W, n_windows=n), r, (chunk, min_len, min_cells))
            assert same(host(plan.emissions(dev, thr, min_len, min_cells, cap=n * W, n_windows=n)), r, (chunk, min_len, min_cells, "device"))


def test_a_stream_longer_than_one_span(engine):
    """W = 2048 and 1436 windows in one batch (chunk_bytes = 0: 64 MiB of norms a batch): spans of 512 windows, so two span seams and a
    ragged last span, 23 MiB of input; the first seam lies between the NaN window and the +inf window, where the columns are still
    apart.  The planted design again; its 2.9 million cells are beyond a flood fill in Python, so the list is held to the CPU twin,
    which test_emissions_cpu holds to the flood fill, and to the design's teeth."""
    import torch
    W = 2048
    span = SPAN_CELLS // W
    n = 3 * span - 100
    bits, thr, nb = planted_case(n, W)
    data = util.impulse_stream(bits, W)
    assert len(data) <= 32 << 20
    plan = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, len(data) // 8, width=W, chunk_bytes=0)
    assert plan.complete_windows() >= n
    ref = engine.emissions_of(nb.view(F32), thr, cap=1 << 20)
    assert ref[1] < 1 << 20
    planted_teeth(ref[0], bits, thr, n, W, span, True)                     # the seams counted there are the span seams
    assert same(plan.emissions(data, thr, cap=1 << 20, n_windows=n), ref, "host")
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    assert same(host(plan.emissions(dev, thr, cap=1 << 20, n_windows=n)), ref, "device")
    ref = engine.emissions_of(nb.view(F32), thr, 3, 5, cap=1 << 20)
    assert same(host(plan.emissions(dev, thr, 3, 5, cap=1 << 20, n_windows=n)), ref, "filtered")


def test_overflow_keeps_the_prefix_and_the_guards(engine, world):
    import torch
    plan, data, dev, norms, n, spec = world("shift_fir_w128")
    W = 128
    thr = threshold_sets(norms)["median"]
    full, found = engine.emissions_of(norms, thr, cap=n * W)
    assert found > 8
    got = plan.emissions(data, thr, cap=0, n_windows=n)                                      # cap 0 and no list: counts only
    assert got[0].size == 0 and got[1] == found
    got = host(plan.emissions(dev, thr, cap=0, n_windows=n))
    assert got[0].size == 0 and got[1] == found
    for cap in (1, found - 1):
        k = min(cap, found)
        buf = np.full((cap + 3) * 56, util.GUARD_BYTE, dtype=np.uint8)
        got = plan.emissions(data, thr, cap=cap, n_windows=n, out=buf[56:56 + cap * 56].view(EMISSION))
        assert got[1] == found and buf[56:56 + k * 56].tobytes() == full[:k].tobytes()
        assert (buf[:56] == util.GUARD_BYTE).all() and (buf[56 + k * 56:] == util.GUARD_BYTE).all()
        # a list that is given sets cap when none is, and bounds the one that is
        buf[:] = util.GUARD_BYTE
        got = plan.emissions(data, thr, n_windows=n, out=buf[56:56 + cap * 56].view(EMISSION))
        assert got[1] == found and got[0].size == k and buf[56:56 + k * 56].tobytes() == full[:k].tobytes()
        assert (buf[:56] == util.GUARD_BYTE).all() and (buf[56 + k * 56:] == util.GUARD_BYTE).all()
        with pytest.raises(ValueError):
            plan.emissions(data, thr, cap=cap + 1, n_windows=n, out=buf[56:56 + cap * 56].view(EMISSION))
        for lead in (64, 56):                                                                # device lists at and off a multiple of 16
            t = torch.full((lead + (cap + 2) * 56,), util.GUARD_BYTE, dtype=torch.uint8, device="cuda")
            got = plan.emissions(dev, thr, cap=cap, n_windows=n, out=t[lead:lead + cap * 56])
            torch.cuda.synchronize()
            h = t.cpu().numpy()
            assert got[1] == found and h[lead:lead + k * 56].tobytes() == full[:k].tobytes()
            assert (h[:lead] == util.GUARD_BYTE).all() and (h[lead + k * 56:] == util.GUARD_BYTE).all()
        for lead in (64, 56):                                                                # host lists at and off a multiple of 16
            hbuf = np.full(lead + (cap + 2) * 56, util.GUARD_BYTE, dtype=np.uint8)
            got = plan.emissions(dev, thr, cap=cap, n_windows=n, out=hbuf[lead:lead + cap * 56].view(EMISSION))
            assert got[1] == found and hbuf[lead:lead + k * 56].tobytes() == full[:k].tobytes()
            assert (hbuf[:lead] == util.GUARD_BYTE).all() and (hbuf[lead + k * 56:] == util.GUARD_BYTE).all()


@pytest.mark.parametrize("name", ["cf32_w4", "cf32_w128"])
def test_cap_ladder(engine, world, name):
    """cap at the wave, round and off-by-one boundaries of the ballot rank every record passes through (63 ... 65, 255 ... 257), at found
    and past it: the list is the twin's first min(found, cap) records byte for byte, found is the twin's, and the guard bytes in front of
    and behind the list are intact.  A host source into a host list and a device source into a device list, where the kernels store."""
    import torch
    plan, data, dev, norms, n, spec = world(name)
    W = spec[3]["width"]
    thr = threshold_sets(norms)["median"]
    full, found = engine.emissions_of(norms, thr, cap=n * W)
    assert found > 257 and full.size == found                              # every cap of the ladder cuts the list
    for cap in (63, 64, 65, 255, 256, 257, found, found + 1):
        k = min(cap, found)
        buf = np.full((cap + 2) * 56, util.GUARD_BYTE, dtype=np.uint8)
        got = plan.emissions(data, thr, cap=cap, n_windows=n, out=buf[56:56 + cap * 56].view(EMISSION))
        t = torch.full(((cap + 2) * 56,), util.GUARD_BYTE, dtype=torch.uint8, device="cuda")
        got_d = plan.emissions(dev, thr, cap=cap, n_windows=n, out=t[56:56 + cap * 56])
        torch.cuda.synchronize()
        for g, h in ((got, buf), (got_d, t.cpu().numpy())):
            assert g[1] == found and g[0].shape[0] == k, cap
            assert h[56:56 + k * 56].tobytes() == full[:k].tobytes(), cap
            assert (h[:56] == util.GUARD_BYTE).all() and (h[56 + k * 56:] == util.GUARD_BYTE).all(), cap


def test_relation_to_the_burst_list(engine, world):
    """min_len = min_cells = 1: every on cell lies in exactly one emission, so the cells of the list sum to the burst list's on_counts;
    at W = 1 an emission is a burst, field for field"""
    plan, data, dev, norms, n, spec = world("cf32_w128")
    for tag, thr in threshold_sets(norms).items():
        lst, found = plan.emissions(data, thr, cap=n * 128, n_windows=n)
        _, _, counts = plan.bursts(data, thr, 1, cap=0, n_windows=n)
        assert found == lst.size and int(lst["cells"].sum()) == int(counts.sum()) > 0, tag
    plan, data, dev, norms, n, spec = world("cf32_w1")
    thr = threshold_sets(norms)["median"]
    lst, found = plan.emissions(data, thr, 2, 1, cap=n, n_windows=n)
    bl, bfound, _ = plan.bursts(data, thr, 2, cap=n, n_windows=n)
    assert found == bfound > 0
    assert lst["first"].tolist() == bl["first"].tolist() and (lst["last"] - lst["first"] + 1).tolist() == bl["length"].tolist()
    assert lst["cells"].tolist() == bl["length"].tolist() and lst["peak_at"].tolist() == bl["peak_at"].tolist()
    assert lst["peak"].tobytes() == bl["peak"].tobytes() and not lst["lo"].any() and not lst["hi"].any() and not lst["end_bin"].any() and not lst["peak_bin"].any()


def test_short_cascade_lists_its_complete_windows(engine):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    thr = threshold_sets(norms)["median"]
    thr[0] = 0                                                                               # bin 0 is on to the end: an emission to close there
    assert not np.isnan(norms).any()
    for first in (0, done - 1, done):
        with pytest.raises(engine.QuadrsError) as e:
            plan.emissions(data, thr, first_window=first, cap=total * 4)
        assert e.value.code == engine._ffi.ERR_SHORT
        if first < done:
            ref = engine.emissions_of(norms[first:done], thr, cap=total * 4)                 # what is open closes at the last complete window
        else:
            ref = (np.zeros(0, EMISSION), 0)
        assert same(e.value.partial, ref, first)
    ref = engine.emissions_of(norms, thr)
    assert ((ref[0]["last"] == done - 1) & (ref[0]["flags"] & 2 != 0)).any()                 # an emission was open at the end


def test_refusals_leave_the_outputs_untouched(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8
    L = _ffi.lib()
    buf = np.frombuffer(fsk, dtype=np.uint8)
    src = buf.ctypes.data_as(C.c_void_p)
    W = 64
    lst = np.full(8 * 56, 0x5A, np.uint8)
    found = C.c_uint64(99)
    ok = np.zeros(W, F32)                                                                    # every cell is on

    def call(plan, thr=ok, min_len=1, min_cells=1, lp=lst.ctypes.data_as(C.c_void_p), cap=8, fp=C.byref(found), first=0, count=4, src_mem=_ffi.MEM_HOST,
             out_mem=_ffi.MEM_HOST):
        t = None if thr is None else np.ascontiguousarray(thr, F32)
        return L.qd_plan_emissions(plan._h, src, src_mem, 0, n, first, count, None if t is None else t.ctypes.data_as(C.c_void_p), min_len, min_cells,
                                   lp, cap, fp, out_mem, None)
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
    assert call(plan, min_len=0) == _ffi.ERR_INVALID and call(plan, min_cells=0) == _ffi.ERR_INVALID and call(plan, lp=None) == _ffi.ERR_INVALID
    assert call(plan, src_mem=9) == _ffi.ERR_INVALID and call(plan, out_mem=9) == _ffi.ERR_INVALID
    assert call(plan, first=0, count=plan.n_windows + 1) == _ffi.ERR_SHORT
    assert call(plan, first=plan.n_windows, count=1) == _ffi.ERR_SHORT
    assert call(plan, cap=(1 << 30) // 56 + 1) == _ffi.ERR_UNSUPPORTED                       # a list workspace above 1 GiB
    assert (lst == 0x5A).all() and found.value == 99
    assert call(plan, first=5, count=0) == 0                                                 # no windows: nothing found, the list untouched
    assert (lst == 0x5A).all() and found.value == 0
    assert call(plan) == 0 and found.value == 1                                              # every cell is on: one emission, cut at both ends
    rec = lst[:56].view(EMISSION)[0]
    assert (int(rec["first"]), int(rec["last"]), int(rec["cells"]), int(rec["lo"]), int(rec["hi"]), int(rec["end_bin"]), int(rec["flags"])) == (0, 3, 4 * W, 0, W - 1, 0, 3)
    assert (lst[56:] == 0x5A).all()
    with pytest.raises(ValueError):
        plan.emissions(fsk, np.zeros(W + 1, F32))
    with pytest.raises(engine.QuadrsError) as e:
        plan.emissions(fsk, -1.0)
    assert e.value.code == _ffi.ERR_INVALID


def test_stats_are_unchanged_by_a_fold(engine, fsk):
    n = len(fsk) // 8
    plan = engine.Plan(0, SR, n, width=64)
    plan.run_host(fsk)
    before = plan.stats()
    fields = [f for f, _ in before._fields_]
    assert before.chunks >= 1 and before.bytes_h2d > 0
    assert plan.emissions(fsk, 0.0)[1] > 0
    after = plan.stats()
    assert [getattr(after, f) for f in fields] == [getattr(before, f) for f in fields]


def test_on_the_callers_stream_behind_a_pending_producer(engine, world):
    """The device source holds NaN poison; on a non-default stream go copies of 1 GiB, then the copy of the true stream into the source.
    The call runs on that stream while the producer is still pending (asserted) and must list the emissions of the TRUE stream, complete
    on return; then a host source on the same side stream."""
    import torch
    plan, data, dev, norms, n, spec = world("cf32_w128")
    thr = threshold_sets(norms)["median"]
    ref = engine.emissions_of(norms, thr, cap=n * 128)
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
        got = plan.emissions(src, thr, cap=n * 128, n_windows=n, device_out=False)
        assert pending, "the producer had finished before the call: the case proves nothing"
        assert same(got, ref, "device source")
        assert same(plan.emissions(data, thr, cap=n * 128, n_windows=n), ref, "host source")
        lst, found = plan.emissions(src, thr, cap=n * 128, n_windows=n)
    side.synchronize()
    assert same(host((lst, found)), ref, "device list")
    del ballast
    torch.cuda.empty_cache()
