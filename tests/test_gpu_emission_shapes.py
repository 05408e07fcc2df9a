"""qd_plan_emissions on the GPU against the flood fill itself, on designed shapes: tone-synthesised cf32 streams (util.tone_stream) plant
the masks of test_emission_shapes_cpu's case table — serpentines, spirals, nested rings, a comb, figures on the tile corners, a
checkerboard; widths 2 ... 4096 — and the list of every run must be the flood-fill referee's (test_emissions_cpu.ref_emissions) of the
plan's own norms, byte for byte: in one batch and across the batch seams of two small plans, host and device sources and lists, two
filters, cap = found and cap = 0; the burst list's on_counts are the design's column sums; two streams longer than a span; the width
limit.  The streams are generated: no golden files."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import util
from test_emission_shapes_cpu import BY_NAME, FILTERS, NAMES, Case, batch_windows, design, filtered, seams_inside
from test_emissions_cpu import ref_emissions
from test_gpu_emissions import SPAN_CELLS, host, same
from test_gpu_parity import assert_norms_close

pytestmark = pytest.mark.gpu

F32 = np.float32
ORACLE_CELLS = 1 << 18                                                      # up to here the oracle's transform of the stream is cheap
SPAN_CASES = {"spiral": Case("span_spiral1_w2048", "spiral", (1,), 2048, 3 * (SPAN_CELLS // 2048) - 100, "", (0, 0)),
              "rings": Case("span_rings_w2048", "rings", (), 2048, 3 * (SPAN_CELLS // 2048) - 100, "", (0, 0))}
SPAN_FILTERS = ((1, 1), (3, 5))


def plant(engine, oracle, case):
    """The case's tone stream through a one-batch plan: (plan, data, dev, mask, norms, thr, ref), ref the flood fill of the measured norms
    (so the peaks are the device's own bits) without a filter.  The conditions are asserted here, before anything else: the mask of the
    norms at the threshold is the design, on and off lie 16 x apart at least, and where the oracle is cheap the norms are its norms at
    0 ulp.  A failure here is the stream builder's, not a finding about the emission kernels."""
    import torch
    mask, levels = design(case)
    n, W = case.n, case.W
    data = util.tone_stream(levels)
    assert len(data) == (n + 1) * W * 8 <= util.PLANTED_CAP
    plan = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, len(data) // 8, width=W, chunk_bytes=0)
    assert plan.complete_windows() >= n
    norms = plan.run_host(data, n_windows=n)
    assert norms.shape == (n, W) and not np.isnan(norms).any()
    on_min = float(norms[mask].min())
    off_max = float(norms[~mask].max()) if not mask.all() else 0.0
    level = math.sqrt(on_min * off_max) if off_max > 0.0 else 0.5           # the geometric middle; 0.5 where nothing off is above zero
    thr = np.full(W, level, F32)
    print("%s: W %d n %d on_min %.9g off_max %.3g on/off %.3g threshold %.3g" % (case.name, W, n, on_min, off_max, on_min / off_max if off_max else math.inf, level))
    assert ((norms >= thr) == mask).all(), "the stream does not plant the design"
    assert on_min >= 16 * off_max, (on_min, off_max)
    assert np.abs(norms[mask] - levels[mask]).max() <= 1e-5, "an on cell's norm is its level"      # 12 f32 stages on levels up to 3: 2e-6
    if n * W <= ORACLE_CELLS:
        want = oracle.Chain.from_bytes(data, engine.FMT_CF32, util.PLANTED_SR).spark_fft(W, None, max_windows=n, want_codes=False)[0]
        assert_norms_close(want, norms, case.name, min_exact=1.0, max_ulp=0)
    ref = ref_emissions(norms.view(np.uint32), thr)
    assert int(ref[0]["cells"].sum()) == int(mask.sum())
    print("%s: found %d, largest emission %d cells" % (case.name, ref[1], int(ref[0]["cells"].max())))
    norms.setflags(write=False)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return plan, data, dev, mask, norms, thr, ref


@pytest.fixture(scope="module")
def planted(engine, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = plant(engine, oracle, BY_NAME[name])
        return cache[name]
    return get


def runs(plan, data, dev, thr, refs, n, what):
    """host source into a host list and device source into a device list, cap = found, under every filter of refs"""
    for (min_len, min_cells), ref in refs.items():
        kw = dict(min_len=min_len, min_cells=min_cells, cap=ref[1], n_windows=n)
        assert same(plan.emissions(data, thr, device_out=False, **kw), ref, (what, min_len, min_cells, "host"))
        assert same(host(plan.emissions(dev, thr, device_out=True, **kw)), ref, (what, min_len, min_cells, "device"))


@pytest.mark.parametrize("name", NAMES)
def test_every_run_is_the_flood_fill(engine, planted, name):
    """Three plans a case: one batch, and two small-chunk plans, of which the first cuts batches of whole tile rows and the second does
    not (at 2048 bins 8 and 12 windows for a device source, 4 and 6 for a host source, whose batches are cut by the 8 bytes of a cf32
    sample; at 4096 bins 8 and 4, 4 and 2).  Below 2048 bins the smallest chunk_bytes a plan takes, 64 KiB, holds the whole design, so
    the small plans run without a seam there; that an emission crosses two seams at least is asserted where the case is in the table
    for its seams."""
    case = BY_NAME[name]
    plan, data, dev, mask, norms, thr, ref = planted(name)
    n, W = case.n, case.W
    tr = util.emissions_tile_rows(W)
    refs = {f: filtered(ref, *f) for f in FILTERS}
    assert same(refs[1, 1], ref[:2]) and refs[1, 1][1] > 0
    runs(plan, data, dev, thr, refs, n, "one batch")
    assert plan.emissions(data, thr, cap=0, n_windows=n, device_out=False)[1] == ref[1]      # cap 0, once: counts only
    for k, chunk in enumerate(case.chunks):
        small = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, len(data) // 8, width=W, chunk_bytes=chunk)
        G = max(int(small.info.tile_windows), 1)
        cw_dev, cw_host = batch_windows(case, chunk, 4, G), batch_windows(case, chunk, 8, G)
        if W >= 2048:
            assert cw_dev == batch_windows(case, chunk) and (cw_dev % tr == 0) == (k == 0), (chunk, G, cw_dev)
        if "d" in case.marked:
            assert len(seams_inside(mask, cw_dev)) >= 2 and len(seams_inside(mask, cw_host)) >= 2
        runs(small, data, dev, thr, refs, n, "chunk_bytes %d" % chunk)
        small.close()


@pytest.mark.parametrize("name", NAMES)
def test_relation_to_the_burst_list(engine, planted, name):
    """min_len 1: the burst list's on_counts are the design's column sums, and the cells of the emission list sum to them"""
    plan, data, dev, mask, norms, thr, ref = planted(name)
    n = mask.shape[0]
    _, _, counts = plan.bursts(data, thr, min_len=1, cap=0, n_windows=n)
    assert counts.astype(np.int64).tolist() == mask.sum(axis=0).tolist()
    lst, found = plan.emissions(data, thr, cap=ref[1], n_windows=n)
    assert found == lst.size and int(lst["cells"].sum()) == int(counts.sum()) > 0


@pytest.mark.parametrize("shape", sorted(SPAN_CASES))
def test_a_designed_stream_longer_than_one_span(engine, oracle, shape):
    """W = 2048 and 1436 windows in one batch: spans of 512 windows, two span seams and a ragged last span, as test_gpu_emissions' span
    test; here the list is held to the flood fill itself.  The spiral's arms (and the rings) cross each seam at more than 256 bins, so
    the virtual row holds that many cells of one root that are no neighbours of each other — or, for the rings, two cells of each of
    more than 128 roots."""
    case = SPAN_CASES[shape]
    t0 = time.perf_counter()
    plan, data, dev, mask, norms, thr, ref = plant(engine, oracle, case)
    n, W = case.n, case.W
    span = SPAN_CELLS // W
    assert span == 512 and n == 1436 and len(data) <= 32 << 20
    for seam in (span, 2 * span):
        across = mask[seam - 1] & mask[seam]
        assert int(across.sum()) > 256 and not (across[:-1] & across[1:]).any()
    if shape == "spiral":
        assert ref[1] == 1 and int(ref[0]["cells"][0]) == int(mask.sum())
    else:
        assert ref[1] == 359 and (np.diff(ref[0]["last"].astype(np.int64)) == 2).all() and int(ref[0]["first"][-1]) == 0
    for min_len, min_cells in SPAN_FILTERS:
        want = filtered(ref, min_len, min_cells)
        assert want[1] > 0
        got = host(plan.emissions(dev, thr, min_len, min_cells, cap=want[1], n_windows=n, device_out=True))
        assert same(got, want, (shape, min_len, min_cells))
    print("%s: %.1f s" % (case.name, time.perf_counter() - t0))


def test_width_8192_is_refused(engine):
    """kEmissionsMaxWidth = 4096 is the widest the sink takes (the cases at 4096 above run it).  A cf32 plan without stages cannot be
    built at 8192 bins at all (a window does not fit a workgroup's LDS); a cascade's norms plan of 8192 bins can, the one of
    test_gpu_cascade's width edges: the sink refuses it with ERR_UNSUPPORTED before it reads anything, and the list and found are left
    as they were"""
    from quadrs_amd import _ffi
    from test_gpu_cascade import SHAPES, _stream_len
    W, n = 8192, 6
    with pytest.raises(engine.QuadrsError) as e:
        engine.Plan(engine.FMT_CF32, util.PLANTED_SR, 4 * W, width=W, chunk_bytes=0)
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    n_samples = _stream_len(SHAPES["LS"], W, W // 2, n)
    plan = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, n_samples, stages=SHAPES["LS"], width=W, stride=W // 2)
    assert plan.width == W and plan.complete_windows() == plan.n_windows == n
    L = _ffi.lib()
    buf = np.zeros(n_samples * 8, dtype=np.uint8)
    lst = np.full(8 * 56, 0x5A, np.uint8)
    found = C.c_uint64(99)
    thr = np.full(W, 0.5, F32)
    rc = L.qd_plan_emissions(plan._h, buf.ctypes.data_as(C.c_void_p), _ffi.MEM_HOST, 0, n_samples, 0, n, thr.ctypes.data_as(C.c_void_p), 1, 1,
                             lst.ctypes.data_as(C.c_void_p), 8, C.byref(found), _ffi.MEM_HOST, None)
    assert rc == _ffi.ERR_UNSUPPORTED and b"too wide" in L.qd_last_error()
    assert (lst == 0x5A).all() and found.value == 99
    with pytest.raises(engine.QuadrsError) as e:
        plan.emissions(buf, thr, n_windows=n)
    assert e.value.code == _ffi.ERR_UNSUPPORTED
