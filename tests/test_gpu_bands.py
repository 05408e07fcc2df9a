"""qd_plan_bands on the GPU: all six outputs byte for byte against qd_bands_fold of the same plan's qd_plan_run norms, which test_gpu_pool's
`world` holds to the oracle; at every width where a norms plan's kind changes and with band sets that take every lane-group width of
k_bands (1, 4, 16, 64 lanes in a wave, 256 through LDS); independent of batches, memory kinds and call order; planted values against the
integer referee of test_bands_cpu; the short cascade, the refusals, and the relation to the bucket sink.  Golden files only."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import util
from test_bands_cpu import INF_BITS, NAN_BITS, NONE, ref_bands, units
from test_gpu_cascade import PROBE, _data
from test_gpu_pool import FAMILIES, SR, WIDTHS, world  # noqa: F401  (world: the module-scoped fixture)
from test_pool_cpu import F32

pytestmark = pytest.mark.gpu

NAMES = ("level", "sum", "count", "peak", "peak_bin", "pick")
DTYPES = (F32, np.float64, np.uint32, F32, np.uint32, np.uint8)


def host(six):
    import torch
    torch.cuda.synchronize()
    out = [None if t is None else (t.cpu().numpy() if hasattr(t, "cpu") else t) for t in six]
    return tuple(None if o is None else o.view(dt) for o, dt in zip(out, DTYPES))      # torch uint32 rows are int32: the same bits


def same6(got, ref):
    assert len(got) == len(ref) == 6
    for name, g, r in zip(NAMES, got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype and g.tobytes() == r.tobytes(), name
    return True


def band_sets(W):
    """name -> bands: the whole window, the halves, every bin (K capped at 255), the inner bins, a ragged overlapping set, a band twice,
    K = 1 and K = 255"""
    sets = {"whole": [(0, W)], "bins": [(b, b + 1) for b in range(min(W, 255))], "k255": [(k % W, k % W + 1) for k in range(255)]}
    if W >= 2:
        sets["halves"] = [(0, W // 2), (W // 2, W)]
        sets["twice"] = [(0, W // 2), (W - 1, W), (0, W // 2)]
    if W >= 4:
        sets["inner"] = [(1, W - 1)]
        sets["ragged"] = [(0, W // 2 + 1), (W // 4, W), (1, 2), (W // 4 + 1, W - 1), (W - 1, W), (2, W - 1), (0, 3)]
    if W == 2048:
        # 1025 bins from bin 3: the workgroup form (256 lanes, through LDS), cut unevenly, next to one-bin bands in the same call
        sets["workgroup"] = [(3, 1028), (0, 1), (1027, 1028), (2047, 2048), (3, 4)]
        sets["wave"] = [(1, 1025), (1024, 2048), (5, 6)]                 # 1024 bins: 64 lanes, 16 bins each
        sets["quarter"] = [(7, 263), (0, 65), (2047, 2048)]              # 256 bins: 16 lanes
    return sets


@pytest.mark.parametrize("name", WIDTHS + FAMILIES)
def test_matches_the_fold_of_the_plans_norms(engine, world, name):
    plan, data, dev, norms, n, spec = world(name)
    W = spec[3]["width"]
    for tag, bands in band_sets(W).items():
        m = min(n, 4096) if tag == "k255" else n                        # 255 bands a window: the narrow plans' first windows will do
        got = host(plan.bands(dev, bands, n_windows=m))
        assert got[0].shape == (m, len(bands)) and got[5].shape == (m,)
        assert same6(got, engine.bands_fold(norms[:m], bands)), tag
    # one-bin bands restated without a sum: the norm itself
    K = min(W, 255)
    level, total, count, peak, peak_bin, pick = host(plan.bands(dev, [(b, b + 1) for b in range(K)], n_windows=n))
    part = norms[:, :K]
    keep = ~np.isnan(part)
    assert keep.any()
    assert level[keep].tobytes() == part[keep].tobytes() and total[keep].tobytes() == part[keep].astype(np.float64).tobytes()
    assert peak[keep].tobytes() == part[keep].tobytes() and (count == keep).all()
    assert (peak_bin == np.where(keep, np.arange(K, dtype=np.uint32), np.uint32(NONE))).all()
    assert (level.view(np.uint32)[~keep] == NAN_BITS).all() and not total[~keep].any() and not peak[~keep].any()
    first = np.where(keep.any(axis=1), np.argmax(np.where(keep, part, F32(-1)), axis=1), 255)
    assert (pick == first).all()                                         # np.argmax: the first of equals, as the pick


@pytest.mark.parametrize("name", ["cf32_w128", "cf32_w4", "shift_fir_w128", "cascade_w16_s8"])
def test_batch_seams_and_sources(engine, world, name):
    """chunk_bytes = 64 KiB: several batches, the last one ragged; pageable, pinned and device sources; host and device outputs; twice
    on a plan"""
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    W = kw["width"]
    small = engine.Plan(fmt, rate, n_samples, chunk_bytes=1 << 16, **kw)
    if name in ("cf32_w128", "cf32_w4"):
        cw = (1 << 16) // (W * 4)                                       # windows a batch holds
        assert n >= 3 * cw + 5
        n = 3 * cw + 5
        norms = norms[:n]
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    sets = band_sets(W)
    for tag in ("ragged", "halves", "k255"):
        bands = sets[tag]
        whole = engine.bands_fold(norms, bands)
        for p in (plan, small):
            assert same6(host(p.bands(dev, bands, n_windows=n)), whole), tag                           # device -> device
            assert same6(p.bands(dev, bands, n_windows=n, device_out=False), whole), tag               # device -> host
            assert same6(p.bands(data, bands, n_windows=n), whole), tag                                # pageable -> host
            assert same6(host(p.bands(data, bands, n_windows=n, device_out=True)), whole), tag         # pageable -> device
            assert same6(p.bands(pin.array, bands, n_windows=n, pinned=True), whole), tag              # pinned -> host
    # a second call on the same plan reuses the workspace: a smaller result after a larger one, and the first again
    a = plan.bands(data, sets["k255"], n_windows=n)
    b = plan.bands(data, sets["whole"], n_windows=n)
    c = plan.bands(data, sets["k255"], n_windows=n)
    assert same6(a, engine.bands_fold(norms, sets["k255"])) and same6(b, engine.bands_fold(norms, sets["whole"])) and same6(c, a)
    a = small.bands(dev, sets["k255"], n_windows=n, device_out=False)
    b = small.bands(dev, sets["whole"], n_windows=7, device_out=False)
    assert same6(a, engine.bands_fold(norms, sets["k255"])) and same6(b, engine.bands_fold(norms[:7], sets["whole"]))
    pin.close()


@pytest.mark.parametrize("name", ["cf32_w128", "cs8_fir_w64_s16", "cascade_w16_s8"])
def test_sub_range_from_a_slab(engine, world, name):
    import torch
    plan, data, dev, norms, n, (fmt, rate, n_samples, kw) = world(name)
    bps = {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
    first, count = 2, n - 3
    a, cnt = plan.src_range(first, count)
    slab = data[a * bps:(a + cnt) * bps]
    for bands in (band_sets(kw["width"])["ragged"], band_sets(kw["width"])["whole"]):
        ref = engine.bands_fold(norms[first:first + count], bands)         # rows count from the range's first window
        assert same6(plan.bands(slab, bands, first, count, src_first=a), ref)
        sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
        assert same6(host(plan.bands(sd, bands, first, count, src_first=a)), ref)


def test_one_output_only(engine, world):
    import torch
    from quadrs_amd import _ffi
    plan, data, dev, norms, n, _ = world("cf32_w128")
    buf = np.frombuffer(data, dtype=np.uint8)
    bands = band_sets(128)["ragged"]
    K = len(bands)
    table = (_ffi.Band * K)(*[_ffi.Band(lo, hi) for lo, hi in bands])
    ref = engine.bands_fold(norms, bands)
    tdts = (torch.float32, torch.float64, torch.int32, torch.float32, torch.int32, torch.uint8)
    for which, (dt, tdt) in enumerate(zip(DTYPES, tdts)):
        fill = 77 if dt in (np.uint32, np.uint8) else -7.5
        row = 1 if which == 5 else K                                 # pick_rows holds one byte a window
        out = np.full((n + 2) * row, fill, dtype=dt)                 # a guard row on either side
        ptrs = [None] * 6
        ptrs[which] = out.ctypes.data + row * out.itemsize
        _ffi.check(_ffi.lib().qd_plan_bands(plan._h, buf.ctypes.data_as(C.c_void_p), _ffi.MEM_HOST, 0, buf.size // 8, 0, n, table, K,
                                            C.byref(_ffi.BandRows(*ptrs)), _ffi.MEM_HOST, None))
        assert out[row:(n + 1) * row].tobytes() == ref[which].tobytes(), NAMES[which]
        assert (out[:row] == dt(fill)).all() and (out[(n + 1) * row:] == dt(fill)).all()
        # device memory at an address that is not a multiple of 16
        lead = next(k for k in range(row + 1, row + 5) if (k * out.itemsize) % 16)
        t = torch.full((lead + (n + 1) * row,), fill, dtype=tdt, device="cuda")
        at = t.data_ptr() + out.itemsize * lead
        assert at % 16 != 0
        ptrs[which] = at
        _ffi.check(_ffi.lib().qd_plan_bands(plan._h, C.c_void_p(dev.data_ptr()), _ffi.MEM_DEVICE, 0, buf.size // 8, 0, n, table, K,
                                            C.byref(_ffi.BandRows(*ptrs)), _ffi.MEM_DEVICE, None))
        torch.cuda.synchronize()
        h = t.cpu().numpy().view(dt)
        assert h[lead:lead + n * row].tobytes() == ref[which].tobytes(), NAMES[which]
        assert (h[:lead] == dt(fill)).all() and (h[lead + n * row:] == dt(fill)).all()
    # the Python view: the outputs that are not asked for are None
    got = host(plan.bands(dev, bands, n_windows=n, outputs=("pick", "peak_bin")))
    assert [g is None for g in got] == [True, True, True, True, False, False]
    assert got[4].tobytes() == ref[4].tobytes() and got[5].tobytes() == ref[5].tobytes()


def sweep_bits():
    """one pattern a window: every cell value of util.exponent_sweep() (every biased exponent at both ends of the mantissa, an addend in
    every limb at every shift), then the range's ends, +0, a NaN window and a +inf window"""
    flat = [b for cell in util.exponent_sweep() for b in cell]
    return np.array(flat + [1, util.PLANT_MAX, 0, util.PLANT_NAN, util.PLANT_INF, 0x3F800000], dtype=np.uint32)


@pytest.mark.parametrize("W,stride,sets", [
    (64, 1, ("whole", "halves", "inner", "ragged", "bins")),             # 4 lanes an item; one
    (2048, 16, ("workgroup", "wave", "quarter", "whole")),               # 256 lanes through LDS, 64 and 16 in a wave
])
def test_planted_values(engine, W, stride, sets):
    bits = sweep_bits()[::stride] if stride > 1 else sweep_bits()
    bits = np.concatenate([bits, np.array([util.PLANT_NAN, util.PLANT_INF, util.PLANT_MAX, 1], np.uint32)])
    data = util.impulse_stream(bits, W)
    plan = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, len(data) // 8, width=W)
    n = bits.size
    assert plan.complete_windows() >= n
    norms = plan.run_host(data, n_windows=n)
    nb = norms.view(np.uint32)
    planted = np.broadcast_to(bits[:, None], nb.shape)
    nan = bits == util.PLANT_NAN
    assert (nb[~nan] == planted[~nan]).all() and np.isnan(norms[nan]).all()          # every bin of window i holds pattern i
    assert nan.any() and (bits == util.PLANT_INF).any() and (bits >> 23 == 0).any() and (bits >> 23 == 254).any()
    for tag in sets:
        bands = band_sets(W)[tag]
        got = plan.bands(data, bands, n_windows=n)
        assert same6(got, engine.bands_fold(norms, bands)), tag
        ref = ref_bands(nb, bands)
        assert same6(got, (ref[0].view(F32), ref[1], ref[2], ref[3].view(F32), ref[4], ref[5])), tag
        # a window of equal values: the level is the value, the peak sits in the band's first bin, the first band is picked
        live = ~nan
        assert (got[0].view(np.uint32)[live] == planted[live][:, :1]).all() and (got[4][live] == [lo for lo, _ in bands]).all()
        assert (got[5][live] == 0).all() and (got[5][nan] == 255).all() and (got[4][nan] == NONE).all()


def test_short_cascade_folds_its_complete_windows(engine):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    bands = [(0, 4), (1, 3), (3, 4)]
    for first in (0, done - 1, done):
        with pytest.raises(engine.QuadrsError) as e:
            plan.bands(data, bands, first_window=first)
        assert e.value.code == engine._ffi.ERR_SHORT
        count = total - first
        ref = [np.concatenate([r, np.full((count - (done - first),) + r.shape[1:], fill, dtype=r.dtype)])
               for r, fill in zip(engine.bands_fold(norms[first:done], bands), (np.uint32(NAN_BITS).view(F32), 0.0, 0, F32(0), NONE, 255))]
        assert same6(e.value.partial, ref), first
    last = e.value.partial                          # from the first incomplete window on: the rows of a band without values
    assert (last[0].view(np.uint32) == NAN_BITS).all() and not last[1].any() and not last[2].any() and not last[3].view(np.uint32).any()
    assert (last[4] == NONE).all() and (last[5] == 255).all()


def test_refusals_leave_the_outputs_untouched(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8
    L = _ffi.lib()
    buf = np.frombuffer(fsk, dtype=np.uint8)
    src = buf.ctypes.data_as(C.c_void_p)
    outs = [np.full(4 * 255, fill, dtype=dt) for dt, fill in zip(DTYPES, (-7.5, -7.5, 77, -7.5, 77, 77))]
    rows = _ffi.BandRows(*[o.ctypes.data for o in outs])

    def table(*pairs):
        return (_ffi.Band * len(pairs))(*[_ffi.Band(lo, hi) for lo, hi in pairs])

    def call(plan, bands, K, out=rows, first=0, count=4, src_mem=_ffi.MEM_HOST, out_mem=_ffi.MEM_HOST):
        return L.qd_plan_bands(plan._h, src, src_mem, 0, n, first, count, bands, K, C.byref(out) if out is not None else None, out_mem, None)
    ok = table((0, 64), (5, 9))
    for epi in (engine.EPI_GLYPH_U8, engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
        assert call(engine.Plan(0, SR, n, width=64, epilogue=epi), ok, 2) == _ffi.ERR_INVALID
    assert call(engine.Plan(0, SR, n, width=64, stride=1, epilogue=engine.EPI_ROWS_F32), ok, 2, count=1) == _ffi.ERR_INVALID
    assert call(engine.Plan(0, SR, n, width=64, shard_devices=[0, 0]), ok, 2) == _ffi.ERR_UNSUPPORTED
    plan = engine.Plan(0, SR, n, width=64)
    assert call(plan, ok, 0) == _ffi.ERR_INVALID
    assert call(plan, table(*[(0, 1)] * 256), 256) == _ffi.ERR_INVALID
    assert call(plan, None, 2) == _ffi.ERR_INVALID
    for bad in ((3, 3), (9, 3), (0, 65), (64, 65)):
        assert call(plan, table((0, 64), bad), 2) == _ffi.ERR_INVALID, bad
    assert call(plan, ok, 2, out=None) == _ffi.ERR_INVALID
    assert call(plan, ok, 2, out=_ffi.BandRows()) == _ffi.ERR_INVALID
    assert call(plan, ok, 2, src_mem=9) == _ffi.ERR_INVALID and call(plan, ok, 2, out_mem=9) == _ffi.ERR_INVALID
    assert call(plan, ok, 2, first=0, count=plan.n_windows + 1) == _ffi.ERR_SHORT
    assert call(plan, ok, 2, first=plan.n_windows, count=1) == _ffi.ERR_SHORT
    assert call(plan, ok, 2, first=5, count=0) == 0                                  # no windows: nothing is touched
    for o, dt, fill in zip(outs, DTYPES, (-7.5, -7.5, 77, -7.5, 77, 77)):
        assert (o == dt(fill)).all()
    # a workspace above 1 GiB: 2^22 windows of width 1, 255 bands, five host rows of 4 and 8 bytes
    wide = engine.Plan(0, SR, (1 << 22) + 1, width=1)
    assert wide.n_windows == 1 << 22
    big = table(*[(0, 1)] * 255)
    assert L.qd_plan_bands(wide._h, src, _ffi.MEM_HOST, 0, (1 << 22) + 1, 0, 1 << 22, big, 255, C.byref(rows), _ffi.MEM_HOST, None) == _ffi.ERR_UNSUPPORTED
    assert b"spans" in L.qd_last_error()
    for o, dt, fill in zip(outs, DTYPES, (-7.5, -7.5, 77, -7.5, 77, 77)):
        assert (o == dt(fill)).all()
    assert call(plan, ok, 2) == 0 and not (outs[0][:8] == F32(-7.5)).any() and (outs[0][8:] == F32(-7.5)).all()
    got = plan.bands(fsk, [(0, 64)], 5, 0)
    assert got[0].shape == (0, 1) and got[5].shape == (0,)
    with pytest.raises(engine.QuadrsError) as e:
        plan.bands(fsk, [(0, 65)])
    assert e.value.code == _ffi.ERR_INVALID


def test_stats_are_unchanged_by_a_fold(engine, fsk):
    n = len(fsk) // 8
    plan = engine.Plan(0, SR, n, width=64)
    plan.run_host(fsk)
    before = plan.stats()
    fields = [f for f, _ in before._fields_]
    assert before.chunks >= 1 and before.bytes_h2d > 0
    plan.bands(fsk, [(0, 32), (32, 64)])
    after = plan.stats()
    assert [getattr(after, f) for f in fields] == [getattr(before, f) for f in fields]


def test_split_two_pick_is_the_bucket_sink_up_to_its_rounding(engine, fsk):
    """The README's FSK chain (shift 280000, lowpass, width 16): `bucket` sums each unshifted half of the spectrum in f32, in order, and
    sends a tie to 1; its first half is fftshifted band 1.  The pick of the two half bands gives the same digit, except in windows where
    the exact half sums S0, S1 lie within the sequential sums' error of each other: W / 2 terms a side, plus the level's one rounding,
    |S0 - S1| <= W 2^-23 max(S0, S1).  Asserted per differing window; their number is not capped (observed: see DESIGN.md 3.20)."""
    n = len(fsk) // 8
    W = 16
    kw = dict(shift_hz=280000, lowpass=(200000, 32, 400), width=W)
    bucket = engine.Plan(0, SR, n, epilogue=engine.EPI_BUCKET2_U8, **kw)
    plan = engine.Plan(0, SR, n, **kw)
    digits = bucket.run_host(fsk).reshape(-1)
    assert set(np.unique(digits)) == {0, 1}
    level, _, count, _, _, pick = plan.bands(fsk, [(0, W // 2), (W // 2, W)], outputs=("level", "count", "pick"))
    # bucket's loop takes floor((len - W) / stride) windows (src/fft.rs:86), sparkfft's the ceiling (:28); window i starts at i stride in both
    m = digits.size
    assert m >= 100 and pick.size in (m, m + 1) and (count == W // 2).all()
    norms = plan.run_host(fsk).view(np.uint32)
    differ = np.flatnonzero(pick[:m] != digits)
    print("bands -split 2 -pick against bucket: %d windows, %d differ" % (m, differ.size))
    for i in differ:
        assert all(int(b) <= INF_BITS for b in norms[i])
        s0, s1 = (sum(units(int(b)) for b in norms[i, a:a + W // 2]) for a in (0, W // 2))
        assert abs(s0 - s1) * Fraction(1 << 23) <= W * max(s0, s1), (i, s0, s1)
    assert set(np.unique(pick)) == {0, 1}                               # both tones are there: swapped bands would differ in every window
