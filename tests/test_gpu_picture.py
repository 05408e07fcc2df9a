"""qd_plan_picture on the GPU: the picture byte for byte against qd_picture_fold of the same plan's qd_plan_run norms, at the awkward page
shapes of test_picture_cpu (w = 101 and 103, stretch 3, clipped and invisible strips), independent of batches, memory kinds and slabs;
planted values against the numpy referee of the definition; the tall strip, the edge counts, the short cascade and the refusals.  The golden
FSK head is the source.  No tolerance anywhere: every comparison is equality of bytes."""
import ctypes as C

import numpy as np
import pytest

import util
from test_gpu_cascade import PROBE, _data
from test_picture_cpu import F32, GAP, INF_BITS, NAN_BITS, ref_color, ref_geometry, special_patterns, sweep_patterns

pytestmark = pytest.mark.gpu

SR = 21_000_000
CHAINS = {
    "readme_fsk_w64_s16": dict(shift_hz=280000, lowpass=(200000, 32, 400), width=64, stride=16),
    "plain_w8_s1": dict(width=8, stride=1),                                                  # the reference's own loop: one window a sample
    "cascade_w16_s8": dict(stages=[("lowpass", (2_000_000, 4, 40)), ("lowpass", (500_000, 4, 40))], width=16, stride=8),
}


def host(pic):
    if hasattr(pic, "cpu"):
        import torch
        torch.cuda.synchronize()
        return pic.cpu().numpy()
    return pic


def pages(engine, W, n):
    """name -> desc: a last strip cut inside a bin's stretch, a strip at oy == h (invisible, it still consumes w windows), and a page of
    stretch 1 that holds all n windows with every 7th column a marker"""
    rh = 3 * W + GAP
    k = max(min(n // 101, 5), 1)
    whole_w = 1000 if n > 4000 else 100
    return {"clipped": engine.picture_desc(101, k * rh + 3 * (W // 2) + 1, 3, 0, 2.29),
            "invisible": engine.picture_desc(103, k * rh, 3, 7, 2.29),
            "whole": engine.picture_desc(whole_w, (n // whole_w + 1) * (W + GAP), 1, 7, 1.0)}


@pytest.fixture(scope="module")
def world(engine, fsk):
    """per chain, made once: the plan, a 64 KiB-chunk plan, the stream on the host and on the device, the complete windows and their
    qd_plan_run norms (test_gpu_pool and test_gpu_parity hold those to the oracle)"""
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            kw = CHAINS[name]
            n_samples = len(fsk) // 8
            plan = engine.Plan(engine.FMT_CF32, SR, n_samples, **kw)
            small = engine.Plan(engine.FMT_CF32, SR, n_samples, chunk_bytes=1 << 16, **kw)
            dev = torch.frombuffer(bytearray(fsk), dtype=torch.uint8).cuda()
            n = plan.complete_windows()
            norms = plan.run_host(fsk, n_windows=n)
            norms.setflags(write=False)
            cache[name] = (plan, small, dev, norms, n, kw["width"])
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CHAINS))
def test_equals_the_fold_of_the_plans_norms(engine, world, fsk, name):
    import torch
    plan, small, dev, norms, n, W = world(name)
    assert n >= 120
    for tag, desc in pages(engine, W, n).items():
        _, max_windows, nbytes = engine.picture_geometry(desc, W)[0:3]
        want = min(n, max_windows)
        ref = engine.picture_fold(norms, desc)
        assert ref.any(), tag
        for p in (plan, small):                                         # the small plan's batch seams fall inside the strips
            pic, painted = p.picture(dev, desc, n_windows=n)                                  # device -> device
            assert painted == want and host(pic).tobytes() == ref.tobytes(), (tag, "dd")
            pic, painted = p.picture(fsk, desc, n_windows=n)                                  # host -> host
            assert painted == want and isinstance(pic, np.ndarray) and pic.tobytes() == ref.tobytes(), (tag, "hh")
        pic, painted = small.picture(dev, desc, n_windows=n, device_out=False)                # device -> host
        assert painted == want and pic.tobytes() == ref.tobytes(), (tag, "dh")
        pic, painted = small.picture(fsk, desc, n_windows=n, device_out=True)                 # host -> device
        assert painted == want and host(pic).tobytes() == ref.tobytes(), (tag, "hd")
        # a device picture at every byte alignment, with guard bytes on either side; the picture is overwritten, not added to
        for lead in (1, 2, 3):
            t = torch.full((lead + nbytes + 5,), 0xAB, dtype=torch.uint8, device="cuda")
            out, painted = plan.picture(dev, desc, n_windows=n, out=t[lead:lead + nbytes])
            got = host(t)
            assert got[lead:lead + nbytes].tobytes() == ref.tobytes(), (tag, lead)
            assert (got[:lead] == 0xAB).all() and (got[lead + nbytes:] == 0xAB).all()
    # a window sub-range from a slab that starts inside the stream: columns count from the range's first window
    first, count = 37, n - 40
    a, cnt = plan.src_range(first, count)
    assert a > 0
    slab = fsk[a * 8:(a + cnt) * 8]
    desc = pages(engine, W, count)["clipped"]
    ref = engine.picture_fold(norms[first:first + count], desc)
    want = min(count, engine.picture_geometry(desc, W)[1])
    for p in (plan, small):
        pic, painted = p.picture(slab, desc, first, count, src_first=a)
        assert painted == want and pic.tobytes() == ref.tobytes()
        sd = torch.frombuffer(bytearray(slab), dtype=torch.uint8).cuda()
        pic, painted = p.picture(sd, desc, first, count, src_first=a)
        assert painted == want and host(pic).tobytes() == ref.tobytes()


def planted_patterns(W):
    """test_picture_cpu's pattern list: the special patterns of every scale's sector edges and the sweep of 0 ... 0x7f800000, in steps of
    997 where the impulse stream of all of them stays below util.PLANTED_CAP (W = 1), else in the smallest multiple of 997 that does"""
    special = np.unique(np.concatenate([special_patterns(s) for s in (2.29, 1.0, 1e-3, 3e38)]))
    room = util.PLANTED_CAP // (8 * W) - special.size - 1
    step = 997 * max(-(-(INF_BITS // 997 + 1) // room), 1)
    return np.concatenate([special, sweep_patterns(step)])


@pytest.mark.parametrize("W", [1, 4, 128, 2048])
def test_planted_values(engine, W):
    """Every painted pixel equals the referee's colour of the planted pattern: the device's divisions, floors and subnormals held to the
    numpy f32 restatement, at stretch 1."""
    bits = planted_patterns(W)
    n = bits.size
    data = util.impulse_stream(bits, W)
    assert len(data) <= util.PLANTED_CAP + 8 * W
    plan = engine.Plan(engine.FMT_CF32, util.PLANTED_SR, len(data) // 8, width=W)
    assert plan.complete_windows() >= n
    nan = bits == NAN_BITS
    assert nan.any() and (bits == INF_BITS).any() and ((bits >> 23 == 0) & (bits > 0)).any() and (bits >> 23 == 254).any()
    w = 1024 if n > 1024 else 100
    strips = -(-n // w)
    rh = W + GAP
    for scale in (2.29, 1.0, 1e-3, 3e38) if W == 128 else (2.29,):
        desc = engine.picture_desc(w, strips * rh, 1, 0, scale)
        assert engine.picture_geometry(desc, W)[1] >= n
        pic, painted = plan.picture(data, desc, n_windows=n)
        assert painted == n
        # pixel (x, y) of strip r is window r w + x: gather the strips' bin rows back into [window, bin, rgb]
        up = pic[::-1].reshape(strips, rh, w, 3)                                              # y from the bottom, strip by strip
        assert not up[:, W:].any()                                                            # the gap rows
        got = up[:, :W].transpose(0, 2, 1, 3).reshape(strips * w, W, 3)
        assert not got[n:].any()                                                              # columns no window reaches
        ref = ref_color(bits.view(F32), scale)
        bad = np.nonzero((got[:n] != ref[:, None, :]).any(axis=(1, 2)))[0]
        assert bad.size == 0, [(hex(int(bits[i])), got[i, 0].tolist(), ref[i].tolist()) for i in bad[:8]]


def test_one_tall_strip(engine, world, fsk):
    W = 4096
    n_samples = len(fsk) // 8
    plan = engine.Plan(engine.FMT_CF32, SR, n_samples, width=W)
    n = plan.complete_windows()
    assert n >= 8
    norms = plan.run_host(fsk, n_windows=n)
    for h in (W + GAP - 1, W - 1000, 2 * (W + GAP) + 77):
        desc = engine.picture_desc(5, h, 1, 0, 2.29)
        strips, max_windows, _ = engine.picture_geometry(desc, W)
        pic, painted = plan.picture(fsk, desc, n_windows=n)
        assert painted == min(n, max_windows) == min(n, 5 * strips)
        assert pic.tobytes() == engine.picture_fold(norms, desc).tobytes() and pic.any()


def test_surplus_windows_are_not_run(engine, world, fsk):
    """n_windows above max_windows: painted == max_windows, and the windows beyond are not even transformed — a slab that holds the
    samples of the first max_windows windows only is enough"""
    plan, small, dev, norms, n, W = world("readme_fsk_w64_s16")
    desc = engine.picture_desc(50, 3 * W + GAP, 3, 0, 2.29)                                   # two strips; the second is invisible
    strips, max_windows, _ = engine.picture_geometry(desc, W)
    assert (strips, max_windows) == (2, 100) and max_windows < n
    a, cnt = plan.src_range(0, max_windows)
    assert a == 0 and cnt < len(fsk) // 8
    ref = engine.picture_fold(norms[:max_windows], desc)
    for p in (plan, small):
        pic, painted = p.picture(fsk[:cnt * 8], desc, n_windows=n)
        assert painted == max_windows and pic.tobytes() == ref.tobytes()
    with pytest.raises(engine.QuadrsError):                                                   # one window more does need more samples
        plan.run_host(fsk[:cnt * 8], n_windows=max_windows + 1)
    pic, painted = plan.picture(fsk, desc, n_windows=0)                                       # no windows: QD_OK and a black picture
    assert painted == 0 and pic.shape == (3 * W + GAP, 50, 3) and not pic.any()


def test_short_cascade_paints_its_complete_windows(engine):
    n = 20_036
    data = _data(0, n, seed=13)
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, stages=PROBE, width=4, stride=4)
    total, done = plan.n_windows, plan.complete_windows()
    assert done == total - 1
    norms = plan.run_host(data, n_windows=done)
    desc = engine.picture_desc(101, (total // 101 + 1) * (3 * 4 + GAP), 3, 0, 2.29)
    assert engine.picture_geometry(desc, 4)[1] >= total
    for first in (0, done - 1, done):
        with pytest.raises(engine.QuadrsError) as e:
            plan.picture(data, desc, first_window=first)
        assert e.value.code == engine._ffi.ERR_SHORT
        pic, painted = e.value.partial
        assert painted == done - first and pic.tobytes() == engine.picture_fold(norms[first:done], desc).tobytes()
    # a page that stops before the incomplete window does not look at it: no short read
    narrow = engine.picture_desc(101, 3 * 4 + GAP - 1, 3, 0, 2.29)
    assert engine.picture_geometry(narrow, 4)[1] == 101 < done
    pic, painted = plan.picture(data, narrow)
    assert painted == 101 and pic.tobytes() == engine.picture_fold(norms, narrow).tobytes()


def test_refusals_leave_the_outputs_untouched(engine, fsk):
    from quadrs_amd import _ffi
    n = len(fsk) // 8
    L = _ffi.lib()
    buf = np.frombuffer(fsk, dtype=np.uint8)
    src = buf.ctypes.data_as(C.c_void_p)
    good = engine.picture_desc(5, 100, 2, 0, 2.29)
    pixels = np.full(5 * 100 * 3, 0xAB, dtype=np.uint8)
    painted = C.c_uint64(777)

    def call(plan, desc=good, first=0, count=4, src_mem=_ffi.MEM_HOST, out_mem=_ffi.MEM_HOST, out=pixels):
        return L.qd_plan_picture(plan._h, src, src_mem, 0, n, first, count, C.byref(desc) if desc is not None else None,
                                 out.ctypes.data_as(C.c_void_p) if out is not None else None, out_mem, C.byref(painted), None)
    for epi in (engine.EPI_GLYPH_U8, engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
        assert call(engine.Plan(0, SR, n, width=64, epilogue=epi)) == _ffi.ERR_INVALID
    assert call(engine.Plan(0, SR, n, width=64, stride=1, epilogue=engine.EPI_ROWS_F32), count=1) == _ffi.ERR_INVALID
    assert call(engine.Plan(0, SR, n, width=64, shard_devices=[0, 0])) == _ffi.ERR_UNSUPPORTED
    assert b"qd_picture_fold" in L.qd_last_error()
    plan = engine.Plan(0, SR, n, width=64)
    for field, value in (("px_width", 0), ("px_height", 0), ("stretch", 0), ("scale", 0.0), ("scale", -1.0), ("scale", float("inf")),
                         ("scale", float("nan")), ("struct_size", 20)):
        d = engine.picture_desc(5, 100, 2, 0, 2.29)
        setattr(d, field, value)
        assert call(plan, d) == _ffi.ERR_INVALID, field
    assert call(plan, None) == _ffi.ERR_INVALID and call(plan, out=None) == _ffi.ERR_INVALID
    assert call(plan, src_mem=9) == _ffi.ERR_INVALID and call(plan, out_mem=9) == _ffi.ERR_INVALID
    assert call(plan, first=0, count=plan.n_windows + 1) == _ffi.ERR_SHORT
    assert call(plan, first=plan.n_windows, count=1) == _ffi.ERR_SHORT
    # a host picture above the 1 GiB workspace (the pages of `huge` are never touched)
    big = engine.picture_desc(20000, 20000, 1, 0, 2.29)
    huge = np.empty(3 * 20000 * 20000, dtype=np.uint8)
    huge[:16] = 0xAB
    assert call(plan, big, out=huge) == _ffi.ERR_UNSUPPORTED and b"workspace" in L.qd_last_error()
    assert (huge[:16] == 0xAB).all()
    assert (pixels == 0xAB).all() and painted.value == 777
    assert call(plan) == 0 and painted.value == 4 and pixels.any()
    with pytest.raises(engine.QuadrsError) as e:
        plan.picture(fsk, engine.picture_desc(5, 0))
    assert e.value.code == _ffi.ERR_INVALID and e.value.partial[1] is None


def test_stats_are_unchanged_by_a_fold(engine, fsk):
    n = len(fsk) // 8
    plan = engine.Plan(0, SR, n, width=64)
    plan.run_host(fsk)
    before = plan.stats()
    fields = [f for f, _ in before._fields_]
    assert before.chunks >= 1 and before.bytes_h2d > 0
    plan.picture(fsk, engine.picture_desc(100, 500))
    after = plan.stats()
    assert [getattr(after, f) for f in fields] == [getattr(before, f) for f in fields]
