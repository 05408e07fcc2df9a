"""Waterfall pictures (qd_picture_*) without a GPU: the colour map and the page layout of the CPU twins against a
numpy f32 restatement of the definition, written op by op here and calling no library function.  Every comparison is equality of bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (2.29, 1.0, 1e-3, 3e38)
INF_BITS, NAN_BITS = 0x7F800000, 0x7FC00000
GAP = 16


# ------------------------------------------------------------------ the referee

def ref_color(x, scale):
    """uint8[..., 3] of f32 norms: the definition, one separately rounded f32 operation a line"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        scaled = x / F32(scale)
        s1 = F32(1.0) - scaled
        hue = (s1 * F32(0.8)) * F32(360.0)
        val = F32(1.0) - s1
        pos = hue - np.floor(hue / F32(360.0)) * F32(360.0)
        h = pos / F32(60.0)
        c = val * F32(1.0)
        m = val - c
        t = h - F32(2.0) * np.floor(h * F32(0.5))
        xx = c * (F32(1.0) - np.abs(t - F32(1.0)))
        for v in (scaled, s1, hue, val, pos, h, c, m, t, xx):
            assert v.dtype == F32
        z = np.zeros_like(c)
        sector = [(F32(k) <= h) & (h < F32(k + 1)) for k in range(5)]         # NaN: every comparison is false, the `else` branch
        r = np.select(sector, [c, xx, z, z, xx], default=c)
        g = np.select(sector, [xx, c, c, xx, z], default=z)
        b = np.select(sector, [z, z, xx, c, c], default=xx)
        out = np.empty(x.shape + (3,), dtype=np.uint8)
        for i, chan in enumerate((r, g, b)):
            v = (chan + m) * F32(256.0)
            assert v.dtype == F32
            byte = np.where(np.isnan(v), F32(0), np.clip(np.trunc(v), F32(0), F32(255)))     # Rust's `as u8`
            out[..., i] = byte.astype(np.uint8)
    return out


def f32_of(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(F32)


def special_patterns(scale):
    """u32 patterns: zero, subnormals, the binade edges, +inf, the quiet NaN, and both f32 neighbours of scale k / 4.8 (the hue sector
    edges) for k = 0 ... 6, with the values themselves"""
    pats = [0, 1, 2, 0x7FFFFF, 0x400000, 0x800000, 0x800001, 0x3F800000, 0x7F7FFFFF, INF_BITS, NAN_BITS, int(F32(1e-40).view(np.uint32))]
    with np.errstate(over="ignore"):
        for k in range(7):
            e = F32(np.float64(F32(scale)) * k / 4.8)
            for v in (np.nextafter(e, F32(0)), e, np.nextafter(e, F32(np.inf))):
                pats.append(int(F32(v).view(np.uint32)))
    return np.array([p for p in pats if p <= INF_BITS or p == NAN_BITS], dtype=np.uint32)


def sweep_patterns(step):
    """every step-th f32 pattern of 0 ... 0x7f800000"""
    return np.arange(0, INF_BITS + 1, step, dtype=np.uint64).astype(np.uint32)


def ref_geometry(W, w, h, stretch):
    row_height = stretch * W + GAP
    strips = h // row_height + 1
    return row_height, strips, strips * w


def ref_picture(norms, W, w, h, stretch, scan, scale, at=0, into=None):
    """`render`'s layout as a literal loop over windows, bins and stretch (src/ui/mod.rs:311-391) on the referee's colours"""
    pic = np.zeros((h, w, 3), dtype=np.uint8) if into is None else into
    row_height, _, max_windows = ref_geometry(W, w, h, stretch)
    colors = ref_color(norms, scale)
    for i in range(norms.shape[0]):
        p = at + i
        x, oy = p % w, (p // w) * row_height
        if oy > h or p >= max_windows:
            break
        for o in range(W):
            rgb = (0, 0, 0) if scan >= 1 and p % scan == 0 else colors[i, o]
            for off in range(stretch):
                y = oy + o * stretch + off
                if y >= h:
                    continue
                pic[h - 1 - y, x] = rgb
    return pic


def page_heights(W, stretch):
    """heights that cut a strip between bins, inside one bin's stretch, exactly at k row_height (the invisible strip that still consumes
    w windows), one above it, and below one row_height"""
    rh = stretch * W + GAP
    hs = {rh + stretch * max(W // 2, 1), rh + stretch * (W - 1) + (stretch + 1) // 2, rh, 2 * rh, 2 * rh + 1, max(rh - GAP - 1, 1), rh - 1}
    return sorted(hs)


# ------------------------------------------------------------------ the colour map

def test_the_definitions_sample_values():
    got = ref_color(np.array([0.25, 1.0, 2.0, 2.29, 2.75, np.nan, np.inf, 0.0, -0.0, 1e-40], dtype=F32), 2.29)
    assert got.tolist() == [[7, 0, 27], [0, 111, 78], [223, 135, 0], [255, 0, 0], [255, 0, 255]] + [[0, 0, 0]] * 5


@pytest.mark.parametrize("scale", SCALES)
def test_color_equals_the_referee(engine, scale):
    bits = np.concatenate([sweep_patterns(997), special_patterns(scale), special_patterns(scale) | np.uint32(0x80000000)])
    x = f32_of(bits)
    got = engine.picture_color(x, scale)
    ref = ref_color(x, scale)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, [(hex(int(bits[i])), got[i].tolist(), ref[i].tolist()) for i in bad[:8]]
    if scale == 2.29:
        with np.errstate(all="ignore"):
            # x >= scale saturates the red channel — as long as the hue stays in the sector it wrapped into (h in [5, 6]: x <= 1.2 scale)
            top = (x >= F32(scale)) & (x <= F32(1.2 * scale))
            assert top.sum() > 100 and (ref[top][:, 0] == 255).all()
        for v in (np.nan, np.inf, 0.0, -0.0, 1e-40):
            assert engine.picture_color(np.array([v], dtype=F32), scale).tolist() == [[0, 0, 0]]


# ------------------------------------------------------------------ the page

def random_norms(rng, n, W):
    """norms spread over the colour map's range, with a NaN, an inf and zeros among them"""
    a = (rng.random((n, W), dtype=F32) * F32(3.0)).astype(F32)
    flat = a.reshape(-1)
    flat[rng.integers(0, flat.size, 3)] = [np.nan, np.inf, 0.0]
    return a


@pytest.mark.parametrize("W", [1, 4, 64])
def test_fold_equals_the_literal_loop(engine, W):
    rng = np.random.default_rng(100 + W)
    shapes = 0
    for w in (5, 100, 101, 103):
        for stretch in (1, 2, 3):
            for k, h in enumerate(page_heights(W, stretch)):
                scan = (0, 1, 7)[(shapes + k) % 3]
                _, strips, max_windows = ref_geometry(W, w, h, stretch)
                n = max_windows + 9                                                           # more windows than the page looks at
                norms = random_norms(rng, n, W)
                desc = engine.picture_desc(w, h, stretch, scan, 2.29)
                assert engine.picture_geometry(desc, W) == (strips, max_windows, 3 * w * h)
                ref = ref_picture(norms, W, w, h, stretch, scan, 2.29)
                got = engine.picture_fold(norms, desc)
                assert got.shape == (h, w, 3) and (got == ref).all(), (W, w, h, stretch, scan)
                # the same range in three parts, out of order
                a, b = n // 3, 2 * n // 3 + 1
                parts = engine.picture_init(desc)
                for lo, hi in ((b, n), (0, a), (a, b)):
                    engine.picture_fold(norms[lo:hi], desc, at=lo, into=parts)
                assert (parts == ref).all(), (W, w, h, stretch, scan)
                shapes += 1
    assert shapes >= 4 * 3 * 5


def test_every_scan_at_every_shape_of_one_width(engine):
    rng = np.random.default_rng(7)
    W = 4
    for w in (5, 101):
        for stretch in (1, 3):
            for scan in (0, 1, 7):
                h = 2 * (stretch * W + GAP) + stretch + 1
                norms = random_norms(rng, 3 * w + 2, W)
                desc = engine.picture_desc(w, h, stretch, scan, 1.0)
                ref = ref_picture(norms, W, w, h, stretch, scan, 1.0)
                assert (engine.picture_fold(norms, desc) == ref).all(), (w, stretch, scan)
                if scan == 1:
                    assert not ref.any()                                                      # the reference's default blackens every column
                if scan == 7:
                    first = ref[h - stretch * W:]                                             # the bottom strip: windows 0 ... w - 1
                    assert not first[:, 0].any() and first[:, 1].any()


def test_windows_beyond_the_page_are_ignored_and_a_fold_accumulates(engine):
    W, w, h = 4, 5, 32                                                                        # row_height 20: strips 2, the second shows 12 rows
    desc = engine.picture_desc(w, h, 1, 0, 2.29)
    assert engine.picture_geometry(desc, W) == (2, 10, 3 * w * h)
    norms = np.full((4, W), 1.0, dtype=F32)
    pic = engine.picture_init(desc)
    assert pic.shape == (h, w, 3) and not pic.any()
    before = pic.copy()
    engine.picture_fold(norms, desc, at=10, into=pic)                                         # at max_windows: nothing
    engine.picture_fold(norms, desc, at=1 << 40, into=pic)
    assert (pic == before).all()
    engine.picture_fold(norms, desc, at=8, into=pic)                                          # windows 8, 9 paint; 10, 11 do not
    ref = ref_picture(norms[:2], W, w, h, 1, 0, 2.29, at=8)
    assert (pic == ref).all() and pic[h - 1 - 20, 3].tolist() == [0, 111, 78]


# ------------------------------------------------------------------ geometry, refusals, layout

def test_geometry(engine):
    for W, w, h, stretch in ((8, 640, 480, 4), (1, 1, 1, 1), (64, 101, 80, 1), (64, 101, 79, 1), (4096, 5, 4096, 1), (2048, 7, 10, 3),
                             (1 << 20, 3, 0xFFFFFFFF, 0xFFFFFFFF)):
        desc = engine.picture_desc(w, h, stretch)
        rh, strips, mw = ref_geometry(W, w, h, stretch)
        assert engine.picture_geometry(desc, W) == (strips, mw, 3 * w * h)
    assert engine.picture_geometry(engine.picture_desc(640, 480), 8) == (480 // 48 + 1, 11 * 640, 640 * 480 * 3)


def test_refusals_leave_the_outputs_untouched(engine):
    from quadrs_amd import _ffi
    L = _ffi.lib()
    good = engine.picture_desc(5, 7, 2, 0, 2.29)
    bad = []
    for field, value in (("px_width", 0), ("px_height", 0), ("stretch", 0), ("scale", 0.0), ("scale", -1.0), ("scale", float("inf")),
                         ("scale", float("nan")), ("struct_size", 20), ("struct_size", 28)):
        d = engine.picture_desc(5, 7, 2, 0, 2.29)
        setattr(d, field, value)
        bad.append(d)
    norms = np.ones((3, 4), dtype=F32)
    for d in bad:
        out = [C.c_uint64(111), C.c_uint64(222), C.c_uint64(333)]
        assert L.qd_picture_geometry(C.byref(d), 4, *[C.byref(o) for o in out]) == _ffi.ERR_INVALID
        assert [o.value for o in out] == [111, 222, 333]
        pic = np.full((7, 5, 3), 0xAB, dtype=np.uint8)
        assert L.qd_picture_fold(pic.ctypes.data_as(C.c_void_p), C.byref(d), 4, 0, norms.ctypes.data_as(C.c_void_p), 3) == _ffi.ERR_INVALID
        assert L.qd_picture_init(pic.ctypes.data_as(C.c_void_p), C.byref(d)) == _ffi.ERR_INVALID
        assert (pic == 0xAB).all()
        with pytest.raises(engine.QuadrsError):
            engine.picture_fold(norms, d)
    out = C.c_uint64(111)
    assert L.qd_picture_geometry(None, 4, C.byref(out), None, None) == _ffi.ERR_INVALID
    assert L.qd_picture_geometry(C.byref(good), 0, C.byref(out), None, None) == _ffi.ERR_INVALID and out.value == 111
    assert L.qd_picture_geometry(C.byref(good), 4, None, None, None) == _ffi.OK
    pic = np.full((7, 5, 3), 0xAB, dtype=np.uint8)
    assert L.qd_picture_fold(None, C.byref(good), 4, 0, norms.ctypes.data_as(C.c_void_p), 3) == _ffi.ERR_INVALID
    assert L.qd_picture_fold(pic.ctypes.data_as(C.c_void_p), C.byref(good), 4, 0, None, 3) == _ffi.ERR_INVALID
    assert L.qd_picture_fold(pic.ctypes.data_as(C.c_void_p), C.byref(good), 4, 0, None, 0) == _ffi.OK
    assert L.qd_picture_init(None, C.byref(good)) == _ffi.ERR_INVALID
    assert (pic == 0xAB).all()
    rgb = np.full((3, 3), 0xAB, dtype=np.uint8)
    x = np.ones(3, dtype=F32)
    for s in (0.0, -2.0, float("inf"), float("nan")):
        assert L.qd_picture_color(x.ctypes.data_as(C.c_void_p), 3, s, rgb.ctypes.data_as(C.c_void_p)) == _ffi.ERR_INVALID
    assert L.qd_picture_color(None, 3, 1.0, rgb.ctypes.data_as(C.c_void_p)) == _ffi.ERR_INVALID
    assert L.qd_picture_color(x.ctypes.data_as(C.c_void_p), 3, 1.0, None) == _ffi.ERR_INVALID
    assert (rgb == 0xAB).all()
    assert L.qd_picture_color(None, 0, 1.0, None) == _ffi.OK


def test_struct_layout_against_the_header(engine, tmp_path):
    from quadrs_amd import _ffi
    src = tmp_path / "layout.cpp"
    fields = [name for name, _ in _ffi.PictureDesc._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrs_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(qd_picture_desc));\n'
                   + "".join('    printf(" %%zu %%zu", offsetof(qd_picture_desc, %s), sizeof(((qd_picture_desc *)0)->%s));\n' % (f, f) for f in fields)
                   + '    printf(" %llu\\n", (unsigned long long)QD_PICTURE_MAX_WORKSPACE);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    nums = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_ffi.PictureDesc)]
    for f in fields:
        want += [getattr(_ffi.PictureDesc, f).offset, getattr(_ffi.PictureDesc, f).size]
    assert nums == want + [_ffi.PICTURE_MAX_WORKSPACE]
    assert fields[0] == "struct_size" and C.sizeof(_ffi.PictureDesc) == 24
    assert engine.picture_desc(3, 4).struct_size == 24
    for name in ("qd_picture_geometry", "qd_picture_color", "qd_picture_init", "qd_picture_fold", "qd_plan_picture"):
        assert name in _ffi.SYMBOLS and hasattr(_ffi.lib(), name)
