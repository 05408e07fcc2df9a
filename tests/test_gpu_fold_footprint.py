"""Footprint tests of the fold sinks (-m gpu): qd_plan_summarize, _pool, _mean, _power, _spread, _density, _bands and _picture read only
qd_plan_src_range of the windows they are asked for and write only the planes they are handed.  The method is test_gpu_footprint.py's:
the slab sits between frames of poison the test owns (util.framed), every output plane in an allocation of its own between guards
(util.fold_plane: at least 64 KiB and four output rows either side), each case runs once per poison pattern and pre-fill, and
util.fold_footprint_violations holds every plane, byte for byte, to the sink's CPU twin over the plan's own qd_plan_run norms of the true,
unframed stream (`world`: those norms are held to the oracle, bit for bit, as every chain here is shift-free).  There is no tolerance.

Per (sink, chain): the whole stream, an interior range off the tile grid and the last three windows; every pool kind, grid, band set and
page; every device plane once at the allocation's alignment and once at its element's alignment but off 16 bytes.  A plane is kept
below PLANE_CAP on the whole-stream range: where a variant's largest plane over it would pass that (density counts at pool 1, 255 bands a window of a
narrow plan) the range [0, n) is cut to its head [0, m); the poison behind the last sample is then the last-three-windows range's.
The picture sink transforms only the windows its page looks at, so its slab is src_range of those.

Soiled workspaces: a stream made of NaN goes through the sink first, from the host and from the device, with more rows than the true run
has.  Positive controls: a changed sample at either end of the slab shows in the first / last row and in no other, so the frames lie
flush against samples the folds consume.  Nothing here provokes a fault: tests/test_fold_footprint_cpu.py is the checker's own control."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bands import band_sets
from test_gpu_footprint import _ranges
from test_gpu_parity import assert_norms_close
from test_gpu_picture import pages
from test_gpu_pool import pools_of
from test_gpu_summary import quantised
from util import (FMT_BYTES, FOLD_FILLS, PLANTED_GRIDS, POISON_WORDS, FoldRun, fold_footprint_violations, fold_guard_bytes, fold_plane, framed,
                  poison, src_frame_bytes)

pytestmark = pytest.mark.gpu

SR = 21_000_000
F32 = np.float32
QS = (0.0, 0.5, 1.0)
GRIDS = [g for g in PLANTED_GRIDS if g in ((0, 256), (1000, 64), (1500, 1))]
PLANE_CAP = 4 << 20
CASC = [("lowpass", (2_000_000, 4, 40)), ("lowpass", (500_000, 4, 40))]
FIR = (200000, 32, 400)
WIDTHS = [f"cf32_w{W}" for W in (1, 2, 4, 64, 256, 2048)]
CHAINS = WIDTHS + ["cs8_fir_w64_s16", "nofir_w4_s2", "cascade_w16_s8"]
PATH_CHAINS = ["cf32_w4", "cf32_w2048", "cs8_fir_w64_s16", "cascade_w16_s8"]
SOILED_CHAINS = ["cf32_w4", "cf32_w256", "cf32_w2048", "cascade_w16_s8"]
CONTROL_CHAINS = ["nofir_w4_s2", "cs8_fir_w64_s16"]


def chain_specs(cupboard, fsk):
    """name -> (format, sample rate, stream, plan keywords, oracle stages); every chain is shift-free"""
    c = {f"cf32_w{W}": (0, SR, fsk * 4, dict(width=W), []) for W in (1, 2, 4, 64, 128, 256, 2048)}
    c["nofir_w4_s2"] = (0, 400, cupboard, dict(width=4, stride=2), [])
    c["cs8_fir_w64_s16"] = (1, SR, quantised(fsk, 1), dict(lowpass=FIR, width=64, stride=16), [("lowpass", FIR)])
    c["cascade_w16_s8"] = (0, SR, fsk, dict(stages=CASC, width=16, stride=8), CASC)
    return c


class World:
    """one chain, made once: the plan, a 64 KiB-chunk plan on demand, the true stream, its complete windows and their norms"""

    def __init__(self, engine, oracle, name, spec):
        self.engine, self.name = engine, name
        self.fmt, self.rate, raw, self.kw, stages = spec
        self.data = np.frombuffer(raw, dtype=np.uint8)
        self.n_samples = self.data.size // FMT_BYTES[self.fmt]
        self.W = self.kw["width"]
        self.plan = engine.Plan(self.fmt, self.rate, self.n_samples, **self.kw)
        self.n = int(self.plan.complete_windows())
        assert self.n >= 6 and len(raw) <= 2 << 20
        self.norms = self.plan.run_host(self.data, n_windows=self.n)
        ch = oracle.Chain.from_bytes(raw, self.fmt, self.rate)
        for _, arg in stages:
            ch = ch.lowpass(*arg)
        ref = ch.spark_fft(self.W, self.kw.get("stride"), max_windows=self.n, want_codes=False)[0]
        assert_norms_close(ref, self.norms, name, min_exact=1.0, max_ulp=0)
        self.norms.setflags(write=False)
        self._small = None

    @property
    def small(self):
        if self._small is None:
            self._small = self.engine.Plan(self.fmt, self.rate, self.n_samples, chunk_bytes=1 << 16, **self.kw)
        return self._small


@pytest.fixture(scope="module")
def world(engine, oracle, cupboard, fsk):
    cache, specs = {}, chain_specs(cupboard, fsk)

    def get(name):
        if name not in cache:
            cache[name] = World(engine, oracle, name, specs[name])
        return cache[name]
    return get


# ------------------------------------------------------------------ the sinks
#
# A sink names its variants for a range of `count` windows of width W, the planes a variant leaves as (name, dtype, shape) — shape[0]
# counts the output rows — the C call into given addresses, and the CPU twin's planes of the range's norms.

def _rows(pool, count):
    return -(-count // min(int(pool), count))


def _lib():
    from quadrs_amd import _ffi
    return _ffi, _ffi.lib()


class Sink:
    host_only = False            # qd_plan_summarize: sum, peak and floor are host memory

    def looked_at(self, param, W, count):
        """the windows of the range that the sink transforms: all of them, but for a picture's page"""
        return count

    def pooled_variants(self, plan, count):
        return list(dict.fromkeys(pools_of(plan, count)))

    def soil(self, w):
        """the variant of the soiling run over the whole stream: more rows than any true run has"""
        return 1

    def row_bytes(self, spec):
        """the bytes of one output row of a plane"""
        return _plane_bytes(spec) // max(int(spec[2][0]), 1)


class PoolSink(Sink):
    name = "pool"
    variants = lambda self, w, first, count: self.pooled_variants(w.plan, count)      # noqa: E731

    def planes(self, pool, W, count):
        return [("peak", F32, (_rows(pool, count), W)), ("floor", F32, (_rows(pool, count), W))]

    def call(self, plan, src, pool, ptr, out_mem, st):
        ffi, L = _lib()
        return L.qd_plan_pool(plan._h, *src, int(pool), ptr["peak"], ptr["floor"], out_mem, st)

    def twin(self, engine, norms, pool):
        return dict(zip(("peak", "floor"), engine.pool_fold(norms, pool)))

    def wrapper(self, plan, src, pool, **kw):
        return dict(zip(("peak", "floor"), plan.pool(src, pool, **kw)))


class MeanSink(PoolSink):
    name, names, dtypes = "mean", ("mean", "sum", "count"), (F32, np.float64, np.uint32)

    def planes(self, pool, W, count):
        return [(n, dt, (_rows(pool, count), W)) for n, dt in zip(self.names, self.dtypes)]

    def call(self, plan, src, pool, ptr, out_mem, st):
        ffi, L = _lib()
        return getattr(L, "qd_plan_" + self.name)(plan._h, *src, int(pool), *[ptr[n] for n in self.names], out_mem, st)

    def twin(self, engine, norms, pool):
        fold, finish = getattr(engine, self.name + "_fold"), getattr(engine, self.name + "_finish")
        return dict(zip(self.names, finish(fold(norms, pool))))

    def wrapper(self, plan, src, pool, **kw):
        return dict(zip(self.names, getattr(plan, self.name)(src, pool, **kw)))


class PowerSink(MeanSink):
    name, names = "power", ("rms", "sumsq", "count")


class SpreadSink(Sink):
    """(pool, outputs): all five planes, and std alone"""
    name = "spread"
    dtypes = dict(std=F32, ssd=np.float64, count=np.uint32, mean=F32, rms=F32)

    def variants(self, w, first, count):
        return [(pool, outs) for pool in self.pooled_variants(w.plan, count) for outs in (tuple(self.dtypes), ("std",))]

    def planes(self, param, W, count):
        pool, outs = param
        return [(n, self.dtypes[n], (_rows(pool, count), W)) for n in outs]

    def call(self, plan, src, param, ptr, out_mem, st):
        ffi, L = _lib()
        rows = ffi.SpreadRows(*[ptr.get(n) for n in self.dtypes])
        return L.qd_plan_spread(plan._h, *src, int(param[0]), C.byref(rows), out_mem, st)

    def twin(self, engine, norms, param):
        pool, outs = param
        got = dict(zip(self.dtypes, engine.spread_finish(engine.spread_fold(norms, pool), outputs=outs)))
        return {n: got[n] for n in outs}

    def wrapper(self, plan, src, param, **kw):
        got = dict(zip(self.dtypes, plan.spread(src, param[0], outputs=param[1], **kw)))
        return {n: got[n] for n in param[1]}

    def soil(self, w):
        return (1, tuple(self.dtypes))


class DensitySink(Sink):
    """(pool, level0, L): the counts and the three traces"""
    name = "density"

    def variants(self, w, first, count):
        return [(pool, level0, L) for pool in self.pooled_variants(w.plan, count) for level0, L in GRIDS]

    def planes(self, param, W, count):
        pool, _, L = param
        return [("counts", np.uint32, (_rows(pool, count), W, L)), ("trace", F32, (len(QS), _rows(pool, count), W))]

    def call(self, plan, src, param, ptr, out_mem, st):
        ffi, L = _lib()
        q = (C.c_double * len(QS))(*QS)
        return L.qd_plan_density(plan._h, *src, int(param[0]), int(param[1]), int(param[2]), ptr["counts"], q, len(QS), ptr["trace"], out_mem, st)

    def twin(self, engine, norms, param):
        pool, level0, L = param
        counts = engine.density_fold(norms, pool, level0, L)
        return dict(counts=counts, trace=np.stack([engine.density_quantile(counts, level0, q)[0] for q in QS]))

    def wrapper(self, plan, src, param, **kw):
        return dict(zip(("counts", "trace"), plan.density(src, param[0], param[1], param[2], q=QS, **kw)))

    def soil(self, w):
        return (1, 1500, 1)

    def row_bytes(self, spec):
        return _plane_bytes(spec) // max(int(spec[2][1] if spec[0] == "trace" else spec[2][0]) * (len(QS) if spec[0] == "trace" else 1), 1)


class BandsSink(Sink):
    """(tag, bands): the five planes of n x K and pick_rows"""
    name = "bands"
    dtypes = dict(level=F32, sum=np.float64, count=np.uint32, peak=F32, peak_bin=np.uint32, pick=np.uint8)

    def variants(self, w, first, count):
        sets = band_sets(w.W)
        assert {len(b) for b in sets.values()} >= {1, 255}
        return [(tag, tuple(b)) for tag, b in sets.items()]

    def planes(self, param, W, count):
        K = len(param[1])
        return [(n, dt, (count,) if n == "pick" else (count, K)) for n, dt in self.dtypes.items()]

    def call(self, plan, src, param, ptr, out_mem, st):
        ffi, L = _lib()
        K = len(param[1])
        table = (ffi.Band * K)(*[ffi.Band(lo, hi) for lo, hi in param[1]])
        rows = ffi.BandRows(*[ptr[n] for n in self.dtypes])
        return L.qd_plan_bands(plan._h, *src, table, K, C.byref(rows), out_mem, st)

    def twin(self, engine, norms, param):
        return dict(zip(self.dtypes, engine.bands_fold(norms, param[1])))

    def wrapper(self, plan, src, param, **kw):
        return dict(zip(self.dtypes, plan.bands(src, param[1], **kw)))

    def soil(self, w):
        return ("soil", tuple((b, b + 1) for b in range(min(w.W, 255))))


class PictureSink(Sink):
    """(tag, page): the pixels; windows beyond the page's max_windows are not transformed"""
    name = "picture"

    def variants(self, w, first, count):
        p = pages(w.engine, w.W, count)
        return [(tag, p[tag]) for tag in ("clipped", "invisible")]

    def looked_at(self, param, W, count):
        import quadrs_amd
        return min(count, quadrs_amd.picture_geometry(param[1], W)[1])

    def planes(self, param, W, count):
        d = param[1]
        return [("pixels", np.uint8, (d.px_height, d.px_width, 3))]

    def call(self, plan, src, param, ptr, out_mem, st):
        ffi, L = _lib()
        painted = C.c_uint64(0xFFFFFFFFFFFFFFFF)
        rc = L.qd_plan_picture(plan._h, *src, C.byref(param[1]), ptr["pixels"], out_mem, C.byref(painted), st)
        assert rc or painted.value == self.looked_at(param, plan.width, src[-1]), (painted.value, src[-1])
        return rc

    def twin(self, engine, norms, param):
        return dict(pixels=engine.picture_fold(norms, param[1]))

    def wrapper(self, plan, src, param, **kw):
        return dict(pixels=plan.picture(src, param[1], **kw)[0])

    def soil(self, w):
        wide = 1000 if w.n > 4000 else 100
        return ("soil", w.engine.picture_desc(wide, (w.n // wide + 1) * (w.W + 16), 1, 0, 2.29))


class SummarySink(Sink):
    """no variants: the struct's bytes, peak and floor, all host memory"""
    name, host_only = "summarize", True
    variants = lambda self, w, first, count: [None]          # noqa: E731

    def planes(self, param, W, count):
        ffi, _ = _lib()
        return [("summary", np.uint8, (C.sizeof(ffi.Summary),)), ("peak", F32, (1, W)), ("floor", F32, (1, W))]

    def call(self, plan, src, param, ptr, out_mem, st):
        ffi, L = _lib()
        return L.qd_plan_summarize(plan._h, *src, C.cast(C.c_void_p(ptr["summary"]), C.POINTER(ffi.Summary)), ptr["peak"], ptr["floor"], st)

    def twin(self, engine, norms, param):
        s = engine.summary_fold(norms)
        return dict(summary=np.frombuffer(bytes(s.c), dtype=np.uint8), peak=s.peak, floor=s.floor)

    def wrapper(self, plan, src, param, **kw):
        kw.pop("device_out", None)
        s = plan.summarize(src, **kw)
        return dict(summary=np.frombuffer(bytes(s.c), dtype=np.uint8), peak=s.peak, floor=s.floor)

    def soil(self, w):
        return None


SINKS = {s.name: s for s in (SummarySink(), PoolSink(), MeanSink(), PowerSink(), SpreadSink(), DensitySink(), BandsSink(), PictureSink())}


# ------------------------------------------------------------------ the framed run

PATHS = {"dd": ("device", "device"), "hh": ("host", "host"), "pd": ("pinned", "device")}       # source memory -> plane memory


def _plane_bytes(spec):
    name, dt, shape = spec
    return int(np.prod(shape)) * np.dtype(dt).itemsize


def _addr(buf):
    return buf.body.data_ptr() if buf.kind == "device" else buf.body.ctypes.data


class Slabs:
    """the framed slabs of one test, uploaded once per (memory, poison pattern, sample range) and shared by the variants"""

    def __init__(self, engine, plan, fmt, data):
        self.engine, self.plan, self.fmt, self.data, self.cache = engine, plan, fmt, data, {}
        self.frame = src_frame_bytes(plan.info, fmt)
        assert self.frame >= 1 << 20

    def get(self, kind, which, a, cnt):
        key = (kind, which, a, cnt)
        if key not in self.cache:
            bps = FMT_BYTES[self.fmt]
            self.cache[key] = framed(kind, self.fmt, which, self.frame, self.data[a * bps:(a + cnt) * bps], self.frame, self.engine)
        return self.cache[key]

    def close(self):
        for s in self.cache.values():
            s.close()
        self.cache = {}


def _one_run(engine, plan, sink, param, slabs, first, count, which, path, skewed):
    """windows [first, first + count) from a framed slab of exactly src_range of the windows the sink looks at, declared through
    src_first, into one framed plane per output; returns the FoldRun"""
    import torch
    ffi, _ = _lib()
    W = plan.width
    src_kind, out_kind = PATHS[path]
    if sink.host_only:
        out_kind = "host"
    a, cnt = plan.src_range(first, sink.looked_at(param, W, count))
    src = slabs.get(src_kind, which, a, cnt)
    planes, row_bytes, ptr = {}, {}, {}
    for spec in sink.planes(param, W, count):
        name, dt, shape = spec
        item = np.dtype(dt).itemsize
        row_bytes[name] = sink.row_bytes(spec)
        planes[name] = fold_plane(out_kind, row_bytes[name], _plane_bytes(spec), FOLD_FILLS[which], item if skewed else 0, engine)
        ptr[name] = _addr(planes[name])
        assert planes[name].lo >= fold_guard_bytes(row_bytes[name]) and ptr[name] % item == 0
        if skewed and out_kind == "device":
            assert ptr[name] % 16 == item % 16 != 0
    mem = {"device": ffi.MEM_DEVICE, "host": ffi.MEM_HOST, "pinned": ffi.MEM_HOST_PINNED}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if src_kind == "device" else None
    torch.cuda.synchronize()
    rc = sink.call(plan, (C.c_void_p(_addr(src)), mem[src_kind], a, cnt, first, count), param, ptr, mem[out_kind], st)
    assert rc == 0, (sink.name, param, first, count, path, ffi.lib().qd_last_error())
    run = FoldRun(planes, row_bytes, FOLD_FILLS[which], src)
    for p in planes.values():
        p.close()
    return run


def _head(sink, param, W, count):
    """the leading windows of a range whose largest plane stays below PLANE_CAP (see the module's docstring)"""
    def largest(c):
        return max(_plane_bytes(s) for s in sink.planes(param, W, c))
    if largest(count) <= PLANE_CAP:
        return count
    lo, hi = 1, count                      # largest(lo) <= cap < largest(hi); plane sizes grow with the count
    assert largest(lo) <= PLANE_CAP, (sink.name, param)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if largest(mid) <= PLANE_CAP else (lo, mid)
    return lo


def _check(w, plan, sink, slabs, first, count, paths=("dd",), variants=None):
    for param in (sink.variants(w, first, count) if variants is None else variants):
        n = _head(sink, param, w.W, count) if (first, count) == (0, w.n) else count      # the other ranges are a few tiles long
        look = sink.looked_at(param, w.W, n)
        refs = sink.twin(w.engine, w.norms[first:first + look], param)
        for path in paths:
            for skewed in ((False,) if PATHS[path][1] == "host" or sink.host_only else (False, True)):
                runs = [_one_run(w.engine, plan, sink, param, slabs, first, n, which, path, skewed) for which in range(len(POISON_WORDS))]
                bad = fold_footprint_violations(runs, refs)
                tag = param[0] if sink.name in ("bands", "picture") else param
                assert not bad, (sink.name, w.name, tag, first, n, path, skewed, bad)


def _three_ranges(w, plan, sink, paths=("dd",)):
    slabs = Slabs(w.engine, plan, w.fmt, w.data)
    for first, count in _ranges(plan, w.n):
        _check(w, plan, sink, slabs, first, count, paths)
    slabs.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("sink", list(SINKS))
def test_device_folds_stay_inside_their_slab_and_planes(world, sink, chain):
    """device source -> device planes (summarize: host planes), every variant, three ranges, both plane alignments"""
    w = world(chain)
    _three_ranges(w, w.plan, SINKS[sink])


@pytest.mark.parametrize("chain", PATH_CHAINS)
@pytest.mark.parametrize("sink", list(SINKS))
@pytest.mark.parametrize("plan", ["plan", "chunked"])
def test_host_and_pinned_sources(world, plan, sink, chain):
    """host -> host and pinned -> device planes, on the plan and on one whose 64 KiB chunks put batch seams inside rows"""
    w = world(chain)
    _three_ranges(w, w.small if plan == "chunked" else w.plan, SINKS[sink], paths=("hh", "pd"))


# ------------------------------------------------------------------ soiled workspaces

def _host(planes):
    import torch
    torch.cuda.synchronize()
    return {n: (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)) for n, t in planes.items() if t is not None}


def _same(got, ref):
    assert set(got) == set(ref)
    for n in ref:
        assert got[n].tobytes() == np.ascontiguousarray(ref[n]).tobytes(), n
    return True


@pytest.mark.parametrize("chain", SOILED_CHAINS)
@pytest.mark.parametrize("sink", list(SINKS))
def test_soiled_workspaces_do_not_leak(world, sink, chain):
    """A whole stream MADE of NaN goes through the sink first, from the host and from the device, with more rows than the true run
    has: the carrier, the ring, the accumulator slots and the plane slots then hold NaN and the folds of NaN.  The result is the
    twin's of all-NaN norms (count 0, mean NaN, the identities).  Then the interior range of the true stream is held to the footprint."""
    import torch
    w, s = world(chain), SINKS[sink]
    assert w.fmt == 0
    nan_stream = poison(0, w.data.size, 0)
    nan_norms = np.full((w.n, w.W), np.nan, dtype=F32)
    first, count = _ranges(w.plan, w.n)[1]
    variants = s.variants(w, first, count)
    param = s.soil(w)
    soil_rows = max(int(sp[2][0]) for sp in s.planes(param, w.W, w.n))
    true_rows = max(int(sp[2][0]) for v in variants for sp in s.planes(v, w.W, count))
    assert soil_rows > true_rows or s.host_only or s.name == "picture", (soil_rows, true_rows)
    ref = s.twin(w.engine, nan_norms, param)
    for name, plane in ref.items():
        if name in ("count", "counts"):
            assert not plane.any()
        if name in ("mean", "level", "std", "rms"):
            assert np.isnan(plane).all()
    slabs = Slabs(w.engine, w.plan, w.fmt, w.data)
    for src in (nan_stream, torch.from_numpy(nan_stream.copy()).cuda()):
        got = _host(s.wrapper(w.plan, src, param, n_windows=w.n))
        assert _same(got, ref), (s.name, chain)
        if s.name == "summarize":
            assert w.engine.summary_fold(nan_norms).n_nan == w.n * w.W
        _check(w, w.plan, s, slabs, first, count, paths=("hh", "dd"), variants=variants)
    slabs.close()


# ------------------------------------------------------------------ positive controls

def _control_stream(w):
    """(clean stream, spoil(sample) -> stream): cf32: the true stream, and a quiet NaN on the sample.  cs8 has no NaN, and a code
    change on the true stream cannot work at the head: the first consumed sample meets the FIR's edge tap alone, 1.4e-11, far below
    half an ulp of the true norms.  So the cs8 stream is all zero codes (norms exactly 0) and the sample's I becomes 127: every norm
    of the one window that consumes it is then at least the edge tap times 127/128, not 0."""
    if w.fmt == 0:
        def spoil(sample):
            d = w.data.copy()
            d.view("<u4")[2 * sample:2 * sample + 2] = POISON_WORDS[0]
            return d
        return w.data, spoil
    assert w.fmt == 1
    zero = np.zeros_like(w.data)

    def spoil(sample):
        d = zero.copy()
        d[2 * sample] = 127
        return d
    return zero, spoil


def _control_param(s, w, count):
    """a variant in which every window of the range shows: one row a window or three, a grid that holds 0 and tiny values apart, a page
    of one strip at stretch 1 whose scale is of the size of the stream's norms (cs8: of the edge tap), so that no window is black"""
    if s.name in ("mean", "power"):
        return 3
    if s.name == "spread":
        return (3, tuple(s.dtypes))
    if s.name == "density":
        return (3, 0, 256)
    if s.name == "bands":
        return ("halves", ((0, w.W // 2), (w.W // 2, w.W)))
    if s.name == "picture":
        return ("strip", w.engine.picture_desc(count, w.W, 1, 0, float(np.median(w.norms)) if w.fmt == 0 else 1e-11))
    return 1 if s.name == "pool" else None


def _by_row(s, planes, param):
    """every plane as [rows, bytes]: a pooled row, a window's bands, a window's column of pixels; the summary is one row"""
    out = {}
    for n, a in planes.items():
        a = np.asarray(a)
        if s.name == "density" and n == "trace":
            a = a.transpose(1, 0, 2)
        if s.name == "picture":
            a = a.transpose(1, 0, 2)
        if s.name == "summarize":
            a = a.reshape(1, -1)
        a = np.ascontiguousarray(a)
        out[n] = a.view(np.uint8).reshape(a.shape[0], -1)
    return out


@pytest.mark.parametrize("chain", CONTROL_CHAINS)
@pytest.mark.parametrize("sink", list(SINKS))
def test_positive_control_edge_samples_reach_edge_rows(world, sink, chain):
    """A changed sample at the END of the slab changes the last row (the last window's cells) and no earlier one; on the first
    CONSUMED sample (behind a lowpass of T taps the first T - T/2 samples of a window feed no output: the skip of
    test_positive_control_edge_samples_reach_edge_windows) it changes the first row only.  The slabs are tight, so the poison check
    is not vacuous."""
    import torch
    w, s = world(chain), SINKS[sink]
    skip = 0 if chain == "nofir_w4_s2" else FIR[2] - FIR[2] // 2
    clean, spoil = _control_stream(w)
    bps = FMT_BYTES[w.fmt]
    for first, count in _ranges(w.plan, w.n)[:2]:
        param = _control_param(s, w, count)
        a, cnt = w.plan.src_range(first, count)
        assert s.looked_at(param, w.W, count) == count

        def rows(stream, device):
            slab = stream[a * bps:(a + cnt) * bps]
            src = torch.from_numpy(slab.copy()).cuda() if device else slab
            return _by_row(s, _host(s.wrapper(w.plan, src, param, first_window=first, n_windows=count, src_first=a)), param)
        for device in (True, False):
            base = rows(clean, device)
            last, head = rows(spoil(a + cnt - 1), device), rows(spoil(a + skip), device)
            R = next(iter(base.values())).shape[0]
            for got, row in ((last, R - 1), (head, 0)):
                changed = np.zeros(R, dtype=bool)
                for n in base:
                    assert got[n].shape == base[n].shape
                    changed |= (got[n] != base[n]).any(axis=1)
                assert changed[row] and changed.sum() == 1, (s.name, chain, first, count, device, row, np.flatnonzero(changed)[:8])
