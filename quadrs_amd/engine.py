"""Python view of the C ABI (tests / bench plumbing; the compute is in libquadrs_hip.so).

Host numpy arrays go through the QD_MEM_HOST paths; torch CUDA tensors are passed by address
(QD_MEM_DEVICE) on torch's current stream.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi
from ._ffi import MEM_DEVICE, MEM_HOST, check, lib

_FMT_BYTES = {0: 8, 1: 2, 2: 2, 3: 4}


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _cur_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def shift_ratio(frequency, sample_rate):
    """Shift::new's ratio (src/shift.rs:28)."""
    return lib().qd_shift_ratio(int(frequency), int(sample_rate))


def lowpass_design(frequency, sample_rate, size):
    """lowpass_filter(cutoff, size) (src/filter.rs:86-105)."""
    out = np.zeros(size, dtype=np.float32)
    check(lib().qd_lowpass_design(int(frequency), int(sample_rate), size, _np_ptr(out)))
    return out


WINDOW_RECT, WINDOW_BH = 0, 1      # qd_chain_desc.windowing / qd_rows_desc.windowing


def window_design(windowing, W):
    """qd_window_design: the W-float table of a window — ones (WINDOW_RECT) or generate_blackman_harris_window (WINDOW_BH, src/ffts.rs:110-119)."""
    out = np.zeros(int(W), dtype=np.float32)
    check(lib().qd_window_design(int(windowing), int(W), _np_ptr(out)))
    return out


def unpack(fmt, data):
    """FileFormat::to_cf32 over a block (src/lib.rs:231-255) on the GPU; returns float32 (n,2)."""
    data = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
    n = data.size // _FMT_BYTES[fmt]
    out = np.zeros((n, 2), dtype=np.float32)
    check(lib().qd_unpack(fmt, _np_ptr(data), n, _np_ptr(out), MEM_HOST))
    return out


def shift(x, abs_off, ratio):
    """Shift::read_at's loop (src/shift.rs:48-52) on float32 (n,2); returns a new array."""
    out = np.array(x, dtype=np.float32, copy=True).reshape(-1, 2)
    check(lib().qd_shift(_np_ptr(out), out.shape[0], int(abs_off), float(ratio), MEM_HOST))
    return out


def lowpass_block(taps, D, raw, valid=None, out_cap=None):
    """LowPass::read_at on a fetched block (src/filter.rs:68-83)."""
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 2)
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    valid = raw.shape[0] if valid is None else valid
    T = taps.size
    if out_cap is None:
        out_cap = max((valid - T) // D, 0) if valid >= T else 0
    out = np.zeros((max(out_cap, 1), 2), dtype=np.float32)
    produced = C.c_size_t(0)
    check(lib().qd_lowpass_block(_np_ptr(taps), T, int(D), _np_ptr(raw), valid, _np_ptr(out), out_cap,
                                 C.byref(produced), MEM_HOST))
    return produced.value, out[:out_cap]


def fft_norm_batch(x, W, n_fft, in_stride):
    """Radix4 forward FFT + fftshift + norm per window (src/fft.rs:25,32,48-53)."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
    out = np.zeros((n_fft, W), dtype=np.float32)
    check(lib().qd_fft_norm_batch(_np_ptr(x), W, n_fft, in_stride, _np_ptr(out), MEM_HOST))
    return out


def bits_scan(marks, scale, cap=None):
    """bits::scan (src/bits.rs:3-55) over 0 / non-0 marks (e.g. an EPI_MARK_U8 output) at `scale` marks per bit: (error, bits).
    Raises QuadrsError(ERR_PANIC) where the reference's loop never terminates.  cap: size of the bits buffer (default: enough)."""
    marks = np.ascontiguousarray(marks).astype(np.uint8, copy=False).reshape(-1)
    if cap is None:
        # a run of r marks emits round(r / scale) <= r / scale + 1 / 2 bits and the accepted runs partition at most all marks
        cap = int(min(marks.size / scale + marks.size / 2 + 2, 1 << 40)) if scale > 0 and np.isfinite(scale) else 0
    bits = np.zeros(max(cap, 1), dtype=np.uint8)
    produced, error = C.c_size_t(0), C.c_double(0.0)
    check(lib().qd_bits_scan(_np_ptr(marks), marks.size, float(scale), _np_ptr(bits), cap, C.byref(produced), C.byref(error)))
    return error.value, bits[:produced.value].copy()


def gen(cos_hz, sample_rate, first, n):
    """Gen::read_at (src/gen.rs:35-47) on the GPU; returns float32 (n,2)."""
    cos = np.ascontiguousarray(cos_hz, dtype=np.int64)
    out = np.zeros((n, 2), dtype=np.float32)
    check(lib().qd_gen(_np_ptr(cos), cos.size, int(sample_rate), int(first), n, _np_ptr(out), MEM_HOST))
    return out


def gen_device(cos_hz, sample_rate, first, out):
    """Gen::read_at (src/gen.rs:35-47) straight into a device buffer: `out` is a float32 (n,2) torch tensor on the GPU
    (the `gen ... | lowpass | sparkfft` chains of BASELINE configs[3] never cross PCIe)."""
    cos = np.ascontiguousarray(cos_hz, dtype=np.int64)
    assert _is_torch(out) and out.is_cuda and out.is_contiguous() and out.dtype.itemsize == 4
    n = out.numel() // 2
    check(lib().qd_gen(_np_ptr(cos), cos.size, int(sample_rate), int(first), n, C.c_void_p(out.data_ptr()), MEM_DEVICE))
    return out


def take_fft(x, width, output_len, slice_=None, windowing=1, in_first=0, samples_len=None):
    """take_fft (src/ffts.rs:18-85) over cf32 samples x = samples [in_first, in_first+len(x)) of the viewed stream."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
    samples_len = in_first + x.shape[0] if samples_len is None else samples_len
    rows = np.zeros((output_len, width), dtype=np.float32)
    s, e = slice_ if slice_ else (0, 0)
    check(lib().qd_take_fft(_np_ptr(x), in_first, x.shape[0], samples_len, 1 if slice_ else 0, s, e, width, windowing,
                            output_len, _np_ptr(rows), MEM_HOST))
    return rows


def plan_options(kernel_policy=_ffi.KERNEL_AUTO, nco_order=0, copy_threads=0, chunk_bytes=0, shard_devices=None, tile_hint=None):
    """qd_plan_options (include/quadrs_hip.h): how a plan picks its kernel and moves host-resident streams."""
    o = _ffi.PlanOptions()
    o.struct_size = C.sizeof(_ffi.PlanOptions)
    o.kernel_policy, o.nco_order, o.copy_threads, o.chunk_bytes = kernel_policy, nco_order, copy_threads, chunk_bytes
    if shard_devices:
        o.n_shards = len(shard_devices)
        for i, d in enumerate(shard_devices):
            o.shard_device[i] = d
    if tile_hint:
        for i, v in enumerate(tile_hint):
            o.tile_hint[i] = int(v)
    return o


def options_from_env(**overrides):
    """Harness convenience (tests, bench.py, scripts/; Plan() consults it only when QUADRS_AMD_HARNESS_ENV=1): the library
    itself reads no tuning environment variables, so the knobs the test matrix is run under are translated HERE into an
    explicit qd_plan_options —
    QD_NO_FIXED=1 -> QD_KERNEL_GENERIC, QD_JIT=1 / 0 -> QD_KERNEL_SPECIALISE / QD_KERNEL_NO_PLAN_TIME,
    QD_TUNE=G:NT:FIRR:FIRB:LB:PAD:BATCH:WG_PER_CU -> tile_hint, QD_NCO_ORDER, QD_CHUNK_MB, QD_COPY_THREADS."""
    e = os.environ
    kw = dict(kernel_policy=_ffi.KERNEL_AUTO)
    if e.get("QD_NO_FIXED"):
        kw["kernel_policy"] = _ffi.KERNEL_GENERIC
    elif e.get("QD_JIT") == "1":
        kw["kernel_policy"] = _ffi.KERNEL_SPECIALISE
    elif e.get("QD_JIT") == "0":
        kw["kernel_policy"] = _ffi.KERNEL_NO_PLAN_TIME
    if e.get("QD_TUNE") and not e.get("QD_NO_FIXED"):
        kw["tile_hint"] = [int(v) for v in e["QD_TUNE"].split(":")][:8]
    if e.get("QD_NCO_ORDER") in ("1", "2"):
        kw["nco_order"] = int(e["QD_NCO_ORDER"])
    if e.get("QD_CHUNK_MB"):
        kw["chunk_bytes"] = int(e["QD_CHUNK_MB"]) << 20
    if e.get("QD_COPY_THREADS"):
        kw["copy_threads"] = int(e["QD_COPY_THREADS"])
    kw.update(overrides)
    return kw


class PinnedBuffer:
    """Host memory from qd_host_alloc (QD_MEM_HOST_PINNED) viewed as a numpy uint8 array."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        check(lib().qd_host_alloc(max(int(nbytes), 1), C.byref(self.ptr)))
        self.nbytes = int(nbytes)
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(max(self.nbytes, 1),))[:self.nbytes]

    def close(self):
        if self.ptr:
            self.array = None
            lib().qd_host_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stage_array(stages):
    """[("shift", f), ("lowpass", (frequency, decimate, size)), ...] (source to sink) -> a ctypes qd_stage array"""
    arr = (_ffi.Stage * max(len(stages), 1))()
    for i, (kind, arg) in enumerate(stages):
        if kind == "shift":
            arr[i].kind, arr[i].shift_hz = _ffi.STAGE_SHIFT, int(arg)
        elif kind == "lowpass":
            freq, decimate, size = arg
            arr[i].kind, arr[i].lowpass_hz, arr[i].decimate, arr[i].taps = _ffi.STAGE_LOWPASS, int(freq), int(decimate), int(size)
        else:
            raise ValueError(f"unknown stage kind {kind!r}")
    return arr


def _sink_desc(fmt, sample_rate, n_samples, width, stride, epilogue, rng, mode):
    d = _ffi.ChainDesc()
    d.struct_size = C.sizeof(_ffi.ChainDesc)
    d.format, d.sample_rate, d.n_samples = fmt, sample_rate, n_samples
    d.width = width
    d.stride = width if stride is None else stride
    d.epilogue, d.mode = epilogue, mode
    if rng is not None:
        d.has_range, d.range_min, d.range_max = 1, rng[0], rng[1]
    return d


def stages_geometry(fmt, sample_rate, n_samples, stages, width=128, stride=None, epilogue=_ffi.EPI_NORMS_F32):
    """qd_stages_geometry: the figures of the plan a stage list makes, from host arithmetic alone (no device).
    Returns (PlanInfo, complete_windows)."""
    d = _sink_desc(fmt, sample_rate, n_samples, width, stride, epilogue, None, _ffi.MODE_EXACT)
    info, done = _ffi.PlanInfo(), C.c_uint64()
    check(lib().qd_stages_geometry(C.byref(d), stage_array(stages), len(stages), C.byref(info), C.byref(done)))
    return info, done.value


def rows_desc(output_len, slice_=None, windowing=1):
    """qd_rows_desc: take_fft's output_len rows over slice_ = (start, end) of the sink's samples (None: (0, len - W))."""
    r = _ffi.RowsDesc()
    r.struct_size = C.sizeof(_ffi.RowsDesc)
    r.output_len, r.windowing = int(output_len), int(windowing)
    if slice_ is not None:
        r.has_slice, r.start, r.end = 1, int(slice_[0]), int(slice_[1])
    return r


def rows_geometry(fmt, sample_rate, n_samples, width, output_len, slice_=None, windowing=1, shift_hz=None, lowpass=None):
    """qd_rows_geometry (host arithmetic, no device): the row offsets (in the sink's samples) of take_fft over the chain
    from -> [shift] -> [lowpass] and the source range the rows read.  Returns (offsets, src_first, src_count)."""
    d = _sink_desc(fmt, sample_rate, n_samples, width, 1, _ffi.EPI_ROWS_F32, None, _ffi.MODE_EXACT)
    if shift_hz is not None:
        d.has_shift, d.shift_hz = 1, int(shift_hz)
    if lowpass is not None:
        d.has_lowpass, d.lowpass_hz, d.decimate, d.taps = 1, int(lowpass[0]), int(lowpass[1]), int(lowpass[2])
    r = rows_desc(output_len, slice_, windowing)
    offs = np.zeros(max(int(output_len), 1), dtype=np.uint64)
    a, b = C.c_uint64(), C.c_uint64()
    check(lib().qd_rows_geometry(C.byref(d), C.byref(r), _np_ptr(offs), int(output_len), C.byref(a), C.byref(b)))
    return offs[:int(output_len)], a.value, b.value


class Summary:
    """qd_summary with its peak / floor arrays (include/quadrs_hip.h, "level summary"): min, max, n_nan, n_windows, hist (uint64[2048]),
    peak and floor (float32[width]).  A new one holds the fold identities (qd_summary_init)."""

    def __init__(self, width):
        self.c = _ffi.Summary()
        self.peak = np.zeros(int(width), dtype=np.float32)
        self.floor = np.zeros(int(width), dtype=np.float32)
        check(lib().qd_summary_init(C.byref(self.c), _np_ptr(self.peak), _np_ptr(self.floor), int(width)))

    width = property(lambda self: self.c.width)
    n_windows = property(lambda self: self.c.n_windows)
    n_nan = property(lambda self: self.c.n_nan)
    min = property(lambda self: np.float32(self.c.min))
    max = property(lambda self: np.float32(self.c.max))

    @property
    def hist(self):
        return np.ctypeslib.as_array(self.c.hist).copy()

    def fold(self, norms):
        """qd_summary_fold: rows of `width` host float32 into this summary; returns self."""
        a = np.ascontiguousarray(norms, dtype=np.float32).reshape(-1, self.width)
        check(lib().qd_summary_fold(C.byref(self.c), _np_ptr(self.peak), _np_ptr(self.floor), _np_ptr(a), a.shape[0]))
        return self

    def merge(self, other):
        """qd_summary_merge: self (+)= other; returns self."""
        check(lib().qd_summary_merge(C.byref(self.c), _np_ptr(self.peak), _np_ptr(self.floor), C.byref(other.c), _np_ptr(other.peak),
                                     _np_ptr(other.floor)))
        return self

    def quantile(self, q):
        """qd_summary_quantile: the (lo, hi) float32 edges of the bucket that holds the q-quantile."""
        lo, hi = C.c_float(), C.c_float()
        check(lib().qd_summary_quantile(C.byref(self.c), float(q), C.byref(lo), C.byref(hi)))
        return np.float32(lo.value), np.float32(hi.value)

    def tobytes(self):
        """every field, for bit-for-bit comparisons"""
        return bytes(self.c) + self.peak.tobytes() + self.floor.tobytes()


def summary_init(width):
    """qd_summary_init: the fold identities for rows of `width` bins."""
    return Summary(width)


def summary_fold(norms, width=None, into=None):
    """qd_summary_fold of host norms rows (a 2-D array, or flat with width=) into `into` or a new Summary."""
    a = np.asarray(norms, dtype=np.float32)
    s = into if into is not None else Summary(a.shape[-1] if width is None else width)
    return s.fold(a)


def summary_merge(dst, src):
    """qd_summary_merge: dst (+)= src."""
    return dst.merge(src)


def summary_quantile(summary, q):
    """qd_summary_quantile."""
    return summary.quantile(q)


def pool_init(width, rows):
    """qd_pool_init: (peak_rows, floor_rows), float32[rows, width] each, holding the fold identities 0.0 / +inf."""
    peak = np.empty((int(rows), int(width)), dtype=np.float32)
    floor = np.empty((int(rows), int(width)), dtype=np.float32)
    check(lib().qd_pool_init(_np_ptr(peak), _np_ptr(floor), int(width), int(rows)))
    return peak, floor


def pool_fold(norms, pool, at=0, into=None):
    """qd_pool_fold: norms rows (n, width) are windows at, at+1, ... of a range and accumulate into rows (at + i) // pool of
    into=(peak_rows, floor_rows) (either may be None), or of new arrays of ceil((at + n) / pool) rows.  Returns (peak_rows, floor_rows)."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    if into is None:
        into = pool_init(width, -(-(int(at) + n) // int(pool)) if pool else 0)
    peak, floor = into
    check(lib().qd_pool_fold(_np_ptr(peak) if peak is not None else None, _np_ptr(floor) if floor is not None else None, width, int(pool),
                             int(at), _np_ptr(a), n))
    return peak, floor


def _limb_init(name, words, width, rows):
    """qd_<name>_init over a new uint64[rows, width, words]"""
    acc = np.empty((int(rows), int(width), words), dtype=np.uint64)
    check(getattr(lib(), "qd_%s_init" % name)(_np_ptr(acc), int(width), int(rows)))
    return acc


def _limb_fold(name, words, norms, pool, at, into):
    """qd_<name>_fold of norms rows (n, width) into `into`, or into a new accumulator of ceil((at + n) / pool) rows"""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    if into is None:
        into = _limb_init(name, words, width, -(-(int(at) + n) // int(pool)) if pool else 0)
    check(getattr(lib(), "qd_%s_fold" % name)(_np_ptr(into), width, int(pool), int(at), _np_ptr(a), n))
    return into


def _limb_merge(name, dst, src):
    """qd_<name>_merge: dst += src"""
    if dst.shape != src.shape:
        raise ValueError("accumulators of different shapes do not merge")
    check(getattr(lib(), "qd_%s_merge" % name)(_np_ptr(dst), _np_ptr(np.ascontiguousarray(src, dtype=np.uint64)), dst.shape[1], dst.shape[0]))
    return dst


def mean_init(width, rows):
    """qd_mean_init: the exact-sum accumulator of `rows` rows of `width` cells, uint64[rows, width, MEAN_WORDS], all words 0."""
    return _limb_init("mean", _ffi.MEAN_WORDS, width, rows)


def mean_fold(norms, pool, at=0, into=None):
    """qd_mean_fold: norms rows (n, width) are windows at, at+1, ... of a range and accumulate into rows (at + i) // pool of the
    accumulator `into`, or of a new one of ceil((at + n) / pool) rows.  Returns the accumulator."""
    return _limb_fold("mean", _ffi.MEAN_WORDS, norms, pool, at, into)


def mean_merge(dst, src):
    """qd_mean_merge: dst += src word by word (two accumulators of the same rows and width).  Returns dst."""
    return _limb_merge("mean", dst, src)


def mean_finish(acc):
    """qd_mean_finish: (mean float32, sum float64, count uint32), [rows, width] each, every cell rounded once from its exact sum."""
    rows, width = acc.shape[0], acc.shape[1]
    mean = np.empty((rows, width), dtype=np.float32)
    total = np.empty((rows, width), dtype=np.float64)
    count = np.empty((rows, width), dtype=np.uint32)
    check(lib().qd_mean_finish(_np_ptr(acc), width, rows, _np_ptr(mean), _np_ptr(total), _np_ptr(count)))
    return mean, total, count


def power_init(width, rows):
    """qd_power_init: the exact sum-of-squares accumulator of `rows` rows of `width` cells, uint64[rows, width, POWER_WORDS], all words 0."""
    return _limb_init("power", _ffi.POWER_WORDS, width, rows)


def power_fold(norms, pool, at=0, into=None):
    """qd_power_fold: norms rows (n, width) are windows at, at+1, ... of a range and their squares accumulate into rows (at + i) // pool
    of the accumulator `into`, or of a new one of ceil((at + n) / pool) rows.  Returns the accumulator."""
    return _limb_fold("power", _ffi.POWER_WORDS, norms, pool, at, into)


def power_merge(dst, src):
    """qd_power_merge: dst += src word by word (two accumulators of the same rows and width).  Returns dst."""
    return _limb_merge("power", dst, src)


def power_finish(acc):
    """qd_power_finish: (rms float32, sumsq float64, count uint32), [rows, width] each, every cell rounded once from its exact sum of
    squares."""
    rows, width = acc.shape[0], acc.shape[1]
    rms = np.empty((rows, width), dtype=np.float32)
    total = np.empty((rows, width), dtype=np.float64)
    count = np.empty((rows, width), dtype=np.uint32)
    check(lib().qd_power_finish(_np_ptr(acc), width, rows, _np_ptr(rms), _np_ptr(total), _np_ptr(count)))
    return rms, total, count


SPREAD_OUTPUTS = ("std", "ssd", "count", "mean", "rms")
_SPREAD_DTYPES = {"std": "float32", "ssd": "float64", "count": "uint32", "mean": "float32", "rms": "float32"}


def _spread_wanted(outputs):
    want = SPREAD_OUTPUTS if outputs is None else tuple(outputs)
    if any(o not in SPREAD_OUTPUTS for o in want):
        raise ValueError("outputs are named from %r" % (SPREAD_OUTPUTS,))
    return [o for o in SPREAD_OUTPUTS if o in want]


def _spread_rows(ptr_of):
    """a qd_spread_rows whose pointers come from ptr_of (output name -> address or None)"""
    def addr(p):
        return p.value if isinstance(p, C.c_void_p) else p
    return _ffi.SpreadRows(*[addr(ptr_of.get(o)) for o in SPREAD_OUTPUTS])


def spread_init(width, rows):
    """qd_spread_init: the exact sum and sum-of-squares accumulator of `rows` rows of `width` cells, uint64[rows, width, SPREAD_WORDS], all
    words 0."""
    return _limb_init("spread", _ffi.SPREAD_WORDS, width, rows)


def spread_fold(norms, pool, at=0, into=None):
    """qd_spread_fold: norms rows (n, width) are windows at, at+1, ... of a range; they and their squares accumulate into rows
    (at + i) // pool of the accumulator `into`, or of a new one of ceil((at + n) / pool) rows.  Returns the accumulator."""
    return _limb_fold("spread", _ffi.SPREAD_WORDS, norms, pool, at, into)


def spread_merge(dst, src):
    """qd_spread_merge: dst += src word by word (two accumulators of the same rows and width).  Returns dst."""
    return _limb_merge("spread", dst, src)


def spread_finish(acc, outputs=None):
    """qd_spread_finish: (std float32, ssd float64, count uint32, mean float32, rms float32), [rows, width] each, every cell rounded once
    from its exact sums.  outputs: the names to work out (SPREAD_OUTPUTS; the default is all); the others are None."""
    rows, width = acc.shape[0], acc.shape[1]
    out = {o: np.empty((rows, width), dtype=_SPREAD_DTYPES[o]) for o in _spread_wanted(outputs)}
    r = _spread_rows({o: _np_ptr(a) for o, a in out.items()})
    check(lib().qd_spread_finish(_np_ptr(acc), width, rows, C.byref(r)))
    return tuple(out.get(o) for o in SPREAD_OUTPUTS)


BAND_OUTPUTS = ("level", "sum", "count", "peak", "peak_bin", "pick")
_BAND_DTYPES = {"level": "float32", "sum": "float64", "count": "uint32", "peak": "float32", "peak_bin": "uint32", "pick": "uint8"}


def _band_wanted(outputs):
    want = BAND_OUTPUTS if outputs is None else tuple(outputs)
    if any(o not in BAND_OUTPUTS for o in want):
        raise ValueError("outputs are named from %r" % (BAND_OUTPUTS,))
    return [o for o in BAND_OUTPUTS if o in want]


def _band_table(bands):
    """(qd_band array or None, K) of a sequence of (lo, hi) pairs"""
    pairs = [(int(lo), int(hi)) for lo, hi in bands]
    if any(not 0 <= x <= 0xffffffff for pair in pairs for x in pair):
        raise ValueError("a band's bins are unsigned 32-bit numbers")
    return ((_ffi.Band * len(pairs))(*[_ffi.Band(lo, hi) for lo, hi in pairs]) if pairs else None), len(pairs)


def _band_rows(ptr_of):
    """a qd_band_rows whose pointers come from ptr_of (output name -> address or None)"""
    def addr(p):
        return p.value if isinstance(p, C.c_void_p) else p
    return _ffi.BandRows(*[addr(ptr_of.get(o)) for o in BAND_OUTPUTS])


def bands_fold(norms, bands, outputs=None):
    """qd_bands_fold, the CPU twin of Plan.bands: norms rows (n, width) and K bands (lo, hi) of fftshifted bins into (level float32, sum
    float64, count uint32, peak float32, peak_bin uint32)[n, K] and pick uint8[n].  outputs: the names to work out (BAND_OUTPUTS; the
    default is all); the others are None."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    table, K = _band_table(bands)
    out = {o: np.empty((n,) if o == "pick" else (n, K), dtype=_BAND_DTYPES[o]) for o in _band_wanted(outputs)}
    r = _band_rows({o: _np_ptr(x) for o, x in out.items()})
    check(lib().qd_bands_fold(_np_ptr(a), width, n, table, K, C.byref(r)))
    return tuple(out.get(o) for o in BAND_OUTPUTS)


BURST_DTYPE = np.dtype([("first", "<u8"), ("length", "<u8"), ("peak_at", "<u8"), ("bin", "<u4"), ("peak", "<f4")])      # qd_burst, 32 bytes
BURSTS_DEFAULT_CAP = 1 << 20


def _burst_thresholds(thresholds, width):
    """float32[width] of a scalar (one level for every bin) or of `width` values"""
    t = np.asarray(thresholds, dtype=np.float32)
    if t.ndim == 0:
        t = np.full(width, t, dtype=np.float32)
    t = np.ascontiguousarray(t.reshape(-1))
    if t.size != width:
        raise ValueError("thresholds holds %d values for %d bins" % (t.size, width))
    return t


def _burst_cap(cap, n, width):
    """cap as given, else what cannot overflow (a bin holds at most ceil(n / 2) bursts), at most BURSTS_DEFAULT_CAP"""
    return min(-(-int(n) // 2) * int(width), BURSTS_DEFAULT_CAP) if cap is None else int(cap)


def _burst_list(into):
    """(list pointer or None, cap) of a BURST_DTYPE array or None"""
    return (None, 0) if into is None or into.size == 0 else (_np_ptr(into), into.size)


def _list_fold(call, state, norms, thresholds, mins, at, into, found, *more):
    """qd_<sink>_fold of norms rows (n, width), windows at, at+1, ..., behind record `found` of `into`; `mins` are the sink's minima and
    `more` what its call takes behind found.  Returns the new found."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    t = _burst_thresholds(thresholds, width)
    f = C.c_uint64(int(found))
    check(call(_np_ptr(state), width, _np_ptr(t), *mins, int(at), _np_ptr(a) if n else None, n, *_burst_list(into), C.byref(f), *more))
    return f.value


def _list_finish(call, state, width, mins, into, found):
    """qd_<sink>_finish of a state of `width` bins behind record `found` of `into`.  Returns found."""
    f = C.c_uint64(int(found))
    check(call(_np_ptr(state), width, *mins, *_burst_list(into), C.byref(f)))
    return f.value


def bursts_init(width):
    """qd_bursts_init: (state uint64[3 width + 1], on_counts uint64[width]) with no run open."""
    state = np.empty(_ffi.BURSTS_WORDS * int(width) + 1, dtype=np.uint64)
    on_counts = np.empty(int(width), dtype=np.uint64)
    check(lib().qd_bursts_init(_np_ptr(state), _np_ptr(on_counts), int(width)))
    return state, on_counts


def bursts_fold(state, norms, thresholds, min_len=1, at=0, into=None, found=0, on_counts=None):
    """qd_bursts_fold: norms rows (n, width) are windows at, at+1, ... of a range.  The bursts that end in them go to the BURST_DTYPE array
    `into` (its length is cap; None: count only) from record `found` on.  Returns the new found."""
    return _list_fold(lib().qd_bursts_fold, state, norms, thresholds, (int(min_len),), at, into, found, None if on_counts is None else _np_ptr(on_counts))


def bursts_finish(state, min_len=1, into=None, found=0):
    """qd_bursts_finish: closes the open runs at the last window folded; the state is left as bursts_init leaves it.  Returns found."""
    return _list_finish(lib().qd_bursts_finish, state, (state.size - 1) // _ffi.BURSTS_WORDS, (int(min_len),), into, found)


def bursts_of(norms, thresholds, min_len=1, cap=None):
    """The CPU twin of Plan.bursts on norms rows (n, width): (list BURST_DTYPE[min(found, cap)], found, on_counts uint64[width])."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    state, on_counts = bursts_init(width)
    into = np.zeros(_burst_cap(cap, n, width), dtype=BURST_DTYPE)
    found = bursts_fold(state, a, thresholds, min_len, 0, into, 0, on_counts)
    found = bursts_finish(state, min_len, into, found)
    return into[:min(found, into.size)], found, on_counts


EMISSION_DTYPE = np.dtype([("first", "<u8"), ("last", "<u8"), ("cells", "<u8"), ("peak_at", "<u8"), ("lo", "<u4"), ("hi", "<u4"), ("end_bin", "<u4"),
                           ("peak_bin", "<u4"), ("peak", "<f4"), ("flags", "<u4")])      # qd_emission, 56 bytes
EMISSIONS_DEFAULT_CAP = 1 << 20


def _emission_cap(cap, n, width):
    """cap as given, else what cannot overflow (no two neighbouring cells belong to two emissions), at most EMISSIONS_DEFAULT_CAP"""
    return min(-(-int(n) * int(width) // 2), EMISSIONS_DEFAULT_CAP) if cap is None else int(cap)


def emissions_init(width):
    """qd_emissions_init: state uint64[8 width + 2] with nothing open."""
    state = np.empty(_ffi.EMISSIONS_WORDS * int(width) + 2, dtype=np.uint64)
    check(lib().qd_emissions_init(_np_ptr(state), int(width)))
    return state


def emissions_fold(state, norms, thresholds, min_len=1, min_cells=1, at=0, into=None, found=0):
    """qd_emissions_fold: norms rows (n, width) are windows at, at+1, ... of a range.  The emissions that end above them go to the
    EMISSION_DTYPE array `into` (its length is cap; None: count only) from record `found` on.  Returns the new found."""
    return _list_fold(lib().qd_emissions_fold, state, norms, thresholds, (int(min_len), int(min_cells)), at, into, found)


def emissions_finish(state, min_len=1, min_cells=1, into=None, found=0):
    """qd_emissions_finish: closes what is open at the last window folded; the state is left as emissions_init leaves it.  Returns found."""
    return _list_finish(lib().qd_emissions_finish, state, (state.size - 2) // _ffi.EMISSIONS_WORDS, (int(min_len), int(min_cells)), into, found)


def emissions_of(norms, thresholds, min_len=1, min_cells=1, cap=None):
    """The CPU twin of Plan.emissions on norms rows (n, width): (list EMISSION_DTYPE[min(found, cap)], found)."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    state = emissions_init(width)
    into = np.zeros(_emission_cap(cap, n, width), dtype=EMISSION_DTYPE)
    found = emissions_fold(state, a, thresholds, min_len, min_cells, 0, into, 0)
    found = emissions_finish(state, min_len, min_cells, into, found)
    return into[:min(found, into.size)], found


CUT_DTYPE = np.dtype([("shift_hz", "<i8"), ("lowpass_hz", "<u8"), ("decimate", "<u8"), ("taps", "<u8"), ("first", "<u8"), ("count", "<u8")])      # qd_cut, 48 bytes


def cut_rule(guard_bins=1, oversample=2, pad=1, taps=0, max_decimate=0):
    """a qd_cut_rule: guard bins on either side of the emission's bins, output rate over twice the lowpass, extra outputs on either side,
    the filter size (0: from the decimation) and the largest decimation (0: QD_CUT_MAX_DECIMATE)."""
    return _ffi.CutRule(C.sizeof(_ffi.CutRule), int(guard_bins), int(oversample), int(pad), int(taps), int(max_decimate))


def cut_of_emission(desc, first_window, emission, rule=None):
    """qd_cut_of_emission (host arithmetic): the cut of one EMISSION_DTYPE record of a list made by a plan with ChainDesc `desc` (Plan.desc)
    from window first_window on.  Returns a CUT_DTYPE scalar."""
    rule = cut_rule() if rule is None else rule
    e = _ffi.Emission.from_buffer_copy(np.asarray(emission, dtype=EMISSION_DTYPE).reshape(1).tobytes())
    cut = _ffi.Cut()
    check(lib().qd_cut_of_emission(C.byref(desc), int(first_window), C.byref(e), C.byref(rule), C.byref(cut)))
    return np.frombuffer(bytes(cut), dtype=CUT_DTYPE)[0]


def _cut_table(cuts):
    a = np.ascontiguousarray(cuts, dtype=CUT_DTYPE).reshape(-1)
    return a if a.size else np.zeros(1, dtype=CUT_DTYPE)[:0], int(np.asarray(cuts).reshape(-1).size)


def cuts_geometry(sample_rate, n_samples, cuts):
    """qd_cuts_geometry (host arithmetic): (offsets uint64[n + 1], src_first, src_count) of a CUT_DTYPE list."""
    a, n = _cut_table(cuts)
    offs = np.zeros(n + 1, dtype=np.uint64)
    lo, cnt = C.c_uint64(), C.c_uint64()
    check(lib().qd_cuts_geometry(int(sample_rate), int(n_samples), _np_ptr(a) if n else None, n, _np_ptr(offs), C.byref(lo), C.byref(cnt)))
    return offs, lo.value, cnt.value


def cuts_run(fmt, sample_rate, n_samples, src, cuts, src_first=0, src_count=None, pinned=False, out=None, chunk_bytes=0, stream=None):
    """qd_cuts_run: every cut of a CUT_DTYPE list in one call.  src holds the raw bytes of source samples [src_first, +src_count): bytes /
    a numpy array (host; pinned=True for a PinnedBuffer array) or a torch CUDA tensor (device).  out: None (host results), a PinnedBuffer
    array (with pinned=True) or a torch CUDA tensor of at least total x 8 bytes (device results).  Returns one float32 (count, 2) array per
    cut: numpy views of one host buffer, or views of `out` for a torch tensor."""
    a, n = _cut_table(cuts)
    offs = np.zeros(n + 1, dtype=np.uint64)
    lo, cnt = C.c_uint64(), C.c_uint64()
    check(lib().qd_cuts_geometry(int(sample_rate), int(n_samples), _np_ptr(a) if n else None, n, _np_ptr(offs), C.byref(lo), C.byref(cnt)))
    total = int(offs[n])
    if _is_torch(src):
        ptr, mem, have, keep = C.c_void_p(src.data_ptr()), MEM_DEVICE, src.numel() * src.element_size() // _FMT_BYTES.get(fmt, 1), src
        st = _cur_stream() if stream is None else C.c_void_p(stream)
    else:
        keep = np.ascontiguousarray(np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else src.view(np.uint8).reshape(-1))
        ptr, mem, have = _np_ptr(keep), (_ffi.MEM_HOST_PINNED if pinned else MEM_HOST), keep.size // _FMT_BYTES.get(fmt, 1)      # (an unknown format is the library's to refuse)
        st = None if stream is None else C.c_void_p(stream)
    src_count = have if src_count is None else int(src_count)
    if out is not None and _is_torch(out):
        import torch
        flat, out_ptr, out_mem = out.view(-1).view(torch.float32), C.c_void_p(out.data_ptr()), MEM_DEVICE
        assert flat.numel() >= 2 * total, "out is smaller than the cuts' total"
        views = [flat[2 * int(offs[k]):2 * int(offs[k + 1])].view(-1, 2) for k in range(n)]
    else:
        flat = np.zeros(2 * max(total, 1), dtype=np.float32) if out is None else out.view(np.float32).reshape(-1)
        assert flat.size >= 2 * total, "out is smaller than the cuts' total"
        out_ptr, out_mem = _np_ptr(flat), (_ffi.MEM_HOST_PINNED if (pinned and out is not None) else MEM_HOST)
        views = [flat[2 * int(offs[k]):2 * int(offs[k + 1])].reshape(-1, 2) for k in range(n)]
    opts = plan_options(chunk_bytes=int(chunk_bytes))
    check(lib().qd_cuts_run(int(fmt), int(sample_rate), int(n_samples), ptr, mem, int(src_first), src_count, _np_ptr(a) if n else None, n,
                            out_ptr, out_mem, C.byref(opts), st))
    del keep
    return views


SEGMENT_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8")])      # qd_segment, 16 bytes


def symbols_desc(epilogue, width, stride=None, rng=None, windowing=0, iq_bytes=0):
    """a qd_symbols_desc: EPI_BUCKET2_U8 or EPI_MARK_U8 over windows of `width` samples every `stride` (None: width); rng = (min, ...) is
    the mark sink's range; iq_bytes caps cuts_symbols' device workspace (0: 1 GiB)."""
    return _ffi.SymbolsDesc(C.sizeof(_ffi.SymbolsDesc), int(epilogue), int(width), int(width if stride is None else stride),
                            0 if rng is None else 1, 0.0 if rng is None else float(rng[0]), int(windowing), 0, int(iq_bytes))


def _segment_table(segments):
    a = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE).reshape(-1)
    return a, int(a.size)


def symbols_geometry(desc, segments):
    """qd_symbols_geometry (host arithmetic): offsets uint64[n + 1] of a SEGMENT_DTYPE list, offsets[n] the total of bytes."""
    a, n = _segment_table(segments)
    offs = np.zeros(n + 1, dtype=np.uint64)
    check(lib().qd_symbols_geometry(C.byref(desc), _np_ptr(a) if n else None, n, _np_ptr(offs)))
    return offs


def _symbols_out(out, total, offs, n, pinned):
    """(keep, pointer, memory kind, per-segment views) of a symbol call's output: None (a new host buffer), a numpy uint8 array (pinned=True
    for a PinnedBuffer array) or a torch CUDA uint8 tensor."""
    if out is not None and _is_torch(out):
        flat = out.view(-1)
        assert flat.element_size() == 1 and flat.numel() >= total, "out is smaller than the symbols' total"
        return flat, C.c_void_p(flat.data_ptr()), MEM_DEVICE, [flat[int(offs[k]):int(offs[k + 1])] for k in range(n)]
    flat = np.zeros(max(total, 1), dtype=np.uint8) if out is None else out.view(np.uint8).reshape(-1)
    assert flat.size >= total, "out is smaller than the symbols' total"
    return flat, _np_ptr(flat), (_ffi.MEM_HOST_PINNED if (pinned and out is not None) else MEM_HOST), [flat[int(offs[k]):int(offs[k + 1])] for k in range(n)]


def symbols_run(desc, iq, segments, pinned=False, out=None, stream=None):
    """qd_symbols_run: one byte per FFT window of every segment of a SEGMENT_DTYPE list over the cf32 buffer iq: a numpy array (host;
    pinned=True for a PinnedBuffer array) or a torch CUDA tensor (device).  out as for cuts_run, in bytes.  Returns one uint8 array per
    segment: numpy views of one host buffer, or views of `out` for a torch tensor."""
    a, n = _segment_table(segments)
    offs = symbols_geometry(desc, a)
    if _is_torch(iq):
        keep, ptr, mem, n_in = iq, C.c_void_p(iq.data_ptr()), MEM_DEVICE, iq.numel() * iq.element_size() // 8
        st = _cur_stream() if stream is None else C.c_void_p(stream)
    else:
        keep = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
        ptr, mem, n_in = _np_ptr(keep), (_ffi.MEM_HOST_PINNED if pinned else MEM_HOST), keep.size // 8
        st = None if stream is None else C.c_void_p(stream)
    flat, out_ptr, out_mem, views = _symbols_out(out, int(offs[n]), offs, n, pinned)
    check(lib().qd_symbols_run(C.byref(desc), ptr, mem, n_in, _np_ptr(a) if n else None, n, out_ptr, out_mem, st))
    del keep
    return views


def cuts_symbols(fmt, sample_rate, n_samples, src, cuts, desc, src_first=0, src_count=None, pinned=False, out=None, chunk_bytes=0, stream=None):
    """qd_cuts_symbols: cuts_run and symbols_run in one call, the IQ staying on the device; cut k is segment k.  src as for cuts_run, out as
    for symbols_run.  Returns one uint8 array per cut."""
    a, n = _cut_table(cuts)
    segs = np.zeros(n, dtype=SEGMENT_DTYPE)
    segs["count"] = a["count"]
    try:
        offs = symbols_geometry(desc, segs)
    except _ffi.QuadrsError:                             # the call below names the first offender in ITS order: the cuts' checks come first
        check(lib().qd_cuts_symbols(int(fmt), int(sample_rate), int(n_samples), None, MEM_HOST, int(src_first), 0 if src_count is None else int(src_count),
                                    _np_ptr(a) if n else None, n, C.byref(desc), None, MEM_HOST, None, None))
        raise
    if _is_torch(src):
        ptr, mem, have, keep = C.c_void_p(src.data_ptr()), MEM_DEVICE, src.numel() * src.element_size() // _FMT_BYTES.get(fmt, 1), src
        st = _cur_stream() if stream is None else C.c_void_p(stream)
    else:
        keep = np.ascontiguousarray(np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else src.view(np.uint8).reshape(-1))
        ptr, mem, have = _np_ptr(keep), (_ffi.MEM_HOST_PINNED if pinned else MEM_HOST), keep.size // _FMT_BYTES.get(fmt, 1)
        st = None if stream is None else C.c_void_p(stream)
    src_count = have if src_count is None else int(src_count)
    flat, out_ptr, out_mem, views = _symbols_out(out, int(offs[n]), offs, n, pinned)
    opts = plan_options(chunk_bytes=int(chunk_bytes))
    check(lib().qd_cuts_symbols(int(fmt), int(sample_rate), int(n_samples), ptr, mem, int(src_first), src_count, _np_ptr(a) if n else None, n,
                                C.byref(desc), out_ptr, out_mem, C.byref(opts), st))
    del keep
    return views


def picture_desc(px_width, px_height, stretch=4, scan=0, scale=2.29):
    """a qd_picture_desc: the page of a waterfall picture.  stretch 4 and scale 2.29 are the reference's; scan 0 (no marker columns) is
    not: its default of 1 blackens every column."""
    return _ffi.PictureDesc(C.sizeof(_ffi.PictureDesc), int(px_width), int(px_height), int(stretch), int(scan), float(scale))


def picture_geometry(desc, width):
    """qd_picture_geometry: (strips, max_windows, bytes) of the page for windows of `width` bins."""
    s, m, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib().qd_picture_geometry(C.byref(desc), int(width), C.byref(s), C.byref(m), C.byref(b)))
    return s.value, m.value, b.value


def picture_color(norms, scale=2.29):
    """qd_picture_color, the colour map alone on the host: float32 norms of any shape into uint8 R,G,B of that shape + (3,)."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    rgb = np.empty(a.shape + (3,), dtype=np.uint8)
    check(lib().qd_picture_color(_np_ptr(a), a.size, float(scale), _np_ptr(rgb)))
    return rgb


def picture_init(desc):
    """qd_picture_init: a black picture, uint8[px_height, px_width, 3], top row first."""
    pixels = np.empty((desc.px_height, desc.px_width, 3), dtype=np.uint8)
    check(lib().qd_picture_init(_np_ptr(pixels), C.byref(desc)))
    return pixels


def picture_fold(norms, desc, at=0, into=None):
    """qd_picture_fold, the CPU twin of Plan.picture: norms rows (n, width) are windows at, at+1, ... of a range and paint their columns
    into the picture `into`, or into a new black one.  Returns the picture, uint8[px_height, px_width, 3]."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    if into is None:
        picture_geometry(desc, width)            # a refused desc has no picture to start from
        into = picture_init(desc)
    check(lib().qd_picture_fold(_np_ptr(into), C.byref(desc), width, int(at), _np_ptr(a), n))
    return into


def density_init(width, levels, rows):
    """qd_density_init: the level counts of `rows` rows of `width` bins, uint32[rows, width, levels], all words 0."""
    counts = np.empty((int(rows), int(width), int(levels)), dtype=np.uint32)
    check(lib().qd_density_init(_np_ptr(counts), int(width), int(levels), int(rows)))
    return counts


def density_fold(norms, pool, level0, levels, at=0, into=None):
    """qd_density_fold: norms rows (n, width) are windows at, at+1, ... of a range and are counted into rows (at + i) // pool of the
    counts `into`, or of new ones of ceil((at + n) / pool) rows.  Returns the counts."""
    a = np.ascontiguousarray(norms, dtype=np.float32)
    n, width = a.shape
    if into is None:
        into = density_init(width, levels, -(-(int(at) + n) // int(pool)) if pool else 0)
    check(lib().qd_density_fold(_np_ptr(into), width, int(level0), int(levels), int(pool), int(at), _np_ptr(a), n))
    return into


def density_merge(dst, src):
    """qd_density_merge: dst += src word by word (two count arrays of the same rows, width and levels).  Returns dst."""
    if dst.shape != src.shape:
        raise ValueError("counts of different shapes do not merge")
    check(lib().qd_density_merge(_np_ptr(dst), _np_ptr(np.ascontiguousarray(src, dtype=np.uint32)), dst.shape[1], dst.shape[2], dst.shape[0]))
    return dst


def density_quantile(counts, level0, q):
    """qd_density_quantile: (lo float32, hi float32, n uint32), [rows, width] each — per cell the bounds of the level that holds the
    q-quantile of its values, and how many values it holds."""
    rows, width, levels = counts.shape
    lo = np.empty((rows, width), dtype=np.float32)
    hi = np.empty((rows, width), dtype=np.float32)
    n = np.empty((rows, width), dtype=np.uint32)
    check(lib().qd_density_quantile(_np_ptr(counts), width, int(level0), levels, rows, float(q), _np_ptr(lo), _np_ptr(hi), _np_ptr(n)))
    return lo, hi, n


class Plan:
    """The fused chain  from -> [shift] -> [lowpass] -> sparkfft|bucket  (Operation::exec, src/lib.rs:83-175); with
    stages=[("shift", f), ("lowpass", (frequency, decimate, size)), ...] any stage list the CLI folds (qd_plan_create_stages)."""

    def __init__(self, fmt, sample_rate, n_samples, shift_hz=None, lowpass=None, width=128, stride=None,
                 epilogue=_ffi.EPI_NORMS_F32, rng=None, options=None, mode=_ffi.MODE_EXACT, stages=None, windowing=0, **option_kw):
        if stages is not None and (shift_hz is not None or lowpass is not None):
            raise ValueError("stages= describes the whole chain: it does not combine with shift_hz= / lowpass=")
        self.stages = list(stages) if stages is not None else None
        d = _ffi.ChainDesc()
        d.struct_size = C.sizeof(_ffi.ChainDesc)
        d.format = fmt
        d.sample_rate = sample_rate
        d.n_samples = n_samples
        if shift_hz is not None:
            d.has_shift, d.shift_hz = 1, int(shift_hz)
        if lowpass is not None:
            freq, decimate, size = lowpass          # (frequency, -decimate [8], size = 2*-power [40])
            d.has_lowpass, d.lowpass_hz, d.decimate, d.taps = 1, int(freq), int(decimate), int(size)
        d.width = width
        d.stride = width if stride is None else stride
        d.epilogue = epilogue
        d.mode = mode            # MODE_FAST: permission to fuse the FIR's multiply-adds (never the default)
        d.windowing = int(windowing)     # WINDOW_BH: sink sample k of every window times window_design(1, width)[k], in front of the FFT
        if rng is not None:
            d.has_range, d.range_min, d.range_max = 1, rng[0], rng[1]
        self.desc = d
        self._h = C.c_void_p()
        hint_from_env = False
        if options is None:
            # A user's plan is described by its arguments alone.  Only under the harness gate (QUADRS_AMD_HARNESS_ENV=1, set by
            # tests/conftest.py, bench.py and scripts/) are the QD_* names of the test matrix translated into options.
            if os.environ.get("QUADRS_AMD_HARNESS_ENV") == "1":
                kw = options_from_env(**option_kw)
                hint_from_env = "tile_hint" in kw and "tile_hint" not in option_kw
            else:
                kw = dict(option_kw)
            options = plan_options(**kw)
        def create(opts):
            if self.stages is None:
                return lib().qd_plan_create_ex(C.byref(d), C.byref(opts), C.byref(self._h))
            return lib().qd_plan_create_stages(C.byref(d), stage_array(self.stages), len(self.stages), C.byref(opts), C.byref(self._h))
        rc = create(options)
        if rc == _ffi.ERR_INVALID and hint_from_env and b"tile_hint" in lib().qd_last_error():
            kw.pop("tile_hint")                      # a sweep's tiling that does not fit this chain: the library's own choice
            options = plan_options(**kw)
            rc = create(options)
        check(rc)
        self.options = options
        info = _ffi.PlanInfo()
        check(lib().qd_plan_get_info(self._h, C.byref(info)))
        self.info = info
        self.n_windows = info.n_windows
        self.width = width
        self.epilogue = epilogue

    def close(self):
        if self._h:
            lib().qd_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def taps(self):
        out = np.zeros(int(self.desc.taps) if self.desc.has_lowpass else 0, dtype=np.float32)
        if out.size:
            check(lib().qd_plan_get_taps(self._h, _np_ptr(out), out.size))
        return out

    def stage_taps(self, stage):
        """taps of lowpass stage `stage` (index into stages=)"""
        kind, arg = self.stages[stage]
        out = np.zeros(int(arg[2]) if kind == "lowpass" else 1, dtype=np.float32)
        check(lib().qd_plan_get_stage_taps(self._h, stage, _np_ptr(out), out.size))
        return out

    def complete_windows(self):
        """leading windows whose read_exact_at succeeds (qd_plan_complete_windows)"""
        n = C.c_uint64()
        check(lib().qd_plan_complete_windows(self._h, C.byref(n)))
        return n.value

    def kernel_name(self):
        """the main kernel's name as rocprofv3 lists it (qd_plan_kernel_name)"""
        buf = C.create_string_buffer(512)
        check(lib().qd_plan_kernel_name(self._h, buf, 512))
        return buf.value.decode()

    def src_range(self, first_window, n_windows):
        a, b = C.c_uint64(), C.c_uint64()
        check(lib().qd_plan_src_range(self._h, first_window, n_windows, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _out_shape_dtype(self, n_windows):
        if self.epilogue == _ffi.EPI_NORMS_F32:
            return (n_windows, self.width), np.float32
        if self.epilogue == _ffi.EPI_GLYPH_U8:
            return (n_windows, self.width), np.uint8
        if self.epilogue == _ffi.EPI_CF32_BLOCKS:
            return (n_windows * self.width, 2), np.float32
        return (n_windows,), np.uint8

    def run_host(self, data, first_window=0, n_windows=None, src_first=0, pinned=False, out=None):
        """data: bytes / uint8 array holding source samples [src_first, ...).  Returns a numpy array.
        pinned=True: `data` (and `out`, if given) are PinnedBuffer arrays -> QD_MEM_HOST_PINNED, no staging copy."""
        buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1))
        n_windows = self.n_windows - first_window if n_windows is None else n_windows
        shape, dt = self._out_shape_dtype(n_windows)
        out_mem = MEM_HOST
        if out is None:
            out = np.zeros(shape, dtype=dt)
        else:
            out = out.view(dt)[:int(np.prod(shape))].reshape(shape)
            out_mem = _ffi.MEM_HOST_PINNED if pinned else MEM_HOST
        count = buf.size // _FMT_BYTES[self.desc.format]
        if n_windows:
            check(lib().qd_plan_run(self._h, _np_ptr(buf), _ffi.MEM_HOST_PINNED if pinned else MEM_HOST, src_first, count,
                                    first_window, n_windows, _np_ptr(out), out_mem, None))
        return out

    def stats(self):
        st = _ffi.PlanStats()
        check(lib().qd_plan_get_stats(self._h, C.byref(st)))
        return st

    def shard_info(self, g):
        si = _ffi.ShardInfo()
        check(lib().qd_plan_shard_info(self._h, g, C.byref(si)))
        return si

    def run_sharded_host(self, data, pinned=False, out=None):
        """qd_plan_run_sharded: the whole stream from one host buffer over the plan's shards (one thread per shard).
        out: an optional host array to write into (a run that ends in QD_ERR_SHORT leaves its complete windows there)."""
        buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1))
        shape, dt = self._out_shape_dtype(self.n_windows)
        out = np.zeros(shape, dtype=dt) if out is None else out.view(dt)[:int(np.prod(shape))].reshape(shape)
        check(lib().qd_plan_run_sharded(self._h, _np_ptr(buf), _ffi.MEM_HOST_PINNED if pinned else MEM_HOST, _np_ptr(out), MEM_HOST))
        return out

    def run_sharded_device(self, slab_ptrs, out_ptrs, sync=True):
        """qd_plan_run_sharded_device: slab_ptrs[g] / out_ptrs[g] are device addresses on shard g's device."""
        n = len(slab_ptrs)
        a = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in slab_ptrs])
        b = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in out_ptrs])
        check(lib().qd_plan_run_sharded_device(self._h, a, b, 1 if sync else 0))

    def run_device(self, src, out, first_window=0, n_windows=None, src_first=0, src_count=None, stream=None):
        """src/out: torch CUDA tensors (any dtype, contiguous).  Enqueues on torch's current stream."""
        n_windows = self.n_windows - first_window if n_windows is None else n_windows
        if src_count is None:
            src_count = src.numel() * src.element_size() // _FMT_BYTES[self.desc.format]
        st = _cur_stream() if stream is None else C.c_void_p(stream)
        check(lib().qd_plan_run(self._h, C.c_void_p(src.data_ptr()), MEM_DEVICE, src_first, src_count, first_window,
                                n_windows, C.c_void_p(out.data_ptr()), MEM_DEVICE, st))

    def take_fft(self, data, output_len, slice_=None, windowing=1, src_first=0, out=None):
        """qd_plan_take_fft of an EPI_ROWS_F32 plan: the (output_len, width) float32 rows of take_fft over the chain.
        data: bytes / numpy array (host; returns a numpy array) or a torch CUDA tensor (device; enqueued on torch's current
        stream, returns a float32 CUDA tensor — `out` if given) holding source samples [src_first, ...)."""
        r = rows_desc(output_len, slice_, windowing)
        if _is_torch(data):
            import torch
            count = data.numel() * data.element_size() // _FMT_BYTES[self.desc.format]
            if out is None:
                out = torch.empty((int(output_len), self.width), dtype=torch.float32, device=data.device)
            check(lib().qd_plan_take_fft(self._h, C.byref(r), C.c_void_p(data.data_ptr()), MEM_DEVICE, src_first, count,
                                         C.c_void_p(out.data_ptr()), MEM_DEVICE, _cur_stream()))
            return out
        buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1))
        rows = np.zeros((int(output_len), self.width), dtype=np.float32)
        check(lib().qd_plan_take_fft(self._h, C.byref(r), _np_ptr(buf), MEM_HOST, src_first, buf.size // _FMT_BYTES[self.desc.format],
                                     _np_ptr(rows), MEM_HOST, None))
        return rows

    def _src_args(self, src, pinned):
        """(ptr, mem, count, stream, keepalive) of a fold's source: bytes / numpy array (host; pinned=True for a PinnedBuffer array) or a
        torch CUDA tensor (device, torch's current stream)."""
        if _is_torch(src):
            return C.c_void_p(src.data_ptr()), MEM_DEVICE, src.numel() * src.element_size() // _FMT_BYTES[self.desc.format], _cur_stream(), src
        buf = np.ascontiguousarray(np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else src.view(np.uint8).reshape(-1))
        return _np_ptr(buf), (_ffi.MEM_HOST_PINNED if pinned else MEM_HOST), buf.size // _FMT_BYTES[self.desc.format], None, buf

    def _fold_rows(self, call, dtypes, src, pool, first_window, n_windows, src_first, pinned, device_out, shapes=None):
        """one [ceil(n_windows / pool), width] array per dtype, filled by `call` (qd_plan_pool, qd_plan_mean, qd_plan_density): torch CUDA
        tensors (the default for a torch src; uint32 as int32, the same bits) or numpy arrays.  shapes(rows): the arrays' shapes where they
        are not [rows, width].  A failing call's error carries them as e.partial."""
        n_windows = self.n_windows - first_window if n_windows is None else n_windows
        rows = -(-n_windows // min(int(pool), n_windows)) if pool and n_windows else 0
        ptr, mem, count, st, _keep = self._src_args(src, pinned)
        shape = shapes(rows) if shapes else [(rows, self.width)] * len(dtypes)
        if _is_torch(src) if device_out is None else device_out:
            import torch
            out = tuple(torch.empty(sh, dtype=getattr(torch, t.replace("uint32", "int32")), device="cuda") for t, sh in zip(dtypes, shape))
            ptrs, out_mem = [C.c_void_p(o.data_ptr()) for o in out], MEM_DEVICE
        else:
            out = tuple(np.empty(sh, dtype=t) for t, sh in zip(dtypes, shape))
            ptrs, out_mem = [_np_ptr(o) for o in out], MEM_HOST
        try:
            check(call(self._h, ptr, mem, src_first, count, first_window, n_windows, int(pool), *ptrs, out_mem, st))
        except _ffi.QuadrsError as e:
            e.partial = out                      # QD_ERR_SHORT of a cascade: the complete windows are folded
            raise
        return out

    def summarize(self, src, first_window=0, n_windows=None, src_first=0, pinned=False):
        """qd_plan_summarize of an EPI_NORMS_F32 plan: the Summary (min, max, n_nan, n_windows, hist, peak, floor) of windows
        [first_window, +n_windows) without bringing the norms back.  src: bytes / numpy array (host; pinned=True for a PinnedBuffer
        array) or a torch CUDA tensor (device, torch's current stream) holding source samples [src_first, ...)."""
        n_windows = self.n_windows - first_window if n_windows is None else n_windows
        s = Summary(self.width)
        ptr, mem, count, st, _keep = self._src_args(src, pinned)
        check(lib().qd_plan_summarize(self._h, ptr, mem, src_first, count, first_window, n_windows, C.byref(s.c), _np_ptr(s.peak),
                                      _np_ptr(s.floor), st))
        return s

    def pool(self, src, pool, first_window=0, n_windows=None, src_first=0, pinned=False, device_out=None):
        """qd_plan_pool of an EPI_NORMS_F32 plan: (peak_rows, floor_rows), float32[ceil(n_windows / pool), width] each — per bin the max /
        min over each group of `pool` consecutive windows of [first_window, +n_windows).  src as for summarize.  device_out: the rows as
        torch CUDA tensors (the default for a torch src) instead of numpy arrays."""
        return self._fold_rows(lib().qd_plan_pool, ("float32", "float32"), src, pool, first_window, n_windows, src_first, pinned, device_out)

    def mean(self, src, pool, first_window=0, n_windows=None, src_first=0, pinned=False, device_out=None):
        """qd_plan_mean of an EPI_NORMS_F32 plan: (mean_rows float32, sum_rows float64, count_rows uint32), [ceil(n_windows / pool), width]
        each — per bin the exact sum of each group of `pool` consecutive windows of [first_window, +n_windows), rounded once, its mean
        rounded once, and the number of non-NaN values.  src and device_out as for pool (a torch count_rows is int32: the same bits)."""
        return self._fold_rows(lib().qd_plan_mean, ("float32", "float64", "uint32"), src, pool, first_window, n_windows, src_first, pinned, device_out)

    def power(self, src, pool, first_window=0, n_windows=None, src_first=0, pinned=False, device_out=None):
        """qd_plan_power of an EPI_NORMS_F32 plan: (rms_rows float32, sumsq_rows float64, count_rows uint32), [ceil(n_windows / pool), width]
        each — per bin the root mean square of each group of `pool` consecutive windows of [first_window, +n_windows), rounded once from
        the exact sum of squares, that sum rounded once, and the number of non-NaN values.  src and device_out as for pool (a torch
        count_rows is int32: the same bits)."""
        return self._fold_rows(lib().qd_plan_power, ("float32", "float64", "uint32"), src, pool, first_window, n_windows, src_first, pinned, device_out)

    def spread(self, src, pool, first_window=0, n_windows=None, src_first=0, pinned=False, device_out=None, outputs=None):
        """qd_plan_spread of an EPI_NORMS_F32 plan: (std_rows float32, ssd_rows float64, count_rows uint32, mean_rows float32, rms_rows
        float32), [ceil(n_windows / pool), width] each — per bin of each group of `pool` consecutive windows of [first_window, +n_windows)
        the population standard deviation rounded once from the exact sum and sum of squares, the sum of squared deviations rounded once,
        the number of non-NaN values, and Plan.mean's mean and Plan.power's rms bit for bit, from one pass.  src and device_out as for
        pool (a torch count_rows is int32: the same bits).  outputs: the names to work out (SPREAD_OUTPUTS; the default is all); the
        others are None and cost nothing."""
        names = _spread_wanted(outputs)

        def call(h, ptr, mem, src_first, count, first_window, n_windows, pool, *rest):
            ptrs, (out_mem, st) = rest[:-2], rest[-2:]
            r = _spread_rows(dict(zip(names, ptrs)))
            return lib().qd_plan_spread(h, ptr, mem, src_first, count, first_window, n_windows, pool, C.byref(r), out_mem, st)
        out = dict(zip(names, self._fold_rows(call, tuple(_SPREAD_DTYPES[o] for o in names), src, pool, first_window, n_windows, src_first,
                                              pinned, device_out)))
        return tuple(out.get(o) for o in SPREAD_OUTPUTS)

    def bands(self, src, bands, first_window=0, n_windows=None, src_first=0, pinned=False, device_out=None, outputs=None):
        """qd_plan_bands of an EPI_NORMS_F32 plan: (level_rows float32, sum_rows float64, count_rows uint32, peak_rows float32,
        peak_bin_rows uint32)[n_windows, K] and pick_rows uint8[n_windows] — per window of [first_window, +n_windows) and band (lo, hi)
        of fftshifted bins the exact sum rounded once, its mean rounded once, the number of non-NaN values, the peak and the lowest bin
        that holds it, and per window the loudest band.  src and device_out as for pool (torch uint32 rows are int32: the same bits).
        outputs: the names to work out (BAND_OUTPUTS; the default is all); the others are None and cost nothing."""
        names = _band_wanted(outputs)
        table, K = _band_table(bands)

        def call(h, ptr, mem, src_first, count, first_window, n_windows, _pool, *rest):
            ptrs, (out_mem, st) = rest[:-2], rest[-2:]
            r = _band_rows(dict(zip(names, ptrs)))
            return lib().qd_plan_bands(h, ptr, mem, src_first, count, first_window, n_windows, table, K, C.byref(r), out_mem, st)
        shapes = lambda rows: [(rows,) if o == "pick" else (rows, K) for o in names]      # noqa: E731
        out = dict(zip(names, self._fold_rows(call, tuple(_BAND_DTYPES[o] for o in names), src, 1, first_window, n_windows, src_first, pinned,
                                              device_out, shapes)))
        return tuple(out.get(o) for o in BAND_OUTPUTS)

    def _list_call(self, call, dtype, cap_rule, mins, src, thresholds, cap, first_window, n_windows, src_first, pinned, device_out, out, counts=None):
        """(list, found) of a list sink's `call` (qd_plan_bursts, qd_plan_emissions) whose records are `dtype`: cap from `out`, else from
        cap_rule; `mins` are the sink's minima.  counts: (counts_out,) where the call also fills a plane of width uint64 words, which
        then comes third.  A failing call's error carries the result as e.partial."""
        n_windows = self.n_windows - first_window if n_windows is None else n_windows
        ptr, mem, count, st, _keep = self._src_args(src, pinned)
        W, size = self.width, dtype.itemsize
        t = _burst_thresholds(thresholds, W)
        dev = (_is_torch(src) if device_out is None else device_out) if out is None else _is_torch(out)
        if out is None:
            cap = cap_rule(cap, n_windows, W)
        else:                                    # the list given holds what it holds: cap defaults to it and may not exceed it
            room = (out.numel() * out.element_size() if _is_torch(out) else out.nbytes) // size
            cap = room if cap is None else int(cap)
            if cap > room:
                raise ValueError("cap %d above the %d records that out holds" % (cap, room))
        cnt = counts[0] if counts else None
        if cnt is not None and (cnt.numel() * cnt.element_size() if _is_torch(cnt) else cnt.nbytes) < 8 * W:
            raise ValueError("counts_out holds fewer than %d uint64 words" % W)
        if dev:
            import torch
            lst = torch.empty((cap, size), dtype=torch.uint8, device="cuda") if out is None else out
            lptr, out_mem = C.c_void_p(lst.data_ptr()) if cap else None, MEM_DEVICE
            if counts:
                cnt = torch.empty(W, dtype=torch.int64, device="cuda") if cnt is None else cnt
                counts = (C.c_void_p(cnt.data_ptr()),)
        else:
            lst = np.zeros(cap, dtype=dtype) if out is None else out
            lptr, out_mem = _np_ptr(lst) if cap else None, (_ffi.MEM_HOST_PINNED if pinned and out is not None else MEM_HOST)
            if counts:
                cnt = np.empty(W, dtype=np.uint64) if cnt is None else cnt
                counts = (_np_ptr(cnt),)
        found = C.c_uint64(0)

        def result():
            k = min(found.value, cap)
            return ((lst.reshape(-1, size)[:k] if dev else lst[:k]), found.value) + ((cnt,) if counts else ())
        try:
            check(call(self._h, ptr, mem, src_first, count, first_window, n_windows, _np_ptr(t), *mins, lptr, cap, C.byref(found), *(counts or ()), out_mem, st))
        except _ffi.QuadrsError as e:
            e.partial = result()
            raise
        return result()

    def bursts(self, src, thresholds, min_len=1, cap=None, first_window=0, n_windows=None, src_first=0, pinned=False, device_out=None,
               out=None, counts_out=None):
        """qd_plan_bursts of an EPI_NORMS_F32 plan: (list, found, on_counts) — the runs of cells at or above the bin's threshold
        (a scalar, or `width` float32 in fftshifted order; NaN masks a bin) in windows [first_window, +n_windows), at least min_len long,
        in the order they end; found counts all of them, the list holds the first min(found, cap) (cap None: what cannot overflow, at
        most BURSTS_DEFAULT_CAP).  src and device_out as for bands: the list is a BURST_DTYPE numpy array, or a torch uint8 CUDA tensor
        [records, 32] with on_counts int64 (the same bits).  out / counts_out: a BURST_DTYPE array or uint8 tensor, and width uint64 words,
        to write into instead; cap then defaults to the records `out` holds and may not exceed them.  A failing call's error carries
        (list, found, on_counts) as e.partial."""
        return self._list_call(lib().qd_plan_bursts, BURST_DTYPE, _burst_cap, (int(min_len),), src, thresholds, cap, first_window, n_windows, src_first,
                               pinned, device_out, out, (counts_out,))

    def emissions(self, src, thresholds, min_len=1, min_cells=1, cap=None, first_window=0, n_windows=None, src_first=0, pinned=False,
                  device_out=None, out=None):
        """qd_plan_emissions of an EPI_NORMS_F32 plan: (list, found) — the 4-connected regions of cells at or above the bin's threshold
        (as for bursts) in windows [first_window, +n_windows), at least min_len windows long and min_cells cells large, in the order they
        end; found counts all of them, the list holds the first min(found, cap) (cap None: what cannot overflow, at most
        EMISSIONS_DEFAULT_CAP).  src and device_out as for bursts: the list is an EMISSION_DTYPE numpy array, or a torch uint8 CUDA tensor
        [records, 56].  out: an EMISSION_DTYPE array or uint8 tensor to write into instead; cap then defaults to the records `out` holds
        and may not exceed them.  A failing call's error carries (list, found) as e.partial."""
        return self._list_call(lib().qd_plan_emissions, EMISSION_DTYPE, _emission_cap, (int(min_len), int(min_cells)), src, thresholds, cap, first_window,
                               n_windows, src_first, pinned, device_out, out)

    def picture(self, src, desc, first_window=0, n_windows=None, src_first=0, pinned=False, out=None, device_out=None):
        """qd_plan_picture of an EPI_NORMS_F32 plan: (pixels uint8[px_height, px_width, 3], painted) — the waterfall picture of windows
        [first_window, +n_windows) on the page `desc` (picture_desc), top row first, and the number of windows transformed.  src as for
        pool.  out: a uint8 numpy array or torch CUDA tensor of 3 w h bytes to paint into (it is overwritten); without it the picture is
        a torch CUDA tensor when device_out (the default for a torch src), else a numpy array.  A failing call's error carries
        (pixels, painted or None) as e.partial."""
        n_windows = self.n_windows - first_window if n_windows is None else n_windows
        ptr, mem, count, st, _keep = self._src_args(src, pinned)
        shape = (desc.px_height, desc.px_width, 3)
        if out is None:
            if _is_torch(src) if device_out is None else device_out:
                import torch
                out = torch.empty(shape, dtype=torch.uint8, device="cuda")
            else:
                out = np.empty(shape, dtype=np.uint8)
        if _is_torch(out):
            optr, out_mem = C.c_void_p(out.data_ptr()), MEM_DEVICE
        else:
            optr, out_mem = _np_ptr(out), (_ffi.MEM_HOST_PINNED if pinned else MEM_HOST)
        painted = C.c_uint64(0xffffffffffffffff)
        try:
            check(lib().qd_plan_picture(self._h, ptr, mem, src_first, count, first_window, n_windows, C.byref(desc), optr, out_mem,
                                        C.byref(painted), st))
        except _ffi.QuadrsError as e:
            e.partial = (out, None if painted.value == 0xffffffffffffffff else painted.value)
            raise
        return out, painted.value

    def density(self, src, pool, level0, levels, q=(), first_window=0, n_windows=None, src_first=0, pinned=False, device_out=None, counts=True):
        """qd_plan_density of an EPI_NORMS_F32 plan: (count_rows uint32[R, width, levels], trace_rows float32[len(q), R, width]),
        R = ceil(n_windows / pool) — per bin of each group of `pool` consecutive windows of [first_window, +n_windows) the number of values
        at each of `levels` buckets of the summary's scale from bucket level0 on, and per q the lower bound of the level that holds the
        group's q-quantile (q = 0.5: the median trace).  counts=False: only the traces (count_rows is None).  src and device_out as for
        pool (a torch count_rows is int32: the same bits)."""
        qs = [float(x) for x in q]
        qa = (C.c_double * max(len(qs), 1))(*qs)
        W, L = self.width, int(levels)

        def call(h, ptr, mem, src_first, count, first_window, n_windows, pool, *rest):
            ptrs, (out_mem, st) = rest[:-2], rest[-2:]
            cptr, tptr = (ptrs[0], ptrs[1]) if counts else (None, ptrs[0])
            return lib().qd_plan_density(h, ptr, mem, src_first, count, first_window, n_windows, pool, int(level0), L, cptr, qa, len(qs),
                                         tptr if qs else None, out_mem, st)
        shapes = lambda rows: ([(rows, W, L)] if counts else []) + [(len(qs), rows, W)]      # noqa: E731
        out = self._fold_rows(call, (("uint32",) if counts else ()) + ("float32",), src, pool, first_window, n_windows, src_first, pinned,
                              device_out, shapes)
        return out if counts else (None, out[0])

    def set_timing(self, on=True):
        check(lib().qd_plan_set_timing(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        ms = C.c_float(0)
        check(lib().qd_plan_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value
