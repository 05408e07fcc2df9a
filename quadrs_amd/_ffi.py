"""ctypes binding of include/quadrs_hip.h (the C ABI).  No torch types cross this boundary:
device buffers are passed as integer addresses (e.g. tensor.data_ptr())."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QD_LIB_PATH") or os.path.join(_HERE, "libquadrs_hip.so")   # QD_LIB_PATH: diagnostic builds

OK, ERR_INVALID, ERR_PANIC, ERR_SHORT, ERR_HIP, ERR_UNSUPPORTED = range(6)
FMT_CF32, FMT_CS8, FMT_CU8, FMT_CS16 = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE, MEM_HOST_PINNED = 0, 1, 2
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_SPECIALISE, KERNEL_NO_PLAN_TIME = 0, 1, 2, 3
MODE_EXACT, MODE_FAST = 0, 1
MAX_SHARDS = 16
EPI_NORMS_F32, EPI_GLYPH_U8, EPI_BUCKET2_U8, EPI_CF32_BLOCKS, EPI_MARK_U8, EPI_ROWS_F32 = 0, 1, 2, 3, 4, 5

# every symbol include/quadrs_hip.h declares
SYMBOLS = [
    "qd_last_error", "qd_version", "qd_device_count", "qd_set_device", "qd_pair_bytes", "qd_unpack",
    "qd_shift_ratio", "qd_shift", "qd_lowpass_design", "qd_window_design", "qd_lowpass_block", "qd_fft_norm_batch",
    "qd_plan_create", "qd_plan_destroy", "qd_plan_get_info", "qd_plan_get_taps", "qd_plan_src_range",
    "qd_plan_run", "qd_plan_set_timing", "qd_plan_last_kernel_ms", "qd_gen", "qd_take_fft",
    "qd_device_alloc", "qd_device_free", "qd_device_copy",
    "qd_set_stream", "qd_release_workspaces", "qd_plan_create_ex", "qd_plan_shard_info", "qd_plan_run_sharded",
    "qd_plan_run_sharded_device", "qd_plan_get_stats", "qd_host_alloc", "qd_host_free", "qd_host_register",
    "qd_host_unregister", "qd_plan_kernel_name", "qd_plan_create_stages", "qd_plan_get_stage_taps",
    "qd_plan_complete_windows", "qd_stages_geometry", "qd_bits_scan", "qd_rows_geometry", "qd_plan_take_fft",
    "qd_summary_init", "qd_summary_fold", "qd_summary_merge", "qd_summary_quantile", "qd_plan_summarize",
    "qd_pool_init", "qd_pool_fold", "qd_plan_pool",
    "qd_mean_init", "qd_mean_fold", "qd_mean_merge", "qd_mean_finish", "qd_plan_mean",
    "qd_power_init", "qd_power_fold", "qd_power_merge", "qd_power_finish", "qd_plan_power",
    "qd_spread_init", "qd_spread_fold", "qd_spread_merge", "qd_spread_finish", "qd_plan_spread",
    "qd_density_init", "qd_density_fold", "qd_density_merge", "qd_density_quantile", "qd_plan_density",
    "qd_bands_fold", "qd_plan_bands",
    "qd_picture_geometry", "qd_picture_color", "qd_picture_init", "qd_picture_fold", "qd_plan_picture",
    "qd_bursts_init", "qd_bursts_fold", "qd_bursts_finish", "qd_plan_bursts",
    "qd_emissions_init", "qd_emissions_fold", "qd_emissions_finish", "qd_plan_emissions",
    "qd_cuts_geometry", "qd_cuts_run", "qd_cut_of_emission",
    "qd_symbols_geometry", "qd_symbols_run", "qd_cuts_symbols",
]
SUMMARY_BUCKETS = 2048
MEAN_WORDS = 10
POWER_WORDS = 19
SPREAD_WORDS = 28
DENSITY_MAX_LEVELS, DENSITY_BUCKETS, DENSITY_MAX_Q = 256, 2041, 8
BANDS_MAX, BAND_NONE = 255, 0xffffffff
PICTURE_MAX_WORKSPACE = 1 << 30
BURSTS_WORDS, BURSTS_MAX_WORKSPACE = 3, 1 << 30
EMISSIONS_WORDS, EMISSIONS_MAX_WORKSPACE, EMISSIONS_MAX_WIDTH = 8, 1 << 30, 4096
CUT_MAX_DECIMATE, CUT_MAX_TAPS = 1024, 4096
STAGE_SHIFT, STAGE_LOWPASS = 1, 2
MAX_STAGES = 8


class ChainDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("format", C.c_int32), ("sample_rate", C.c_uint64),
        ("n_samples", C.c_uint64), ("has_shift", C.c_int32), ("_pad0", C.c_int32),
        ("shift_hz", C.c_int64), ("has_lowpass", C.c_int32), ("_pad1", C.c_int32),
        ("lowpass_hz", C.c_uint64), ("decimate", C.c_uint64), ("taps", C.c_uint64),
        ("width", C.c_uint64), ("stride", C.c_uint64), ("epilogue", C.c_int32),
        ("has_range", C.c_int32), ("range_min", C.c_float), ("range_max", C.c_float),
        ("mode", C.c_int32), ("windowing", C.c_int32),
    ]


class PlanInfo(C.Structure):
    _fields_ = [
        ("n_windows", C.c_uint64), ("decimated_len", C.c_uint64), ("out_sample_rate", C.c_uint64),
        ("out_bytes_per_window", C.c_uint64), ("raw_per_window", C.c_uint64), ("raw_step", C.c_uint64),
        ("ratio", C.c_double), ("tile_windows", C.c_uint32), ("threads", C.c_uint32),
        ("lds_bytes", C.c_uint32), ("kernel_kind", C.c_uint32), ("kernel_flags", C.c_uint32), ("_reserved", C.c_uint32),
    ]


class SpreadRows(C.Structure):
    """qd_spread_rows: the five result rows of a deviation fold; a NULL pointer is an output not asked for."""
    _fields_ = [("std_rows", C.c_void_p), ("ssd_rows", C.c_void_p), ("count_rows", C.c_void_p), ("mean_rows", C.c_void_p), ("rms_rows", C.c_void_p)]


class Band(C.Structure):
    """qd_band: fftshifted bins [lo, hi)."""
    _fields_ = [("lo", C.c_uint32), ("hi", C.c_uint32)]


class BandRows(C.Structure):
    """qd_band_rows: the six result rows of a band fold; a NULL pointer is an output not asked for."""
    _fields_ = [("level_rows", C.c_void_p), ("sum_rows", C.c_void_p), ("count_rows", C.c_void_p), ("peak_rows", C.c_void_p),
                ("peak_bin_rows", C.c_void_p), ("pick_rows", C.c_void_p)]


class PictureDesc(C.Structure):
    """qd_picture_desc: the page of a waterfall picture."""
    _fields_ = [("struct_size", C.c_uint32), ("px_width", C.c_uint32), ("px_height", C.c_uint32), ("stretch", C.c_uint32), ("scan", C.c_uint32),
                ("scale", C.c_float)]


class Cut(C.Structure):
    """qd_cut: shift, lowpass, decimation and output range [first, first + count) of one cut, 48 bytes."""
    _fields_ = [("shift_hz", C.c_int64), ("lowpass_hz", C.c_uint64), ("decimate", C.c_uint64), ("taps", C.c_uint64),
                ("first", C.c_uint64), ("count", C.c_uint64)]


class CutRule(C.Structure):
    """qd_cut_rule: how qd_cut_of_emission sizes a cut."""
    _fields_ = [("struct_size", C.c_uint32), ("guard_bins", C.c_uint32), ("oversample", C.c_uint32), ("pad", C.c_uint32),
                ("taps", C.c_uint64), ("max_decimate", C.c_uint64)]


class SymbolsDesc(C.Structure):
    """qd_symbols_desc: the sink of a symbol list, 48 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("epilogue", C.c_int32), ("width", C.c_uint64), ("stride", C.c_uint64),
                ("has_range", C.c_int32), ("range_min", C.c_float), ("windowing", C.c_int32), ("_pad", C.c_int32), ("iq_bytes", C.c_uint64)]


class Emission(C.Structure):
    """qd_emission, 56 bytes (engine.EMISSION_DTYPE is the same layout)."""
    _fields_ = [("first", C.c_uint64), ("last", C.c_uint64), ("cells", C.c_uint64), ("peak_at", C.c_uint64), ("lo", C.c_uint32), ("hi", C.c_uint32),
                ("end_bin", C.c_uint32), ("peak_bin", C.c_uint32), ("peak", C.c_float), ("flags", C.c_uint32)]


class Stage(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("_pad", C.c_int32), ("shift_hz", C.c_int64),
        ("lowpass_hz", C.c_uint64), ("decimate", C.c_uint64), ("taps", C.c_uint64),
    ]


class PlanOptions(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("kernel_policy", C.c_int32), ("nco_order", C.c_int32),
        ("copy_threads", C.c_uint32), ("chunk_bytes", C.c_uint64), ("n_shards", C.c_uint32),
        ("shard_device", C.c_int32 * MAX_SHARDS), ("tile_hint", C.c_uint32 * 8),
    ]


class ShardInfo(C.Structure):
    _fields_ = [
        ("w0", C.c_uint64), ("w1", C.c_uint64), ("own_first", C.c_uint64), ("own_count", C.c_uint64),
        ("halo", C.c_uint64), ("device", C.c_int32), ("_pad", C.c_int32),
    ]


class PlanStats(C.Structure):
    _fields_ = [
        ("wall_ms", C.c_double), ("stage_ms", C.c_double), ("bytes_h2d", C.c_uint64), ("bytes_d2h", C.c_uint64),
        ("chunks", C.c_uint32), ("_pad", C.c_uint32),
    ]


class RowsDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("has_slice", C.c_int32), ("start", C.c_uint64), ("end", C.c_uint64),
        ("output_len", C.c_uint64), ("windowing", C.c_int32), ("_pad", C.c_int32),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("width", C.c_uint32), ("n_windows", C.c_uint64), ("n_nan", C.c_uint64),
        ("min", C.c_float), ("max", C.c_float), ("hist", C.c_uint64 * SUMMARY_BUCKETS),
    ]


class QuadrsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"quadrs-hip status {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load the HIP extension.  There is no CPU fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python quadrs_amd/build.py` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # One HIP runtime per process: PyTorch bundles its own libamdhip64 (SONAME libamdhip64.so.7,
        # but its dependants ask for "libamdhip64.so"), so if this library were loaded first the
        # process would end up with two runtimes and torch tensors / streams could not be shared.
        # Importing torch first makes our DT_NEEDED libamdhip64.so.7 resolve to torch's copy.
        try:
            import torch  # noqa: F401
        except ImportError:      # a torch-less host (e.g. the C++ CLI) simply uses /opt/rocm's runtime
            pass
        L = C.CDLL(LIB_PATH)
        vp, u64, i64, sz, f32, f64, i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_size_t, C.c_float, C.c_double, C.c_int
        sig = {
            "qd_last_error": (C.c_char_p, []),
            "qd_version": (C.c_char_p, []),
            "qd_device_count": (i32, [C.POINTER(i32)]),
            "qd_set_device": (i32, [i32]),
            "qd_pair_bytes": (u64, [i32]),
            "qd_unpack": (i32, [i32, vp, sz, vp, i32]),
            "qd_shift_ratio": (f64, [i64, u64]),
            "qd_shift": (i32, [vp, sz, u64, f64, i32]),
            "qd_lowpass_design": (i32, [u64, u64, sz, vp]),
            "qd_window_design": (i32, [i32, sz, vp]),
            "qd_lowpass_block": (i32, [vp, sz, u64, vp, sz, vp, sz, C.POINTER(sz), i32]),
            "qd_fft_norm_batch": (i32, [vp, sz, sz, sz, vp, i32]),
            "qd_plan_create": (i32, [C.POINTER(ChainDesc), C.POINTER(vp)]),
            "qd_plan_destroy": (i32, [vp]),
            "qd_plan_get_info": (i32, [vp, C.POINTER(PlanInfo)]),
            "qd_plan_get_taps": (i32, [vp, vp, sz]),
            "qd_plan_kernel_name": (i32, [vp, C.c_char_p, sz]),
            "qd_plan_src_range": (i32, [vp, u64, u64, C.POINTER(u64), C.POINTER(u64)]),
            "qd_plan_run": (i32, [vp, vp, i32, u64, u64, u64, u64, vp, i32, vp]),
            "qd_plan_set_timing": (i32, [vp, i32]),
            "qd_plan_last_kernel_ms": (i32, [vp, C.POINTER(f32)]),
            "qd_gen": (i32, [vp, sz, u64, u64, sz, vp, i32]),
            "qd_device_alloc": (i32, [sz, C.POINTER(C.c_void_p)]),
            "qd_device_free": (i32, [vp]),
            "qd_device_copy": (i32, [vp, i32, vp, i32, sz]),
            "qd_take_fft": (i32, [vp, u64, sz, u64, i32, u64, u64, sz, i32, sz, vp, i32]),
            "qd_set_stream": (i32, [vp]),
            "qd_release_workspaces": (i32, []),
            "qd_plan_create_ex": (i32, [C.POINTER(ChainDesc), C.POINTER(PlanOptions), C.POINTER(vp)]),
            "qd_plan_shard_info": (i32, [vp, C.c_uint32, C.POINTER(ShardInfo)]),
            "qd_plan_run_sharded": (i32, [vp, vp, i32, vp, i32]),
            "qd_plan_run_sharded_device": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32]),
            "qd_plan_get_stats": (i32, [vp, C.POINTER(PlanStats)]),
            "qd_host_alloc": (i32, [sz, C.POINTER(vp)]),
            "qd_host_free": (i32, [vp]),
            "qd_host_register": (i32, [vp, sz]),
            "qd_host_unregister": (i32, [vp]),
            "qd_plan_create_stages": (i32, [C.POINTER(ChainDesc), C.POINTER(Stage), sz, C.POINTER(PlanOptions), C.POINTER(vp)]),
            "qd_plan_get_stage_taps": (i32, [vp, C.c_uint32, vp, sz]),
            "qd_plan_complete_windows": (i32, [vp, C.POINTER(u64)]),
            "qd_stages_geometry": (i32, [C.POINTER(ChainDesc), C.POINTER(Stage), sz, C.POINTER(PlanInfo), C.POINTER(u64)]),
            "qd_bits_scan": (i32, [vp, sz, f64, vp, sz, C.POINTER(sz), C.POINTER(f64)]),
            "qd_rows_geometry": (i32, [C.POINTER(ChainDesc), C.POINTER(RowsDesc), vp, sz, C.POINTER(u64), C.POINTER(u64)]),
            "qd_plan_take_fft": (i32, [vp, C.POINTER(RowsDesc), vp, i32, u64, u64, vp, i32, vp]),
            "qd_summary_init": (i32, [C.POINTER(Summary), vp, vp, C.c_uint32]),
            "qd_summary_fold": (i32, [C.POINTER(Summary), vp, vp, vp, u64]),
            "qd_summary_merge": (i32, [C.POINTER(Summary), vp, vp, C.POINTER(Summary), vp, vp]),
            "qd_summary_quantile": (i32, [C.POINTER(Summary), f64, C.POINTER(f32), C.POINTER(f32)]),
            "qd_plan_summarize": (i32, [vp, vp, i32, u64, u64, u64, u64, C.POINTER(Summary), vp, vp, vp]),
            "qd_pool_init": (i32, [vp, vp, C.c_uint32, u64]),
            "qd_pool_fold": (i32, [vp, vp, C.c_uint32, u64, u64, vp, u64]),
            "qd_plan_pool": (i32, [vp, vp, i32, u64, u64, u64, u64, u64, vp, vp, i32, vp]),
            "qd_mean_init": (i32, [vp, C.c_uint32, u64]),
            "qd_mean_fold": (i32, [vp, C.c_uint32, u64, u64, vp, u64]),
            "qd_mean_merge": (i32, [vp, vp, C.c_uint32, u64]),
            "qd_mean_finish": (i32, [vp, C.c_uint32, u64, vp, vp, vp]),
            "qd_plan_mean": (i32, [vp, vp, i32, u64, u64, u64, u64, u64, vp, vp, vp, i32, vp]),
            "qd_power_init": (i32, [vp, C.c_uint32, u64]),
            "qd_power_fold": (i32, [vp, C.c_uint32, u64, u64, vp, u64]),
            "qd_power_merge": (i32, [vp, vp, C.c_uint32, u64]),
            "qd_power_finish": (i32, [vp, C.c_uint32, u64, vp, vp, vp]),
            "qd_plan_power": (i32, [vp, vp, i32, u64, u64, u64, u64, u64, vp, vp, vp, i32, vp]),
            "qd_spread_init": (i32, [vp, C.c_uint32, u64]),
            "qd_spread_fold": (i32, [vp, C.c_uint32, u64, u64, vp, u64]),
            "qd_spread_merge": (i32, [vp, vp, C.c_uint32, u64]),
            "qd_spread_finish": (i32, [vp, C.c_uint32, u64, C.POINTER(SpreadRows)]),
            "qd_plan_spread": (i32, [vp, vp, i32, u64, u64, u64, u64, u64, C.POINTER(SpreadRows), i32, vp]),
            "qd_bands_fold": (i32, [vp, C.c_uint32, u64, C.POINTER(Band), C.c_uint32, C.POINTER(BandRows)]),
            "qd_plan_bands": (i32, [vp, vp, i32, u64, u64, u64, u64, C.POINTER(Band), C.c_uint32, C.POINTER(BandRows), i32, vp]),
            "qd_picture_geometry": (i32, [C.POINTER(PictureDesc), C.c_uint32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
            "qd_picture_color": (i32, [vp, sz, f32, vp]),
            "qd_picture_init": (i32, [vp, C.POINTER(PictureDesc)]),
            "qd_picture_fold": (i32, [vp, C.POINTER(PictureDesc), C.c_uint32, u64, vp, u64]),
            "qd_plan_picture": (i32, [vp, vp, i32, u64, u64, u64, u64, C.POINTER(PictureDesc), vp, i32, C.POINTER(u64), vp]),
            "qd_bursts_init": (i32, [vp, vp, C.c_uint32]),
            "qd_bursts_fold": (i32, [vp, C.c_uint32, vp, u64, u64, vp, u64, vp, u64, C.POINTER(u64), vp]),
            "qd_bursts_finish": (i32, [vp, C.c_uint32, u64, vp, u64, C.POINTER(u64)]),
            "qd_plan_bursts": (i32, [vp, vp, i32, u64, u64, u64, u64, vp, u64, vp, u64, C.POINTER(u64), vp, i32, vp]),
            "qd_emissions_init": (i32, [vp, C.c_uint32]),
            "qd_emissions_fold": (i32, [vp, C.c_uint32, vp, u64, u64, u64, vp, u64, vp, u64, C.POINTER(u64)]),
            "qd_emissions_finish": (i32, [vp, C.c_uint32, u64, u64, vp, u64, C.POINTER(u64)]),
            "qd_plan_emissions": (i32, [vp, vp, i32, u64, u64, u64, u64, vp, u64, u64, vp, u64, C.POINTER(u64), i32, vp]),
            "qd_cuts_geometry": (i32, [u64, u64, vp, sz, vp, C.POINTER(u64), C.POINTER(u64)]),
            "qd_cuts_run": (i32, [i32, u64, u64, vp, i32, u64, u64, vp, sz, vp, i32, C.POINTER(PlanOptions), vp]),
            "qd_cut_of_emission": (i32, [C.POINTER(ChainDesc), u64, C.POINTER(Emission), C.POINTER(CutRule), C.POINTER(Cut)]),
            "qd_symbols_geometry": (i32, [C.POINTER(SymbolsDesc), vp, sz, vp]),
            "qd_symbols_run": (i32, [C.POINTER(SymbolsDesc), vp, i32, u64, vp, sz, vp, i32, vp]),
            "qd_cuts_symbols": (i32, [i32, u64, u64, vp, i32, u64, u64, vp, sz, C.POINTER(SymbolsDesc), vp, i32, C.POINTER(PlanOptions), vp]),
            "qd_density_init": (i32, [vp, C.c_uint32, C.c_uint32, u64]),
            "qd_density_fold": (i32, [vp, C.c_uint32, C.c_uint32, C.c_uint32, u64, u64, vp, u64]),
            "qd_density_merge": (i32, [vp, vp, C.c_uint32, C.c_uint32, u64]),
            "qd_density_quantile": (i32, [vp, C.c_uint32, C.c_uint32, C.c_uint32, u64, f64, vp, vp, vp]),
            "qd_plan_density": (i32, [vp, vp, i32, u64, u64, u64, u64, u64, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, i32, vp]),
        }
        for name, (res, args) in sig.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                # only a diagnostic library named by QD_LIB_PATH (an older build kept for a before / after timing) may lack an entry point
                if os.environ.get("QD_LIB_PATH") and name in ("qd_plan_kernel_name",):
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != OK:
        raise QuadrsError(code, lib().qd_last_error().decode(errors="replace"))
