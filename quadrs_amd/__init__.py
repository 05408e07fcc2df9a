"""quadrs_amd — MI355X (gfx950) engine for quadrs' IQ-stream hot path.

The product is quadrs_amd/libquadrs_hip.so (hand-written HIP kernels behind the C ABI in
include/quadrs_hip.h).  This package is the thin Python view of that ABI used by tests and
bench.py; it mirrors the reference's operator names (from / shift / lowpass / sparkfft /
bucket / gen) and error behaviour.  It never computes on the CPU: if the HIP library is
missing, importing `quadrs_amd.engine` objects raises.
"""
from . import _ffi  # noqa: F401
from .engine import (PinnedBuffer, Plan, options_from_env, stages_geometry, rows_geometry, rows_desc, plan_options, fft_norm_batch, gen, gen_device, lowpass_block, lowpass_design, shift, shift_ratio,  # noqa: F401
                     take_fft, unpack, bits_scan, Summary, summary_init, summary_fold, summary_merge, summary_quantile, pool_init, pool_fold,
                     mean_init, mean_fold, mean_merge, mean_finish,
                     power_init, power_fold, power_merge, power_finish,
                     spread_init, spread_fold, spread_merge, spread_finish,
                     density_init, density_fold, density_merge, density_quantile, bands_fold,
                     picture_desc, picture_geometry, picture_color, picture_init, picture_fold,
                     bursts_init, bursts_fold, bursts_finish, bursts_of, BURST_DTYPE, BURSTS_DEFAULT_CAP,
                     emissions_init, emissions_fold, emissions_finish, emissions_of, EMISSION_DTYPE, EMISSIONS_DEFAULT_CAP,
                     cut_of_emission, cut_rule, cuts_geometry, cuts_run, CUT_DTYPE,
                     symbols_desc, symbols_geometry, symbols_run, cuts_symbols, SEGMENT_DTYPE,
                     window_design, WINDOW_RECT, WINDOW_BH)
from ._ffi import (MODE_EXACT, MODE_FAST, KERNEL_AUTO, KERNEL_GENERIC, KERNEL_NO_PLAN_TIME, KERNEL_SPECIALISE, MEM_DEVICE, MEM_HOST, MEM_HOST_PINNED,  # noqa: F401
                   EPI_BUCKET2_U8, EPI_CF32_BLOCKS, EPI_GLYPH_U8, EPI_MARK_U8, EPI_NORMS_F32, EPI_ROWS_F32, RowsDesc, FMT_CF32, FMT_CS16, FMT_CS8, FMT_CU8,  # noqa: F401
                   QuadrsError)
