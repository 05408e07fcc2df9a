/*
 * quadrs_hip.h — C ABI of the MI355X (gfx950) engine for quadrs' IQ-stream hot path.
 *
 * The reference (FauxFaux/quadrs, Rust) has no FFI seam; the seam this library honours is
 * the set of constructors / sinks `Operation::exec` calls (src/lib.rs:83-175) and the
 * `Samples` sample-block iterator (src/samples.rs:11-28).  Every entry point below names
 * the reference item it replaces.  All pointers are plain C; no C++/torch types cross
 * the boundary.  Nothing here aborts or unwinds: every function returns a qd_status and
 * qd_last_error() gives a thread-local message.
 *
 * Two granularities, same kernels underneath:
 *   fine-grained  — mirrors `read_at` so shift.rs / filter.rs / fft.rs stay thin shims;
 *   coarse (plan) — one call covers a batch of FFT windows of the fused chain
 *                   unpack -> shift -> lowpass -> FFT -> |X| -> epilogue.
 *
 * Data ABI: qd_c32 == num_complex::Complex<f32> == {f32 re, f32 im}, little endian.
 */
#ifndef QUADRS_HIP_H
#define QUADRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { float re, im; } qd_c32;

typedef enum {
    QD_OK = 0,
    QD_ERR_INVALID = 1,      /* bad argument (anyhow::Error class in the reference) */
    QD_ERR_PANIC = 2,        /* the reference would panic here (assert!/unwrap/index) */
    QD_ERR_SHORT = 3,        /* read_exact_at Err: fewer samples than asked (src/samples.rs:17-27) */
    QD_ERR_HIP = 4,          /* a hip* call failed */
    QD_ERR_UNSUPPORTED = 5   /* valid in the reference, not built here yet */
} qd_status;

/* FileFormat, src/lib.rs:61-74 */
typedef enum { QD_FMT_CF32 = 0, QD_FMT_CS8 = 1, QD_FMT_CU8 = 2, QD_FMT_CS16 = 3 } qd_format;

/* where a buffer lives.  QD_MEM_HOST_PINNED: host memory the HIP runtime can DMA from / to directly — allocated by
 * qd_host_alloc, registered by qd_host_register (e.g. an mmap of the file `from` opened, src/samples.rs:51-61), or
 * pinned by the caller's own HIP runtime; the host-resident path then skips its pageable -> pinned staging copy. */
typedef enum { QD_MEM_HOST = 0, QD_MEM_DEVICE = 1, QD_MEM_HOST_PINNED = 2 } qd_mem;

/* what the fused chain leaves per FFT window */
typedef enum {
    QD_EPI_NORMS_F32 = 0,    /* W f32: hypot(re,im) in fftshift order (src/fft.rs:48-53) */
    QD_EPI_GLYPH_U8 = 1,     /* W u8: 0=' ' 1..7='▁'..'▇' 8='█' 255=reference would panic (src/fft.rs:54-60) */
    QD_EPI_BUCKET2_U8 = 2,   /* 1 u8: freq_levels digit (src/fft.rs:95-97) */
    QD_EPI_CF32_BLOCKS = 3,  /* the write sink (do_write, src/lib.rs:199-210): no FFT; a "window" is one full
                                LowPass::read_at block of `width` decimated samples (0x1000 for do_write, a power
                                of two), `stride` is ignored, the output is width qd_c32 per block with the block's
                                own tail truncation.  n_windows counts the FULL blocks, floor((n-T)/(width*D));
                                the ragged end of the stream is left to qd_lowpass_block.  Needs has_lowpass.
                                Behind a cascade (qd_plan_create_stages) a block is the outer read_at(b*width, width)
                                of the nested stages, every stage truncating against its own read of it; n_windows
                                counts the blocks whose source span fits the stream (see the stage lists below). */
    QD_EPI_MARK_U8 = 4,      /* 1 u8 per spark_fft window (the loop of src/fft.rs:28,65: n_windows and qd_plan_src_range are the glyph
                                sink's): 0 when the reference would print the row blank, i.e. every bin has norm < min in f32
                                (src/fft.rs:54-55; min = range_min with has_range, else 0.08f; range_max plays no part), 1 otherwise.
                                A NaN norm or a NaN min compares false: 1.  Equivalently any(code != 0) over the W codes of
                                QD_EPI_GLYPH_U8 for the same plan parameters: the blank / not-blank step of the README's "OOK in
                                sed" example, the input of qd_bits_scan.  Needs no lowpass, takes any stride. */
    QD_EPI_ROWS_F32 = 5      /* take_fft's rows behind the chain (src/ffts.rs:18-85): W f32 per row, fftshifted norms.  width = W, any W >= 1: a
                                power of two runs the chain kernel over rows at irregular offsets, every other width up to 4096 the Bluestein
                                kernel (larger ones: QD_ERR_UNSUPPORTED); stride, has_range and range_* are ignored.  The plan has no window
                                loop of its own — n_windows = 0, out_bytes_per_window = 4 W, raw_per_window = W*D + T — and is run by
                                qd_plan_take_fft (see there); qd_plan_run, qd_plan_src_range, qd_plan_run_sharded* and
                                qd_plan_complete_windows return QD_ERR_INVALID on it.  A row whose source span W*D + T does not fit the
                                160 KiB LDS tile is QD_ERR_UNSUPPORTED at plan creation, and so is this sink behind a cascade
                                (qd_plan_create_stages; a [shift] [lowpass] list is the one-stage plan as for every sink). */
} qd_epilogue;

const char *qd_last_error(void);
const char *qd_version(void);
int qd_device_count(int *count);
int qd_set_device(int device);

/* Stream (a hipStream_t, may be NULL) the fine-grained calls of THIS thread enqueue on; with QD_MEM_DEVICE buffers they
 * then return without synchronising (stream order is the only ordering), with host buffers they return after the
 * copy back.  Temporaries come from a process-wide workspace pool (no hipMalloc / hipFree per call);
 * qd_release_workspaces frees the pool's idle buffers and cached plans. */
int qd_set_stream(void *stream);
int qd_release_workspaces(void);

/* ------------------------------------------------------------------ fine-grained */

/* FileFormat::pair_bytes, src/lib.rs:226-229 */
uint64_t qd_pair_bytes(int fmt);

/* FileFormat::to_cf32 over a block — the loop at src/samples.rs:85-90 (bit-exact). */
int qd_unpack(int fmt, const void *bytes, size_t n_pairs, qd_c32 *out, int mem);

/* Shift::new's ratio, src/shift.rs:28 (host arithmetic, f64). */
double qd_shift_ratio(int64_t frequency, uint64_t sample_rate);

/* Shift::read_at's loop, src/shift.rs:48-52: buf[i] *= e^{+i (abs_off+i)*ratio}, in place;
 * abs_off is the absolute index of buf[0] in the stream (the NCO phase depends on it). */
int qd_shift(qd_c32 *buf, size_t n, uint64_t abs_off, double ratio, int mem);

/* lowpass_filter(cutoff_from_frequency(f, sr) as f32, size), src/filter.rs:29-31,86-105,126-128.
 * Host arithmetic with the platform libm, exactly as the reference does it (O(size), once). */
int qd_lowpass_design(uint64_t frequency, uint64_t sample_rate, size_t size, float *taps);

/* The W-float table of a window (qd_chain_desc.windowing, qd_rows_desc.windowing, qd_take_fft): 1 is
 * generate_blackman_harris_window, src/ffts.rs:110-119, in f32 with the platform cosf like the reference; 0 is ones.
 * Host arithmetic only.  Any other windowing: QD_ERR_INVALID. */
int qd_window_design(int windowing, size_t W, float *w);

/* bits::scan, src/bits.rs:3-55 (host arithmetic, f64): run-length decode n marks (0 / non-0, e.g. a QD_EPI_MARK_U8 output) at
 * `scale` marks per bit.  half = round(scale / 2) (halves away from zero); a run of the expected value (0 first, flipping after every
 * accepted run) ends where the first stretch of more than `half` wrong values began; an accepted run (longer than half) emits
 * round(run / scale) copies of the value into bits[] (0 / 1) and adds |run / scale - rounded| to *error, in order.
 * QD_ERR_PANIC: a run of at most `half` ends before the end of the data — the reference `continue`s without flipping (:9-15), its next
 * run_of returns 0 and the loop never ends; *produced and *error hold what had been emitted up to there.
 * QD_ERR_INVALID: scale not finite or <= 0; or more than `cap` bits, with *produced = the count needed (bits[] holds the first cap;
 * this outranks QD_ERR_PANIC). */
int qd_bits_scan(const uint8_t *marks, size_t n, double scale, uint8_t *bits, size_t cap, size_t *produced, double *error);

/* LowPass::read_at on an already fetched raw block, src/filter.rs:68-83 + complex_convolve
 * :107-124: out[k] = sum_{j<jmax(k)} raw[k*D + c + j]*taps[j], c = T - T/2,
 * jmax = min(T, valid - (k*D + c)); *produced = (valid - T)/D.  QD_ERR_PANIC if valid < T
 * or out_cap < *produced.  Same products, same ascending-j order, no FMA. */
int qd_lowpass_block(const float *taps, size_t T, uint64_t D, const qd_c32 *raw, size_t valid,
                     qd_c32 *out, size_t out_cap, size_t *produced, int mem);

/* Radix4::new(W, Forward) + process + fftshift + norm for n_fft windows, window i starting
 * at in[i*in_stride] (src/fft.rs:25,32,48-53).  norms: n_fft*W f32. */
int qd_fft_norm_batch(const qd_c32 *in, size_t W, size_t n_fft, size_t in_stride, float *norms, int mem);

/* take_fft, src/ffts.rs:18-85 (the spectrogram rows of the egui front end): output_len rows at
 * sample start + round(step*i), step = (end-start)/output_len in f64; optional Blackman-Harris
 * window (windowing 1; src/ffts.rs:110-119, host f32 arithmetic like the reference); forward FFT;
 * fftshifted norms into rows[output_len*W].  `in` holds samples [in_first, in_first+n_in) of the
 * cf32 Samples being viewed, whose len() is samples_len.  has_slice 0 => (0, len - W) (:27-30).
 * Any W: a power of two goes through the chain kernel's Radix4 (bit-exact against the oracle's restatement); every other
 * width up to 4096 (the front end's slider range, src/eui/mod.rs:157) through a Bluestein kernel carried in f64 — rustfft's
 * result for those lengths depends on its planner and host SIMD path (parity unpinned), so the bins are the exact DFT of
 * the windowed f32 samples rounded once to f32.
 * QD_ERR_PANIC / QD_ERR_INVALID mirror the asserts / ensure! at :32-48. */
int qd_take_fft(const qd_c32 *in, uint64_t in_first, size_t n_in, uint64_t samples_len, int has_slice,
                uint64_t start, uint64_t end, size_t W, int windowing, size_t output_len, float *rows, int mem);

/* ------------------------------------------------------------------ coarse-grained plan */

typedef struct qd_plan qd_plan;

typedef struct {
    uint32_t struct_size;     /* sizeof(qd_chain_desc) */
    int32_t  format;          /* qd_format of the source bytes (Operation::From, src/lib.rs:89-96) */
    uint64_t sample_rate;     /* of the source */
    uint64_t n_samples;       /* Samples::len() of the source: the whole stream, absolute indexing */
    int32_t  has_shift;       /* Operation::Shift, src/lib.rs:102-106 */
    int32_t  _pad0;
    int64_t  shift_hz;
    int32_t  has_lowpass;     /* Operation::LowPass, src/lib.rs:107-121 */
    int32_t  _pad1;
    uint64_t lowpass_hz;
    uint64_t decimate;
    uint64_t taps;            /* `size`: 2*power, default 40 (src/args.rs:161-166) */
    uint64_t width;           /* Operation::SparkFft / Bucket, src/lib.rs:122-160 */
    uint64_t stride;
    int32_t  epilogue;        /* qd_epilogue */
    int32_t  has_range;       /* sparkfft -range min:max; else 0.08 / 1.0 (src/fft.rs:22-23) */
    float    range_min, range_max;
    int32_t  mode;            /* qd_mode: QD_MODE_EXACT (0, the default: the reference's products, order and roundings) or QD_MODE_FAST */
    int32_t  windowing;       /* the window of the FFT sinks (NORMS_F32, GLYPH_U8, BUCKET2_U8, MARK_U8): 0 rectangular (none), 1 Blackman-Harris —
                                 sink sample k of every window is multiplied by qd_window_design(1, width)[k] as Complex<f32> * f32 (two
                                 separately rounded products, src/ffts.rs:64-68) behind the lowpass (truncated tail outputs included) and any
                                 shift, in front of the forward FFT; nothing else of the chain changes.  Any other value: QD_ERR_INVALID;
                                 non-zero with QD_EPI_CF32_BLOCKS (no transform): QD_ERR_INVALID; ignored by QD_EPI_ROWS_F32 (qd_rows_desc's
                                 window).  No geometry (qd_plan_info, qd_plan_src_range, qd_stages_geometry, qd_rows_geometry) depends on it. */
} qd_chain_desc;

/* QD_MODE_FAST is a PERMISSION, never the default and never what bench.py's `value` is measured in: the FIR may fuse each
 * multiply with its add (v_pk_fma_f32: one rounding per tap instead of two, same ascending-tap order), which breaks the
 * "within 1 ulp of the reference" bound of the exact mode — outputs stay within a few ulp of the window maximum of it and are, if
 * anything, closer to the infinitely precise filter.  Everything else (unpack, NCO, FFT, |X|) is unchanged.  Kernels without a
 * fused form (runtime-geometry kernels, overlapping windows, short filters) run the exact arithmetic: qd_plan_info.kernel_flags
 * bit 14 says whether the plan's kernel fuses. */
typedef enum { QD_MODE_EXACT = 0, QD_MODE_FAST = 1 } qd_mode;

typedef struct {
    uint64_t n_windows;       /* trip count of the sink's loop: spark_fft `while i < len - W`
                                 (src/fft.rs:28,65) or freq_levels `(len - W)/S` (src/fft.rs:86) */
    uint64_t decimated_len;   /* Samples::len() seen by the sink (LowPass::len, src/filter.rs:45-48) */
    uint64_t out_sample_rate; /* Samples::sample_rate() seen by the sink */
    uint64_t out_bytes_per_window;
    uint64_t raw_per_window;  /* W*D + T source samples one window reads */
    uint64_t raw_step;        /* S*D source samples between window starts */
    double   ratio;           /* Shift ratio (0 if no shift) */
    uint32_t tile_windows;    /* windows per workgroup tile (overlapping lowpass-free windows served by interleaved launches: any range; ranges starting on multiples of this keep the fast path) */
    uint32_t threads;         /* workgroup size */
    uint32_t lds_bytes;
    uint32_t kernel_kind;     /* 0 generic (runtime geometry), 1 built-in shape-specialised, 2 specialised at plan time (hiprtc) */
    uint32_t kernel_flags;    /* variant bits of the main kernel (0 for the generic kernels): 4 packed lane-per-output FIR, 8 row-aligned
                                 phase 1, 32 straight-line shared FIR, 64 deferred FFT, 128 packed two-output FIR, 256 non-temporal stream loads (65536: only rows no other tile reads), 8192 half-window tiles, 16384 fused FIR (QD_MODE_FAST),
                                 32768 three-stage kernel (producer / FIR / FFT waves on consecutive tiles), 131072 its streaming form (runs of tiles, state carried in LDS), 262144 the streaming kernel as the write sink (QD_EPI_CF32_BLOCKS: producers + FIR waves, no FFT stage),
                                 524288 the wave-local kernel of chains WITHOUT a lowpass (stride == width: one wave per tile, no workgroup barriers), 1048576 its form with the base butterflies out of the row registers (W = 128 ... 1024; plan-time builds), 2097152 overlapping windows of 2 ... 8 points, a window per lane (plan-time builds),
                                 4194304 applies the plan's window (qd_chain_desc.windowing; plan-time builds of k_chain);
                                 chosen from the chain's geometry at plan time (built-in kernels: the same predicates, fixed at build time) */
    uint32_t _reserved;
} qd_plan_info;

/* How a plan picks its kernel and moves host-resident streams.  An explicit struct: the shipped library reads no tuning
 * environment variables (only the location of its on-disk code-object cache: QD_JIT_CACHE / XDG_CACHE_HOME / HOME). */
typedef enum {
    QD_KERNEL_AUTO = 0,          /* built-in shape-specialised kernel if one matches, else a cached / worthwhile plan-time build, else generic */
    QD_KERNEL_GENERIC = 1,       /* runtime-geometry kernels only */
    QD_KERNEL_SPECIALISE = 2,    /* always specialise at plan time (hiprtc) when no built-in kernel matches */
    QD_KERNEL_NO_PLAN_TIME = 3   /* built-in or generic; never hiprtc */
} qd_kernel_policy;

#define QD_MAX_SHARDS 16

typedef struct {
    uint32_t struct_size;        /* sizeof(qd_plan_options) */
    int32_t  kernel_policy;      /* qd_kernel_policy */
    int32_t  nco_order;          /* 0: chosen from |ratio|*n_samples; 1 / 2: force the first / second order NCO correction */
    uint32_t copy_threads;       /* host threads of the pageable -> pinned staging copy (QD_MEM_HOST); 0: up to 8 */
    uint64_t chunk_bytes;        /* source bytes per chunk of the host-resident path; 0: 64 MiB */
    uint32_t n_shards;           /* qd_plan_run_sharded*: number of window-range shards; 0 or 1: the current device only */
    int32_t  shard_device[QD_MAX_SHARDS];   /* HIP device of shard g (a device may serve several shards) */
    uint32_t tile_hint[8];       /* tuning: force a plan-time build with this tiling — windows per tile, threads (256 /
                                    512 / 1024), FIR outputs per lane, FIR block taps, waves per SIMD the build is register-
                                    budgeted for, LDS pad elements per row (1 / 2), FFT slots (tiles per FFT batch; 2 with the
                                    deferred FFT) in bits 0-7 of slot 6 and the kernel variant bits above them (4 packed
                                    lane-per-output FIR, 8 row-aligned phase 1, 32 straight-line shared FIR, 64 deferred FFT, 128
                                    packed two-output tile FIR, 256 non-temporal stream loads, 8192 half-window tiles, 16384 fused
                                    multiply-add, 32768 three-stage kernel, 65536 shared rows at the default cache policy, 131072
                                    its streaming form, 262144 the write sink's; a bit a shape cannot take is ignored; bits 1, 2,
                                    16, 512, 1024, 2048 and 4096 are reserved and a hint that carries one is refused with
                                    QD_ERR_INVALID), workgroups per CU; all 0: the library's own choice.
                                    Every variant of one workgroup size computes the same bytes; with a shift stage, tilings of different workgroup
                                    size may round ~1e-8 of the NCO multipliers the other way (DESIGN.md sections 3.1, 4) */
} qd_plan_options;

int qd_plan_create(const qd_chain_desc *desc, qd_plan **plan);
int qd_plan_create_ex(const qd_chain_desc *desc, const qd_plan_options *options, qd_plan **plan);
int qd_plan_destroy(qd_plan *plan);
int qd_plan_get_info(const qd_plan *plan, qd_plan_info *info);
/* taps the plan designed (T floats), for inspection */
int qd_plan_get_taps(const qd_plan *plan, float *taps, size_t cap);
/* the main kernel's name as a profiler lists it (template name with its geometry, e.g. "qd::k_chain_pipe3s<0, 1, FixedGeo<64, 16, 32, 400, 14, ...>, ...>"),
 * NUL-terminated into buf[cap]; reporting only (bench.py's roofline.kernel) */
int qd_plan_kernel_name(const qd_plan *plan, char *buf, size_t cap);

/* source samples [*first, *first + *count) that windows [first_window, first_window+n) read */
int qd_plan_src_range(const qd_plan *plan, uint64_t first_window, uint64_t n_windows,
                      uint64_t *first, uint64_t *count);

/* Run windows [first_window, first_window + n_windows) of the sink's loop.
 * src holds the raw bytes of source samples [src_first, src_first + src_count) (a slab of the
 * stream; absolute sample indices keep the NCO phase identical to a whole-stream run).
 * out receives n_windows * out_bytes_per_window bytes.
 * Device buffers: the kernels are enqueued on `stream` (a hipStream_t, may be NULL) and the
 * call returns without synchronising.  Host buffers: chunked, double-buffered
 * hipMemcpyAsync in and out; returns after the last copy completed.  QD_MEM_HOST goes through a
 * pinned staging ring (a multi-threaded memcpy each way); QD_MEM_HOST_PINNED is copied from / to
 * directly.  src and out may be HOST and HOST_PINNED in any combination. */
int qd_plan_run(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                uint64_t first_window, uint64_t n_windows, void *out, int out_mem, void *stream);

/* Multi-GPU in one process (no Python, no collective).  The sink's windows are split into n_shards contiguous,
 * tile-aligned ranges (the reference's sink loop src/fft.rs:28-65 has no cross-window state); shard g runs on
 * options.shard_device[g] on its own streams, and the outputs concatenate to exactly the bytes of a one-device run.
 *   qd_plan_shard_info     window range and source range of shard g: it OWNS samples [own_first, +own_count) (disjoint,
 *                          in order) and additionally reads `halo` = (W-S)*D+T samples that the next shard owns.
 *   qd_plan_run_sharded    host-resident stream (QD_MEM_HOST / QD_MEM_HOST_PINNED): every shard's chunks, halo included,
 *                          are copied straight from the host buffer — the "host-side halo" of SURVEY section 5; one
 *                          host thread per shard drives that device's double-buffered ring.  Returns when all are done.
 *   qd_plan_run_sharded_device  device-resident, pre-split stream: slabs[g] is a buffer ON shard g's device that holds
 *                          the samples shard g owns and has room for `halo` more behind them; the halo is fetched from
 *                          the next shard's slab with hipMemcpyPeerAsync (xGMI when the devices differ), then the chain
 *                          runs; outs[g] (on the same device) receives that shard's windows.  sync != 0 waits for all.
 */
typedef struct {
    uint64_t w0, w1;             /* windows [w0, w1) of the sink's loop */
    uint64_t own_first, own_count, halo;
    int32_t  device;
    int32_t  _pad;
} qd_shard_info;
int qd_plan_shard_info(const qd_plan *plan, uint32_t shard, qd_shard_info *info);
int qd_plan_run_sharded(qd_plan *plan, const void *src, int src_mem, void *out, int out_mem);
int qd_plan_run_sharded_device(qd_plan *plan, void *const *slabs, void *const *outs, int sync);

/* ------------------------------------------------------------------ stage lists (cascades)
 *
 * The CLI grammar takes `shift` and `lowpass` in any order and number (src/args.rs:19-45); Operation::exec nests them
 * (src/lib.rs:83-175).  qd_chain_desc holds at most one shift ahead of at most one lowpass; a stage list describes the rest.
 * Each stage is validated at ITS OWN input rate, in list order, with the one-stage plan's codes: a shift with
 * |f| >= rate / 2 (src/shift.rs:20-24), decimate 0, taps < 2 and inner len < taps (src/filter.rs:45-48,74) are QD_ERR_PANIC,
 * and so is a sink len < width.  A lowpass's taps are designed for its input rate; its output rate is rate / decimate
 * (integer division, src/filter.rs:51).
 *   [shift] [lowpass]                     routed to the one-stage plan (qd_plan_create_ex): the same kernels, bytes and name;
 *   [shift] lowpass [shift] [lowpass [shift]]  otherwise (e.g. `lowpass shift`, `lowpass lowpass`, `shift lowpass shift
 *                                         lowpass shift`): the fused cascade kernel.  Its envelope: an intermediate block of
 *                                         W*D2 + T2 <= 8192 samples per window (W without a second lowpass), a first stage of
 *                                         at most 4096 taps, any stride; the window's source span (W*D2 + T2)*D1 + T1 is
 *                                         streamed through the workgroup in sub-tiles.  QD_MODE_FAST runs its exact arithmetic.
 *                                         The write sink (QD_EPI_CF32_BLOCKS) runs on its own kernel: read_at blocks of
 *                                         B = width outer outputs (a power of two up to 2^20, stride ignored), computed in
 *                                         sub-blocks; its envelope is a first stage of at most 4096 taps, a second of at most
 *                                         8192, and a block source span (B*D2 + T2)*D1 + T1 of at most 2^31 samples — there
 *                                         is no W*D2 + T2 limit.  n_windows = complete = the full blocks (the ragged end is the
 *                                         caller's), out_bytes_per_window = 8*B, raw_step = B*D2*D1.
 *   anything else (three lowpasses, two shifts in a row, shift-only cascades, a block past the envelope): QD_ERR_UNSUPPORTED;
 *   a write sink without a lowpass (an empty list or a lone shift): QD_ERR_INVALID.
 * A cascade plan's qd_plan_info composes through the stages: raw_per_window / raw_step are the source span / step of a
 * window, decimated_len / out_sample_rate are the sink's, ratio is the first shift's.  qd_plan_src_range, qd_plan_run
 * (device buffers, host buffers in chunks, slabs, window sub-ranges) and qd_plan_run_sharded (any shard devices) work and give
 * the bytes of the whole-stream run, for every sink; qd_plan_run_sharded_device returns QD_ERR_UNSUPPORTED.
 * With two lowpass stages LowPass::len over-reports (src/filter.rs:45-48) and the sink's last window(s) may fail
 * read_exact_at (src/samples.rs:17-27): qd_plan_complete_windows gives the leading windows that succeed, and a run whose range
 * reaches past them writes every complete window of the range and returns QD_ERR_SHORT. */
typedef enum { QD_STAGE_SHIFT = 1, QD_STAGE_LOWPASS = 2 } qd_stage_kind;
typedef struct {                 /* one Operation::Shift / Operation::LowPass, src/lib.rs:102-121 */
    int32_t  kind;               /* qd_stage_kind */
    int32_t  _pad;
    int64_t  shift_hz;           /* QD_STAGE_SHIFT */
    uint64_t lowpass_hz, decimate, taps;   /* QD_STAGE_LOWPASS */
} qd_stage;
#define QD_MAX_STAGES 8
/* desc: source and sink fields (has_shift = has_lowpass = 0, else QD_ERR_INVALID); stages in source-to-sink order */
int qd_plan_create_stages(const qd_chain_desc *desc, const qd_stage *stages, size_t n_stages,
                          const qd_plan_options *options, qd_plan **plan);
/* taps of lowpass stage `stage` (an index into the plan's stage list); QD_ERR_INVALID for a shift stage */
int qd_plan_get_stage_taps(const qd_plan *plan, uint32_t stage, float *taps, size_t cap);
/* leading windows of the sink's loop whose read_exact_at succeeds (== n_windows for every one-stage plan) */
int qd_plan_complete_windows(const qd_plan *plan, uint64_t *n);
/* host arithmetic only (no device): validates like qd_plan_create_stages and fills n_windows, decimated_len, out_sample_rate,
 * out_bytes_per_window, raw_per_window, raw_step and ratio of the plan it would make (other fields 0), and *complete its
 * qd_plan_complete_windows */
int qd_stages_geometry(const qd_chain_desc *desc, const qd_stage *stages, size_t n_stages, qd_plan_info *info, uint64_t *complete);

/* ------------------------------------------------------------------ spectrogram rows (take_fft) behind a chain
 *
 * take_fft(&dyn Samples, ...) (src/ffts.rs:18-85) over the fused chain  from -> [shift] -> [lowpass]  of a QD_EPI_ROWS_F32 plan: output_len
 * rows at sample start + round(step*i) of the SINK's stream (decimated samples behind a lowpass), step = (end-start)/output_len in f64,
 * each the W-point forward FFT of the samples a read_exact_at(offset, W) of the chain returns — a LowPass truncates the row's last
 * outputs against the row's own read (src/filter.rs:68-83) —, under a Blackman-Harris window (windowing 1) or none (0). */
typedef struct {
    uint32_t struct_size;     /* sizeof(qd_rows_desc) */
    int32_t  has_slice;       /* 0: (0, len - W), src/ffts.rs:27-30 */
    uint64_t start, end;      /* the slice, in the sink's samples */
    uint64_t output_len;
    int32_t  windowing;       /* 0 rectangular, 1 Blackman-Harris (src/ffts.rs:110-119) */
    int32_t  _pad;
} qd_rows_desc;

/* Host arithmetic only (no device): validates the chain of desc (its has_shift / has_lowpass fields; width = W, the epilogue is not looked
 * at) with the plan's codes, applies src/ffts.rs:27-48 against the sink's len() with qd_take_fft's codes (QD_ERR_PANIC for the two asserts
 * and the len < W underflow, QD_ERR_INVALID for the ensure!), writes offsets[i] = start + round(step*i) (cap >= output_len entries, else
 * QD_ERR_INVALID) and the source range [*src_first, +*src_count) the rows read: row i reads source samples [off_i*D, off_i*D + W*D + T)
 * ([off_i, off_i + W) without a lowpass).  QD_ERR_SHORT, naming the row, when a row's read_exact_at would fail, i.e. its source span does
 * not fit n_samples: LowPass::len over-reports by one (src/filter.rs:45-48), so a slice that passes the asserts can still end here. */
int qd_rows_geometry(const qd_chain_desc *desc, const qd_rows_desc *rows, uint64_t *offsets, size_t cap, uint64_t *src_first, uint64_t *src_count);

/* The rows of a QD_EPI_ROWS_F32 plan: output_len * W f32 into `rows`, row-major.  src holds the raw bytes of source samples
 * [src_first, src_first + src_count), a slab of the stream that covers every row's span (absolute indices keep the NCO phase); the checks
 * are qd_rows_geometry's plus QD_ERR_SHORT for a row that is not inside the slab.  Device / host / pinned buffers and `stream` as for
 * qd_plan_run: device buffers are enqueued on `stream` and the call returns without waiting for the kernels; host buffers return after the
 * copy back.  Only the slab is read — of a host slab only the stretch the rows span is copied up, in one piece — and only
 * output_len * 4 * W bytes are written.  output_len == 0 is QD_OK. */
int qd_plan_take_fft(qd_plan *plan, const qd_rows_desc *rows_desc, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                     float *rows, int out_mem, void *stream);

/* ------------------------------------------------------------------ the folds of a norms plan
 *
 * The eight sections from here to the waterfall pictures fold the windows of a QD_EPI_NORMS_F32 plan on the device: qd_plan_summarize,
 * _pool, _mean, _power, _spread, _density, _bands and _picture.  THE FOOTPRINT they share: of `src` only qd_plan_src_range of the
 * windows the call transforms is read (all of [first_window, +n_windows); for a picture those its page looks at); only the outputs asked
 * for are written, each over exactly its stated size; all device work is ordered on `stream`; and the results are complete on return,
 * for device outputs too.  tests/test_gpu_fold_footprint.py and tests/test_gpu_fold_streams.py hold every fold to it. */

/* ------------------------------------------------------------------ level summary of a norms plan
 *
 * What `-range` to pass and where in the band the signal sits, without bringing the norms back: FftResult::max / min
 * (src/ffts.rs:101-107) and the `min max` line of ui::render (src/ui/mod.rs:317-409), per bin and as a histogram.  The summary is defined
 * over windows [w0, w0+n) of a QD_EPI_NORMS_F32 plan of width W and folds exactly the f32 values the norms sink writes for them, in
 * fftshifted bin order:
 *   peak[b]   fold of f32::max from 0.0 over the windows, b < W (a NaN is ignored, as f32::max does)
 *   floor[b]  fold of f32::min from +inf (a NaN is ignored)
 *   max, min  the same folds over every bin: the max of peak, the min of floor
 *   hist[i]   values with bits(|x|) >> 20 == i: 8 buckets per octave; zero and the subnormals in bucket 0, +inf in 2040, 2041..2047 stay 0
 *   n_nan     NaN values;  sum(hist) + n_nan == n_windows * W
 * Every field is a max, a min or an integer sum: the result does not depend on the batch, chunk, shard or launch order it was folded
 * in, and parts merge (qd_summary_merge) to exactly the whole.  The values are norms: non-negative or NaN. */
typedef struct {
    uint32_t struct_size;     /* sizeof(qd_summary); qd_summary_init sets it */
    uint32_t width;           /* W */
    uint64_t n_windows;
    uint64_t n_nan;
    float    min, max;
    uint64_t hist[2048];
} qd_summary;

/* The fold identities: no windows, max = 0.0, min = +inf, peak[b] = 0.0, floor[b] = +inf.  peak and floor are caller-owned arrays of
 * `width` f32, here and below; either may be NULL (that fold is then not kept). */
int qd_summary_init(qd_summary *sum, float *peak, float *floor, uint32_t width);
/* Fold n_rows rows of sum->width host f32 (e.g. a qd_plan_run output) into sum / peak / floor: the CPU twin of the kernel behind
 * qd_plan_summarize, bit for bit. */
int qd_summary_fold(qd_summary *sum, float *peak, float *floor, const float *norms, uint64_t n_rows);
/* dst (+)= src: associative and commutative.  QD_ERR_INVALID: different widths, or a dst array without its src array. */
int qd_summary_merge(qd_summary *dst, float *dst_peak, float *dst_floor, const qd_summary *src, const float *src_peak, const float *src_floor);
/* The bucket of the q-quantile (host arithmetic): N = sum(hist), r = max(1, ceil(q N)), j the first bucket whose cumulative count
 * reaches r; the r-th smallest non-NaN value lies in [*lo, *hi), *lo the f32 of bits j << 20, *hi of (j + 1) << 20 (+inf for j = 2040).
 * QD_ERR_INVALID: N == 0 or q outside [0, 1]. */
int qd_summary_quantile(const qd_summary *sum, double q, float *lo, float *hi);

/* The summary of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; src, src_mem, src_first, src_count and `stream` as for
 * qd_plan_run (device, host and pinned sources).  sum, peak and floor are HOST memory and are OVERWRITTEN, not accumulated; the call
 * returns after the result is there.  The windows go batch by batch through the plan's own kernel into a device carrier of at most
 * max(chunk_bytes, one tile of windows) of norms and are folded there; only the summary comes back.
 * Codes as qd_plan_run: QD_ERR_SHORT past the sink's loop (the identities are left), and for a cascade's range past
 * qd_plan_complete_windows (the complete windows of the range are folded, n_windows says how many).  QD_ERR_INVALID for any epilogue
 * other than QD_EPI_NORMS_F32, QD_ERR_UNSUPPORTED for a plan created with shards (summarise each shard's window range on a plan of its
 * own and qd_summary_merge them).  n_windows == 0: QD_OK and the identities. */
int qd_plan_summarize(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                      uint64_t first_window, uint64_t n_windows, qd_summary *sum, float *peak, float *floor, void *stream);

/* ------------------------------------------------------------------ peak-hold rows of a norms plan
 *
 * A spectrum analyser's "max hold" picture of a whole capture: every window is transformed and each group of `pool` consecutive
 * windows is folded per bin into one row.  Over windows [w0, w0+n) of a QD_EPI_NORMS_F32 plan of width W there are R = ceil(n / pool)
 * rows of W f32; row r folds windows [w0 + r pool, min(w0 + (r+1) pool, w0 + n)) — the last row may be ragged — of exactly the f32
 * values the norms sink writes, in fftshifted bin order, by the rules of the summary's peak / floor:
 *   peak_rows[r W + b]   fold of f32::max from 0.0 (a NaN is ignored)
 *   floor_rows[r W + b]  fold of f32::min from +inf (a NaN is ignored)
 * Max and min do not depend on the batch, chunk or launch order they were folded in.  pool >= n: one row, qd_plan_summarize's peak /
 * floor bit for bit; pool == 1: the norms themselves wherever they are not NaN.  Either array may be NULL (that fold is not kept). */

/* The fold identities: peak rows 0.0, floor rows +inf, `rows` rows of `width` host f32 each. */
int qd_pool_init(float *peak_rows, float *floor_rows, uint32_t width, uint64_t rows);
/* The CPU twin of the kernel behind qd_plan_pool, bit for bit: windows at, at+1, ... at+n-1 of a range (n rows of `width` host f32 in
 * `norms`) ACCUMULATE into rows (at + i) / pool of peak_rows / floor_rows, which hold the range's rows from row 0 on.  Parts of a
 * range folded in any order give the whole.  QD_ERR_INVALID: pool == 0, width == 0, both arrays NULL, or norms NULL with n > 0. */
int qd_pool_fold(float *peak_rows, float *floor_rows, uint32_t width, uint64_t pool, uint64_t at,
                 const float *norms, uint64_t n);
/* The pooled rows of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; src, src_mem, src_first, src_count and `stream`
 * as for qd_plan_run (device, host and pinned sources).  peak_rows / floor_rows are R W f32 each of out_mem memory (host, pinned or
 * device; either may be NULL, not both) and are OVERWRITTEN, not accumulated; the call returns after they are complete.  The windows
 * go batch by batch through the plan's own kernel into a device carrier of at most max(chunk_bytes, one tile of windows) of norms and
 * are folded there into an accumulator of R W words per output: the caller's arrays themselves when out_mem is device memory, else a
 * workspace that is copied down once.
 * Codes as qd_plan_summarize: QD_ERR_INVALID for any epilogue other than QD_EPI_NORMS_F32, pool == 0, both outputs NULL or an unknown
 * memory kind; QD_ERR_SHORT past the sink's loop (the outputs are not touched), and for a cascade's range past
 * qd_plan_complete_windows (every complete window of the range is folded; rows without one hold the identities);
 * QD_ERR_UNSUPPORTED for a plan created with shards (give each device a contiguous range of ROWS on a plan of its own).
 * n_windows == 0: QD_OK, nothing is touched. */
int qd_plan_pool(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                 uint64_t first_window, uint64_t n_windows, uint64_t pool,
                 float *peak_rows, float *floor_rows, int out_mem, void *stream);

/* ------------------------------------------------------------------ average-trace rows of a norms plan
 *
 * The spectrum analyser's third trace next to max hold and min hold: over windows [w0, w0+n) of a QD_EPI_NORMS_F32 plan of width W and
 * R = ceil(n / pool) rows grouped exactly as qd_plan_pool groups them, per row r and fftshifted bin b over the f32 values the norms
 * sink writes for the group (a NaN is ignored, the sign bit is dropped: -0.0 counts as 0.0):
 *   count_rows[r W + b]  u32  the number of non-NaN values, +inf included
 *   sum_rows[r W + b]    f64  the EXACT real sum S of the values rounded once, to nearest, ties to even; 0.0 with no values
 *   mean_rows[r W + b]   f32  the rational S / count rounded once to f32, nearest, ties to even, subnormal results included (it is not
 *                             (float)(sum / count)); the quiet NaN 0x7fc00000 with no values
 * Any +inf makes sum and mean +inf.  A floating-point sum depends on its order, so the values are accumulated exactly, in fixed point,
 * and the results depend on no batch, chunk, memory kind, launch or arrival order.  pool == 1: mean is the norm bit for bit wherever
 * it is not NaN and sum == (double)norm.  A group holds at most 2^31 windows.
 *
 * The accumulator is public so that parts merge: rows * width * QD_MEAN_WORDS caller-owned uint64_t, cell (r, b) at
 * (r width + b) QD_MEAN_WORDS.  Words 0-8 are limbs L[0..8] in units of 2^-149, 32 payload bits each plus deferred carries: the cell's
 * exact sum is the sum of L[j] 2^(32 j) 2^-149.  A value of biased exponent e and 23-bit fraction m (m |= 1 << 23 when e != 0), with
 * s = max(e, 1) - 1, j = s >> 5, t = s & 31 and v = (uint64_t)m << t, adds v & 0xffffffff to L[j] and v >> 32 to L[j + 1]; at most 2^31
 * values per cell keep every limb below 2^63.  Word 9 is the count of finite values plus the count of +inf values shifted left by 32.
 * Every word is an integer sum: parts merge by word-wise addition. */
#define QD_MEAN_WORDS 10

/* All words 0: `rows` rows of `width` cells.  QD_ERR_INVALID: acc NULL or width == 0. */
int qd_mean_init(uint64_t *acc, uint32_t width, uint64_t rows);
/* The CPU twin of the kernel behind qd_plan_mean, bit for bit: windows at, at+1, ... at+n-1 of a range (n rows of `width` host f32 in
 * `norms`) ACCUMULATE into rows (at + i) / pool of acc, which holds the range's rows from row 0 on.  Parts of a range folded in any
 * order give the same words.  QD_ERR_INVALID: pool == 0, width == 0, acc NULL, norms NULL with n > 0, or a row whose cells would hold
 * more than 2^31 values (checked once per row before anything is added, counting every window of the call for the row: acc is then
 * unchanged). */
int qd_mean_fold(uint64_t *acc, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n);
/* dst += src, word-wise.  QD_ERR_INVALID: NULL, width == 0, or a cell's count would pass 2^31 (dst is then unchanged). */
int qd_mean_merge(uint64_t *dst, const uint64_t *src, uint32_t width, uint64_t rows);
/* The results of an accumulator, rows * width each; any may be NULL, not all.  QD_ERR_INVALID: acc NULL, width == 0, all outputs NULL. */
int qd_mean_finish(const uint64_t *acc, uint32_t width, uint64_t rows, float *mean_rows, double *sum_rows, uint32_t *count_rows);
/* The average-trace rows of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; src, src_mem, src_first, src_count and
 * `stream` as for qd_plan_run (device, host and pinned sources).  mean_rows / sum_rows / count_rows are R W values each of out_mem
 * memory (host, pinned or device; any may be NULL, not all) and are OVERWRITTEN; the call returns after they are complete.  The windows
 * go batch by batch through the plan's own kernel into a device carrier of at most max(chunk_bytes, one tile of windows) of norms.  A
 * row whose windows one workgroup sees in one batch is rounded in the fold kernel; every other row goes through a device limb
 * accumulator of at most max(2 chunk_bytes, 80 W bytes), whatever R is, and is rounded by a second small kernel.
 * Codes as qd_plan_pool: QD_ERR_INVALID for any epilogue other than QD_EPI_NORMS_F32, pool == 0, pool (clamped to n_windows) above
 * 2^31, all outputs NULL or an unknown memory kind; QD_ERR_SHORT past the sink's loop (the outputs are not touched), and for a
 * cascade's range past qd_plan_complete_windows (every complete window of the range is folded; rows without one hold count 0, sum 0.0,
 * mean NaN); QD_ERR_UNSUPPORTED for a plan created with shards (qd_mean_merge per shard's accumulator, or give each device a
 * contiguous range of ROWS on a plan of its own).  n_windows == 0: QD_OK, nothing is touched. */
int qd_plan_mean(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                 uint64_t first_window, uint64_t n_windows, uint64_t pool,
                 float *mean_rows, double *sum_rows, uint32_t *count_rows, int out_mem, void *stream);

/* ------------------------------------------------------------------ RMS-trace rows of a norms plan
 *
 * The power average (the RMS detector; the Bartlett / Welch estimate) next to max hold, min hold and the average of |X|: over windows
 * [w0, w0+n) of a QD_EPI_NORMS_F32 plan of width W and R = ceil(n / pool) rows grouped exactly as qd_plan_pool and qd_plan_mean group
 * them (ragged last row; pool > n acts as pool = n), per row r and fftshifted bin b over the f32 values v the norms sink writes for the
 * group (a NaN is ignored, the sign bit is dropped):
 *   count_rows[r W + b]  u32  the number of non-NaN values, +inf included
 *   sumsq_rows[r W + b]  f64  the EXACT real sum of v^2 rounded once, to nearest, ties to even; 0.0 with no values; always zero or a
 *                             normal f64 (2^-298 ... < 2^287)
 *   rms_rows[r W + b]    f32  the real number sqrt(sum of v^2 / count) rounded once to f32, nearest, ties to even, subnormal results
 *                             included (it is not (float)sqrt(sumsq / count)); the quiet NaN 0x7fc00000 with no values.  It lies between
 *                             the group's smallest and largest value, so it never overflows
 * Any +inf makes sumsq and rms +inf.  The squares are accumulated exactly, in fixed point, and the results depend on no batch, chunk,
 * memory kind, launch or arrival order.  pool == 1: rms is |norm| bit for bit wherever it is not NaN and sumsq == (double)v * (double)v
 * exactly.  A group holds at most 2^31 windows.
 *
 * The accumulator is public so that parts and shards merge: rows * width * QD_POWER_WORDS caller-owned uint64_t, cell (r, b) at
 * (r width + b) QD_POWER_WORDS.  Words 0-17 are limbs L[0..17] in units of 2^-298, 32 payload bits each plus deferred carries: the
 * cell's exact sum of squares is the sum of L[j] 2^(32 j) 2^-298.  A value of biased exponent e and 23-bit fraction m (m |= 1 << 23
 * when e != 0), with s = max(e, 1) - 1, q = m m (< 2^48), sh = 2 s, j = sh >> 5 (0 ... 15), t = sh & 31 and the 79-bit v = q << t, adds
 * v & 0xffffffff to L[j], (v >> 32) & 0xffffffff to L[j + 1] and v >> 64 to L[j + 2]; at most 2^31 values per cell keep every limb below
 * 2^63 and the carried sum below 2^585 (19 limbs of 32 bits).  Word 18 is the count of finite values plus the count of +inf values
 * shifted left by 32, exactly as QD_MEAN_WORDS' word 9.  Every word is an integer sum: parts merge by word-wise addition. */
#define QD_POWER_WORDS 19

/* All words 0: `rows` rows of `width` cells.  QD_ERR_INVALID: acc NULL or width == 0. */
int qd_power_init(uint64_t *acc, uint32_t width, uint64_t rows);
/* The CPU twin of the kernel behind qd_plan_power, bit for bit: windows at, at+1, ... at+n-1 of a range (n rows of `width` host f32 in
 * `norms`) ACCUMULATE into rows (at + i) / pool of acc, which holds the range's rows from row 0 on.  Parts of a range folded in any
 * order give the same words.  QD_ERR_INVALID: pool == 0, width == 0, acc NULL, norms NULL with n > 0, or a row whose cells would hold
 * more than 2^31 values (checked once per row before anything is added: acc is then unchanged). */
int qd_power_fold(uint64_t *acc, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n);
/* dst += src, word-wise.  QD_ERR_INVALID: NULL, width == 0, or a cell's count would pass 2^31 (dst is then unchanged). */
int qd_power_merge(uint64_t *dst, const uint64_t *src, uint32_t width, uint64_t rows);
/* The results of an accumulator, rows * width each; any may be NULL, not all.  QD_ERR_INVALID: acc NULL, width == 0, all outputs NULL. */
int qd_power_finish(const uint64_t *acc, uint32_t width, uint64_t rows, float *rms_rows, double *sumsq_rows, uint32_t *count_rows);
/* The RMS-trace rows of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; every argument as qd_plan_mean's, the outputs
 * OVERWRITTEN, the call returning after they are complete.  A row whose windows one workgroup sees in one batch is rounded in the fold
 * kernel; every other row goes through a device limb accumulator of at most max(2 chunk_bytes, 152 W bytes), whatever R is, and is
 * rounded by a second small kernel.
 * Codes as qd_plan_mean: QD_ERR_INVALID for any epilogue other than QD_EPI_NORMS_F32, pool == 0, pool (clamped to n_windows) above
 * 2^31, all outputs NULL or an unknown memory kind; QD_ERR_SHORT past the sink's loop (the outputs are not touched), and for a
 * cascade's range past qd_plan_complete_windows (every complete window of the range is folded; rows without one hold count 0, sumsq
 * 0.0, rms NaN); QD_ERR_UNSUPPORTED for a plan created with shards (qd_power_merge per shard's accumulator, or give each device a
 * contiguous range of ROWS on a plan of its own).  n_windows == 0: QD_OK, nothing is touched. */
int qd_plan_power(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                  uint64_t first_window, uint64_t n_windows, uint64_t pool,
                  float *rms_rows, double *sumsq_rows, uint32_t *count_rows, int out_mem, void *stream);

/* ------------------------------------------------------------------ deviation-trace rows of a norms plan
 *
 * The standard deviation per bin (steady or keyed; the error bar of the average trace; the sigma of a "floor + k sigma" threshold) next
 * to max hold, min hold, the average of |X| and the power average: over windows [w0, w0+n) of a QD_EPI_NORMS_F32 plan of width W and
 * R = ceil(n / pool) rows grouped exactly as qd_plan_pool, qd_plan_mean and qd_plan_power group them (ragged last row; pool > n acts as
 * pool = n), per row r and fftshifted bin b over the f32 values v the norms sink writes for the group (a NaN is ignored, the sign bit
 * is dropped).  With n the count of the non-NaN values, A = sum of v as an integer in units of 2^-149, B = sum of v^2 as an integer in
 * units of 2^-298 and D = n B - A^2 (never negative, below 2^616):
 *   count_rows[r W + b]  u32  n, +inf included
 *   ssd_rows[r W + b]    f64  the sum of squared deviations, sum of (v - mean)^2 = D / n, the EXACT rational rounded once, to nearest,
 *                             ties to even; 0.0 or a normal f64 (2^-329 ... < 2^287); 0.0 exactly when all values of the cell are equal
 *                             (n = 1 included).  Divide by n or n - 1 yourself: the library takes no side on Bessel's correction
 *   std_rows[r W + b]    f32  the population standard deviation sqrt(D) / n, the real number, rounded once to f32, nearest, ties to
 *                             even, subnormal results included (it is not (float)sqrt(ssd / n)).  It is at most half the group's
 *                             range, so it never overflows; it may round to +0 with D != 0 (values 0 and one quantum: half a quantum,
 *                             a tie, rounds to 0)
 *   mean_rows[r W + b]   f32  bit for bit qd_plan_mean's mean_rows of the same windows and pool
 *   rms_rows[r W + b]    f32  bit for bit qd_plan_power's rms_rows of the same windows and pool
 * No values: count 0, ssd 0.0, std / mean / rms the quiet NaN 0x7fc00000.  Any +inf counts, makes mean and rms +inf as in their own
 * sinks, and makes std 0x7fc00000 and ssd 0x7ff8000000000000: the deviation of a set that holds an infinity is undefined.  pool == 1:
 * std +0, ssd 0.0, mean and rms |norm| bit for bit wherever the norm is not NaN.  The difference D is taken between two exact
 * integers, so nothing cancels (sumsq / count - (sum / count)^2 in f64 does, catastrophically), and the results depend on no batch,
 * chunk, memory kind, launch or arrival order.  A group holds at most 2^31 windows.
 *
 * The accumulator is public so that parts and shards merge: rows * width * QD_SPREAD_WORDS caller-owned uint64_t, cell (r, b) at
 * (r width + b) QD_SPREAD_WORDS.  Words 0-8 are QD_MEAN_WORDS' limbs L[0..8] in units of 2^-149, words 9-26 QD_POWER_WORDS' limbs
 * L[0..17] in units of 2^-298, each filled by the rule stated there, and word 27 is their count word: the count of finite values plus
 * the count of +inf values shifted left by 32.  Every word is an integer sum: parts merge by word-wise addition. */
#define QD_SPREAD_WORDS 28
/* The result rows of a deviation fold, rows * width values each; any may be NULL, not all. */
typedef struct qd_spread_rows { float *std_rows; double *ssd_rows; uint32_t *count_rows; float *mean_rows; float *rms_rows; } qd_spread_rows;

/* All words 0: `rows` rows of `width` cells.  QD_ERR_INVALID: acc NULL or width == 0. */
int qd_spread_init(uint64_t *acc, uint32_t width, uint64_t rows);
/* The CPU twin of the kernel behind qd_plan_spread, bit for bit: windows at, at+1, ... at+n-1 of a range (n rows of `width` host f32 in
 * `norms`) ACCUMULATE into rows (at + i) / pool of acc, which holds the range's rows from row 0 on.  Parts of a range folded in any
 * order give the same words.  QD_ERR_INVALID: pool == 0, width == 0, acc NULL, norms NULL with n > 0, or a row whose cells would hold
 * more than 2^31 values (checked once per row before anything is added: acc is then unchanged). */
int qd_spread_fold(uint64_t *acc, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n);
/* dst += src, word-wise.  QD_ERR_INVALID: NULL, width == 0, or a cell's count would pass 2^31 (dst is then unchanged). */
int qd_spread_merge(uint64_t *dst, const uint64_t *src, uint32_t width, uint64_t rows);
/* The results of an accumulator into the rows of `out` that are not NULL.  QD_ERR_INVALID: acc NULL, width == 0, out NULL or all of its
 * rows NULL. */
int qd_spread_finish(const uint64_t *acc, uint32_t width, uint64_t rows, const qd_spread_rows *out);
/* The deviation-trace rows of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; every argument as qd_plan_power's, the rows
 * of `out` (R W values each of out_mem memory; any may be NULL, not all) OVERWRITTEN, the call returning after they are complete.  One
 * pass over the carrier gives all five; an output whose pointer is NULL is not worked out where that saves work (no root without
 * std_rows, no division without mean_rows).  A row whose windows one workgroup sees in one batch is rounded in the fold kernel; every
 * other row goes through a device limb accumulator of at most max(2 chunk_bytes, 224 W bytes), whatever R is, and is rounded by a
 * second small kernel.
 * Codes as qd_plan_power: QD_ERR_INVALID for any epilogue other than QD_EPI_NORMS_F32, pool == 0, pool (clamped to n_windows) above
 * 2^31, out NULL or all of its rows NULL, or an unknown memory kind; QD_ERR_SHORT past the sink's loop (the outputs are not touched),
 * and for a cascade's range past qd_plan_complete_windows (every complete window of the range is folded; rows without one hold count
 * 0, ssd 0.0 and NaNs); QD_ERR_UNSUPPORTED for a plan created with shards (qd_spread_merge per shard's accumulator, or give each
 * device a contiguous range of ROWS on a plan of its own).  n_windows == 0: QD_OK, nothing is touched. */
int qd_plan_spread(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                   uint64_t first_window, uint64_t n_windows, uint64_t pool,
                   const qd_spread_rows *out, int out_mem, void *stream);

/* ------------------------------------------------------------------ percentile traces and persistence counts of a norms plan
 *
 * The trace the average cannot be: a noise floor that one burst, or one +inf, does not drag up — a median, or any percentile, per bin —
 * and the analyser's persistence display, how often bin b sat at level l.  Over windows [w0, w0+n) of a QD_EPI_NORMS_F32 plan of width
 * W and R = ceil(n / pool) rows grouped exactly as qd_plan_pool groups them (ragged last row; pool > n acts as pool = n), the values are
 * counted on the summary's bucket scale, cut to a window of `levels` = L buckets that starts at bucket level0:
 *   bits  = bits(x) & 0x7fffffff          the sign bit is dropped; bits > 0x7f800000 is a NaN and is ignored
 *   k     = bits >> 20                    0 ... 2040, 8 buckets per octave, +inf in 2040: qd_summary.hist's scale, so
 *                                         qd_summary_quantile tells which level0 and L to pass
 *   level = min(max(k, level0) - level0, L - 1)
 * Level 0 holds everything at or below the grid's bottom bucket, level L-1 everything at or above its top bucket, +inf included.
 * 1 <= L <= 256 and level0 + L <= 2041.
 *   count_rows[(r W + b) L + l]  u32  the number of the row's non-NaN values of fftshifted bin b at level l, of exactly the f32 values the
 *                                     norms sink writes.  The row's NaN count for a bin is its windows minus the sum over l.
 * A group holds at most 2^31 windows.  Every cell is an integer count: the result depends on no batch, chunk, memory kind, launch or
 * arrival order, and parts merge by addition.
 *
 * Quantile of a cell (qd_summary_quantile's rule, per cell): N = sum over l of count, r = max(1, ceil(q N)) with the product and the ceil
 * in f64, j the first level whose cumulative count reaches r.  The r-th smallest non-NaN value lies in [lo_j, hi_j):
 *   lo_0 = 0.0, lo_j = the f32 of bits (level0 + j) << 20 for j > 0;  hi_j = the f32 of bits (level0 + j + 1) << 20 for j < L-1, hi_{L-1} = +inf
 * An empty cell (N = 0) gives the quiet NaN 0x7fc00000 for both bounds. */

/* A call's counts workspace (host outputs, or no count_rows) is at most this many bytes; above it qd_plan_density is QD_ERR_UNSUPPORTED. */
#define QD_DENSITY_MAX_WORKSPACE (1ull << 30)

/* All words 0: `rows` rows of `width` bins of `levels` counts.  QD_ERR_INVALID: counts NULL, width == 0 or levels == 0. */
int qd_density_init(uint32_t *counts, uint32_t width, uint32_t levels, uint64_t rows);
/* The CPU twin of the kernel behind qd_plan_density, bit for bit: windows at, at+1, ... at+n-1 of a range (n rows of `width` host f32 in
 * `norms`) ACCUMULATE into rows (at + i) / pool of counts, which holds the range's rows from row 0 on.  Parts of a range folded in any
 * order give the same words.  QD_ERR_INVALID: NULL arguments (norms with n > 0), width, pool or levels of 0, a grid outside the limits,
 * or a row whose cells would hold more than 2^31 values (checked once per row before anything is added, counting every window of the
 * call for the row: counts is then unchanged). */
int qd_density_fold(uint32_t *counts, uint32_t width, uint32_t level0, uint32_t levels, uint64_t pool, uint64_t at,
                    const float *norms, uint64_t n);
/* dst += src, word by word.  QD_ERR_INVALID: NULL, width == 0, levels == 0, or a cell's total would pass 2^31 (dst is then unchanged). */
int qd_density_merge(uint32_t *dst, const uint32_t *src, uint32_t width, uint32_t levels, uint64_t rows);
/* Host arithmetic: per cell the bounds of the q-quantile's level and N, rows * width values each; any output may be NULL, not all.
 * QD_ERR_INVALID: counts NULL, width == 0, a grid outside the limits, all outputs NULL, q outside [0, 1] or NaN. */
int qd_density_quantile(const uint32_t *counts, uint32_t width, uint32_t level0, uint32_t levels, uint64_t rows, double q,
                        float *lo_rows, float *hi_rows, uint32_t *n_rows);
/* The level counts of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan, and the percentile traces read off them; src,
 * src_mem, src_first, src_count and `stream` as for qd_plan_run (device, host and pinned sources).  count_rows is R W L u32 and may be
 * NULL.  trace_rows is n_q R W f32, trace i at i R W: the lo bound of the level of the q[i]-quantile of each cell (q = 0.5: the median
 * trace); n_q <= 8, and trace_rows may be NULL when n_q == 0; not both outputs.  The outputs are of out_mem memory (host, pinned or
 * device), are OVERWRITTEN, and the call returns after they are complete.  The windows go batch by batch through the plan's own kernel
 * into a device carrier of at most max(chunk_bytes, one tile of windows) of norms and are counted there into an accumulator of R W L
 * words: count_rows itself when out_mem is device memory and count_rows is given, else a workspace that is copied down once and may
 * not exceed QD_DENSITY_MAX_WORKSPACE (1 GiB) — QD_ERR_UNSUPPORTED, and the caller walks the range in spans of rows.
 * Other codes as qd_plan_pool: QD_ERR_INVALID for any epilogue other than QD_EPI_NORMS_F32, pool == 0, pool (clamped to n_windows)
 * above 2^31, a grid outside the limits, n_q > 8, a q outside [0, 1] or NaN, no output or an unknown memory kind; QD_ERR_SHORT past the
 * sink's loop (the outputs are not touched), and for a cascade's range past qd_plan_complete_windows (every complete window of the
 * range is counted; rows without one hold counts 0 and a NaN trace); QD_ERR_UNSUPPORTED for a plan created with shards (give each
 * device a contiguous range of ROWS on a plan of its own, or qd_density_merge per-shard counts).  n_windows == 0: QD_OK, nothing is
 * touched. */
int qd_plan_density(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                    uint64_t first_window, uint64_t n_windows, uint64_t pool, uint32_t level0, uint32_t levels,
                    uint32_t *count_rows, const double *q, uint32_t n_q, float *trace_rows, int out_mem, void *stream);

/* ------------------------------------------------------------------ band traces of a norms plan
 *
 * The folds above reduce over time, per bin.  This one reduces over FREQUENCY, per window: for every window and each of K chosen ranges
 * of bins it gives the level in the band, the band's peak and where the peak sits, and which band is the loudest — the OOK envelope, an
 * N-FSK demodulator without re-centring (what `bucket -by freq N` would be), several channels out of one transform, the peak track.
 * Over windows [w0, w0+n) of a QD_EPI_NORMS_F32 plan of width W and K bands [lo_k, hi_k) of fftshifted bins (0 <= lo < hi <= W; bands may
 * overlap or repeat), on exactly the f32 values the norms sink writes; window i of the range and band k are at index i K + k:
 *   count_rows     u32  the band's non-NaN values, +inf included
 *   sum_rows       f64  the exact sum of the band's values, rounded once;  no values: 0.0;  any +inf: +inf
 *   level_rows     f32  sum / count, rounded once;  no values: the quiet NaN 0x7fc00000;  any +inf: +inf.  The three are bit for bit
 *                       qd_mean_finish(qd_mean_fold(...)) of the band's values laid out as hi - lo windows of width 1 with pool = hi - lo.
 *   peak_rows      f32  the f32::max fold from 0.0 by qd_plan_pool's rule: a NaN is ignored, the sign bit is dropped
 *   peak_bin_rows  u32  the lowest fftshifted bin of the band whose value equals the peak;  QD_BAND_NONE when count == 0
 *   pick_rows      u8   at index i: the lowest k with the greatest level_rows among the window's bands with count > 0 (such levels are
 *                       non-negative or +inf and compare as bit patterns);  255 when no band of the window holds a value.  It is
 *                       computable from level_rows and count_rows alone.
 * Every output is an integer sum, an integer max or a function of them: no batch, chunk, memory kind or launch order changes a bit.  A
 * one-bin band returns the norm itself: level == norm, sum == (double)norm, count == 1, peak == norm, peak_bin == lo. */
#define QD_BANDS_MAX 255
#define QD_BAND_NONE 0xffffffffu
typedef struct qd_band { uint32_t lo, hi; } qd_band;   /* fftshifted bins [lo, hi), 0 <= lo < hi <= W; bands may overlap or repeat */
/* The result rows of a band fold; a NULL pointer is an output that is not asked for. */
typedef struct qd_band_rows { float *level_rows; double *sum_rows; uint32_t *count_rows;
                              float *peak_rows; uint32_t *peak_bin_rows; uint8_t *pick_rows; } qd_band_rows;

/* The CPU twin of the kernels behind qd_plan_bands, bit for bit: n rows of `width` host f32 into the n x n_bands rows of `out`, which are
 * OVERWRITTEN.  Windows are independent, so the call is stateless: there is no _init / _merge / _finish.  QD_ERR_INVALID: width == 0,
 * n_bands 0 or above QD_BANDS_MAX, bands NULL, a band with lo >= hi or hi > width, out NULL or all of its rows NULL, norms NULL with
 * n > 0.  n == 0: QD_OK, nothing is touched. */
int qd_bands_fold(const float *norms, uint32_t width, uint64_t n, const qd_band *bands, uint32_t n_bands, const qd_band_rows *out);
/* The band traces of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; src, src_mem, src_first, src_count and `stream` as for
 * qd_plan_run (device, host and pinned sources).  The rows of `out` are of out_mem memory (host, pinned or device), n_windows x n_bands
 * each (pick_rows: n_windows), are OVERWRITTEN, and the call returns after they are complete; any may be NULL, not all.  pick_rows needs
 * neither level_rows nor count_rows.  `bands` is host memory and is read before the call returns.  The windows go batch by batch through
 * the plan's own kernel into a device carrier of at most max(chunk_bytes, one tile of windows) of norms and are folded there; rows that
 * are not device memory (and the two pick_rows is read from, when they are not asked for) go through a workspace that is copied down
 * once and may not exceed 1 GiB — QD_ERR_UNSUPPORTED, and the caller walks the range in spans of windows.
 * Other codes as qd_plan_pool: QD_ERR_INVALID for any epilogue other than QD_EPI_NORMS_F32, n_bands 0 or above QD_BANDS_MAX, bands NULL, a
 * band with lo >= hi or hi > W, out NULL or all of its rows NULL, or an unknown memory kind; QD_ERR_SHORT past the sink's loop (the
 * outputs are not touched), and for a cascade's range past qd_plan_complete_windows (every complete window of the range is folded; the
 * rest hold count 0, sum 0.0, level NaN, peak 0.0, QD_BAND_NONE and pick 255); QD_ERR_UNSUPPORTED for a plan created with shards (one plan
 * per contiguous range of windows: the rows simply concatenate).  n_windows == 0: QD_OK, nothing is touched. */
int qd_plan_bands(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                  uint64_t first_window, uint64_t n_windows, const qd_band *bands, uint32_t n_bands,
                  const qd_band_rows *out, int out_mem, void *stream);

/* ------------------------------------------------------------------ waterfall pictures of a norms plan
 *
 * The picture itself: the `render` loop of the reference's conrod front end (src/ui/mod.rs:294-412) behind the norms sink.  Every
 * fftshifted |X| goes through an HSV colour map (:345-372) and the windows' columns are laid into wrapped strips of an RGB image with a
 * `stretch`, a 16-pixel gap and `scan` marker columns (:311-332, :374-391).
 *
 * THE DEFINITION.  palette 0.5.0 is named by Cargo.lock:2650; its source is not at hand, so HSV -> RGB is PARITY UNPINNED, like rustfft.
 * The project pins its own statement instead: the textbook conversion, as palette 0.5 is recalled to write it.  Wherever "the reference's
 * colours" is claimed, this statement is meant.
 *
 * Colour of one norm.  Every operation is one IEEE f32 operation, separately rounded.  Nothing is contracted into an FMA.  Subnormals
 * are kept.
 *   scaled = x / scale                     (scale = 2.29 in the reference, :353)
 *   s1     = 1.0 - scaled
 *   hue    = (s1 * 0.8) * 360.0
 *   val    = 1.0 - s1                      (not `scaled`: the reference subtracts twice, :361-366)
 *   pos    = hue - floor(hue / 360.0) * 360.0
 *   h      = pos / 60.0
 *   c      = val * 1.0 ;  m = val - c
 *   t      = h - 2.0 * floor(h * 0.5)      (h % 2 for finite h >= 0)
 *   xx     = c * (1.0 - |t - 1.0|)
 *   (r,g,b) = 0<=h<1:(c,xx,0)  1<=h<2:(xx,c,0)  2<=h<3:(0,c,xx)  3<=h<4:(0,xx,c)  4<=h<5:(xx,0,c)  else:(c,0,xx)
 *   byte   = Rust's `as u8` of ((chan + m) * 256.0): truncate, saturate to 0..255, NaN -> 0
 * The `else` branch also takes NaN, because every comparison is false there.  The consequences: NaN and +inf give (0,0,0); 0 and -0
 * give (0,0,0); x >= scale saturates the red channel (for x up to 1.2 scale; beyond, the negative hue wraps on through the sectors and red is xx in
 * some of them); 1e-40 gives (0,0,0).  At scale 2.29: 0.25 -> (7,0,27), 1.0 -> (0,111,78),
 * 2.0 -> (223,135,0), 2.29 -> (255,0,0), 2.75 -> (255,0,255).
 *
 * Page.  Pixels are 3 bytes R,G,B, px_width x px_height = w h of them.  Pixel (x, y) lives at byte ((h - 1 - y) w + x) 3, so y = 0 is
 * the bottom row (MemImage::set, :286-291).  Let row_height = stretch W + 16.  Window p of the range, counted from the range's first
 * window, is column x = p % w of strip r = p / w, whose origin is oy = r row_height.  The strip exists iff oy <= h: the reference's test
 * is `>`, so it is not `<` (:330), and a strip at oy == h consumes its windows and shows nothing.  Hence strips = h / row_height + 1, and
 * at most max_windows = strips w windows are ever looked at; the reference breaks out of its loop there.  Bin o of the window, in the
 * fftshifted order the norms sink writes, paints pixel rows y = oy + o stretch + off for off < stretch; rows with y >= h are skipped.
 * A column with scan >= 1 && p % scan == 0 is painted (0,0,0) in place of its colours (:374-376).  scan == 0 means no marker columns:
 * our one extension — the reference never has 0, and its default of 1 blackens every column.  The gap rows, and every pixel that no
 * window reaches, are (0,0,0).
 * Deviation: the reference's ensure!(w > fft_width) ("TODO: window too narrow") is a GUI to-do and not arithmetic; the library does not
 * carry it. */
typedef struct qd_picture_desc {
    uint32_t struct_size;     /* sizeof(qd_picture_desc) */
    uint32_t px_width;        /* w >= 1 */
    uint32_t px_height;       /* h >= 1 */
    uint32_t stretch;         /* >= 1: pixel rows per bin (the reference's Params default: 4, :72-76) */
    uint32_t scan;            /* 0: no marker columns; N: every N-th window's column is black */
    float scale;              /* finite, > 0 (the reference: 2.29, :353) */
} qd_picture_desc;
/* A call's picture workspace (a picture that is not device memory) is at most this many bytes; above it qd_plan_picture is QD_ERR_UNSUPPORTED. */
#define QD_PICTURE_MAX_WORKSPACE (1ull << 30)

/* The page for windows of `width` bins (:311-332): *strips = h / row_height + 1, *max_windows = strips w, *bytes = 3 w h; any of the
 * three may be NULL.  QD_ERR_INVALID (the outputs are not touched): desc NULL or of an unknown struct_size, width == 0, px_width,
 * px_height or stretch of 0, or a scale that is not a finite positive f32.  Every call below refuses a desc by the same rule. */
int qd_picture_geometry(const qd_picture_desc *desc, uint32_t width, uint64_t *strips, uint64_t *max_windows, uint64_t *bytes);
/* The colour map alone, on the host (:345-372): n host f32 into 3 n bytes R,G,B.  QD_ERR_INVALID: a scale that is not finite and
 * positive, or a NULL array with n > 0. */
int qd_picture_color(const float *norms, size_t n, float scale, uint8_t *rgb);
/* Writes black: 3 w h zero bytes of host memory. */
int qd_picture_init(uint8_t *pixels, const qd_picture_desc *desc);
/* The CPU twin of the kernel behind qd_plan_picture, byte for byte: windows at, at+1, ... at+n-1 of a range (n rows of `width` host f32
 * in `norms`) paint their columns into the host picture `pixels`, which holds the whole page.  A window writes only its own column, so
 * parts of a range folded in any order give the whole.  Windows at or beyond max_windows are ignored.  QD_ERR_INVALID: a refused desc,
 * pixels NULL, or norms NULL with n > 0. */
int qd_picture_fold(uint8_t *pixels, const qd_picture_desc *desc, uint32_t width, uint64_t at, const float *norms, uint64_t n);
/* The picture of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan (`render`, :294-412; one transform per window as fft_at,
 * :414-430); src, src_mem, src_first, src_count and `stream` as for qd_plan_run (device, host and pinned sources).  `pixels` is 3 w h
 * bytes of out_mem memory (host, pinned or device, of any alignment) and is OVERWRITTEN: black first, then the columns; the call returns
 * after it is complete.  *painted (may be NULL) is the number of windows transformed: min(n_windows, max_windows), or fewer for a short
 * cascade.  Windows beyond that are not even run through the chain.  The windows go batch by batch through the plan's own kernel into a
 * device carrier of at most max(chunk_bytes, one tile of windows) of norms and are painted from there into the picture itself when
 * out_mem is device memory, else into a workspace that is copied down once.  Each byte of a column is stored once, by one lane, without
 * atomics: no batch, chunk, memory kind or launch order changes a byte.  A fold leaves qd_plan_get_stats alone.
 * Codes as qd_plan_pool: QD_ERR_INVALID for any epilogue other than QD_EPI_NORMS_F32, a refused desc, pixels NULL or an unknown memory
 * kind; QD_ERR_SHORT past the sink's loop (the outputs are not touched), and for a cascade when a window that is looked at is past
 * qd_plan_complete_windows (every complete window of the range is painted and *painted counts them); QD_ERR_UNSUPPORTED for a plan
 * created with shards (one plan per contiguous range of columns, composed on the host the way qd_picture_fold composes parts), and for
 * a picture workspace above QD_PICTURE_MAX_WORKSPACE.  n_windows == 0: QD_OK and a black picture. */
int qd_plan_picture(qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                    uint64_t first_window, uint64_t n_windows, const qd_picture_desc *desc,
                    uint8_t *pixels, int out_mem, uint64_t *painted, void *stream);

/* ------------------------------------------------------------------ burst list of a norms plan
 * What happened when: a threshold per bin, applied to windows [w0, w0 + n) of a QD_EPI_NORMS_F32 plan of width W (exactly the f32 values
 * the norms sink writes), and the list of on/off runs per bin.  `thresholds` is a host array of W f32 in fftshifted bin order.  This is
 * the project's own definition; the reference has no counterpart.
 *
 * Admissible thresholds.  Write a(v) = bits(v) & 0x7fffffff and t_b = bits(thresholds[b]).  A threshold is admissible if its sign bit is
 * clear and it is not a NaN (t_b <= 0x7f800000: +0.0 and +inf are allowed); a NaN of either sign is admissible too and MASKS the bin.
 * Anything else (negative numbers, -0.0, -inf) is QD_ERR_INVALID.
 * On cells.  Cell (i, b) is on when the bin is not masked, a(v) <= 0x7f800000 (a NaN value is never on) and a(v) >= t_b: the sign of a
 * value is dropped, by qd_plan_pool's rule, and the comparison is one of bit patterns, which for these operands is the f32 comparison.
 * A threshold of 0 turns on every non-NaN cell, one of +inf only +inf.
 * Bursts.  A burst is a maximal run of on cells in one bin: windows [first, first + length) of the range, counted from the range's first
 * window, all on, with window first - 1 and window first + length off or outside the range (a run is cut at the range's edges).
 * Peak.  `peak` is the greatest a(v) of the run as an f32 (+inf is possible), `peak_at` the first window of the run, range-relative,
 * that attains it.
 * Which are kept.  A burst is kept iff length >= min_len; min_len >= 1, and 0 is QD_ERR_INVALID.
 * Order.  Ascending (first + length - 1, bin): the last window of the burst, then the bin.  No two bursts share that key.  It is the
 * order of an event log: a burst is reported when it ends.
 * Counts.  *found is the number of kept bursts, always the full count; the list receives the first min(found, cap) of them in that
 * order, and its bytes past that are not touched.  on_counts[b] (optional) is the number of on cells of bin b over the range, the
 * bin's occupancy at this threshold, not filtered by min_len.
 * Determinism.  Every output is an integer count, an integer max or an index: no batch, chunk, piece, memory kind, cap or launch order
 * changes a byte. */
typedef struct qd_burst { uint64_t first, length, peak_at; uint32_t bin; float peak; } qd_burst;   /* 32 bytes, little-endian as it lies */
#define QD_BURSTS_WORDS 3          /* u64 of state per bin: first window of the open run or ~0, its peak_at, its peak bits */
/* A call's list workspace (a list that is not device memory, cap x 32 bytes) is at most this; above it qd_plan_bursts is QD_ERR_UNSUPPORTED. */
#define QD_BURSTS_MAX_WORKSPACE (1ull << 30)

/* The CPU twin, byte for byte.  It is stateful because a run crosses parts: `state` is QD_BURSTS_WORDS*width + 1 u64 of host memory,
 * the last word being the next window expected.  _init: no run open, next window 0, on_counts (may be NULL) zeroed.
 * _fold takes windows at ... at+n-1 of the range (n rows of `width` host f32); `at` must equal the state's next window, else
 * QD_ERR_INVALID.  A burst is detected at the first off window after it: row i emits the runs that ended at i-1, by bin ascending, so
 * the order of emission is the order of the list.  *found is in/out and keeps counting past cap; record number *found goes to
 * list[*found] while that is below cap.  on_counts (may be NULL) is in/out.
 * _finish closes the runs still open, with last window next-1, by bin ascending, and leaves the state as _init does.
 * Any partition of a range into folds followed by _finish gives exactly the list of the definition; n == 0 folds are fine.
 * QD_ERR_INVALID: width 0, NULL state, thresholds or found, an inadmissible threshold, min_len == 0, list == NULL with cap > 0, norms
 * NULL with n > 0. */
int qd_bursts_init  (uint64_t *state, uint64_t *on_counts /* may be NULL */, uint32_t width);
int qd_bursts_fold  (uint64_t *state, uint32_t width, const float *thresholds, uint64_t min_len, uint64_t at,
                     const float *norms, uint64_t n, qd_burst *list, uint64_t cap, uint64_t *found, uint64_t *on_counts);
int qd_bursts_finish(uint64_t *state, uint32_t width, uint64_t min_len, qd_burst *list, uint64_t cap, uint64_t *found);
/* The burst list of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; src, src_mem, src_first, src_count and `stream` as
 * for qd_plan_bands (device, host and pinned sources), and so are the refusals and a cascade's short read.  `list` (cap records) and
 * on_counts (W u64, may be NULL) are of out_mem memory (host, pinned or device); `found` and `thresholds` are host memory, and the call
 * returns after everything is complete.  A list that is not device memory goes through a workspace of cap x 32 bytes that is copied
 * down once (min(found, cap) records of it).  cap == 0 with list == NULL counts only.  The windows go batch by batch through the plan's
 * own kernel into a device carrier and are walked from there; runs are carried from batch to batch on the device.  A fold leaves
 * qd_plan_get_stats alone.
 * QD_ERR_INVALID: any epilogue other than QD_EPI_NORMS_F32, thresholds or found NULL, an inadmissible threshold, min_len == 0, list NULL
 * with cap > 0, an unknown memory kind.  QD_ERR_UNSUPPORTED: a plan created with shards (run one range on one device; joining lists
 * across a seam is the caller's job), a list workspace above QD_BURSTS_MAX_WORKSPACE, a width above 131072.  QD_ERR_SHORT: a range past
 * the sink's loop (the outputs are not touched), and for a cascade a range past qd_plan_complete_windows: the complete part is folded,
 * and the open runs close at the last complete window.  n_windows == 0: QD_OK with *found = 0, on_counts zeroed and the list untouched. */
int qd_plan_bursts  (qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                     uint64_t first_window, uint64_t n_windows, const float *thresholds, uint64_t min_len,
                     qd_burst *list, uint64_t cap, uint64_t *found, uint64_t *on_counts, int out_mem, void *stream);

/* ------------------------------------------------------------------ emission list of a norms plan
 * What happened when, per signal and not per bin: the thresholds of the burst list applied to windows [w0, w0 + n) of a
 * QD_EPI_NORMS_F32 plan of width W, and one record per connected region of on cells in the (window, bin) plane.  This is the
 * project's own definition; the reference has no counterpart.
 *
 * Thresholds, on cells.  Exactly the burst list's rules: a(v) = bits(v) & 0x7fffffff; a threshold is +0 ... +inf, or a NaN of either
 * sign, which masks its bin; negative numbers, -0.0 and -inf are QD_ERR_INVALID; a NaN value is never on.
 * Emission.  A maximal 4-connected set of on cells of the range: cells (i, b) and (i', b') are neighbours iff |i - i'| + |b - b'| = 1.
 * Bins 0 and W - 1 are not neighbours (the fftshifted row does not wrap), and an emission is cut at the range's edges.
 * Record.  first, last: the first and last window, range-relative and inclusive.  cells: the number of on cells.  lo, hi: the lowest
 * and highest bin, inclusive.  end_bin: the lowest bin that is on in window `last`.  peak: the greatest a(v) as an f32 (+inf is
 * possible); (peak_at, peak_bin) is the lexicographically smallest (window, bin) that attains it.  flags: bit 0 is set when the emission
 * touches the range's first window, bit 1 when it touches the range's last window (both mean it was cut); all other bits are 0.
 * Which are kept.  An emission is kept iff last - first + 1 >= min_len and cells >= min_cells; both are >= 1, and 0 is QD_ERR_INVALID.
 * Order.  Ascending (last, end_bin).  Cell (last, end_bin) belongs to exactly one emission, so no two emissions share the key.  It is
 * the order of an event log: an emission is reported when it ends.
 * Counts.  *found is the number of kept emissions, always the full count; the list receives the first min(found, cap) of them in that
 * order, and its bytes past them are not touched.  cap == 0 with list == NULL counts only.
 * Determinism.  Every output is an integer count, an integer extreme or an index: no batch, chunk, span, tile, memory kind, cap or launch
 * order changes a byte. */
typedef struct qd_emission {
    uint64_t first, last, cells, peak_at;
    uint32_t lo, hi, end_bin, peak_bin;
    float    peak;
    uint32_t flags;
} qd_emission;                     /* 56 bytes, little-endian as it lies */
#define QD_EMISSION_CUT_FIRST 1u
#define QD_EMISSION_CUT_LAST  2u
#define QD_EMISSIONS_WORDS 8       /* u64 of state per bin: the bin's open slot or ~0, and the 7 words of one record of the open table */
/* A call's list workspace (a list that is not device memory, cap x 56 bytes) is at most this; above it qd_plan_emissions is
 * QD_ERR_UNSUPPORTED.  The labelling's own workspace stays below it whatever chunk_bytes is. */
#define QD_EMISSIONS_MAX_WORKSPACE (1ull << 30)
#define QD_EMISSIONS_MAX_WIDTH 4096u

/* The CPU twin, byte for byte.  It is stateful because an emission crosses parts: `state` is QD_EMISSIONS_WORDS*width + 2 u64 of host
 * memory: per bin the slot of the emission that is open there in the previous row, or ~0; a table of at most `width` open partial
 * records (a row has at most ceil(width / 2) open emissions); the next window expected; the number of open records.
 * _init: nothing open, next window 0.  _fold takes windows at ... at+n-1 of the range (n rows of `width` host f32), one row at a time;
 * `at` must equal the state's next window, else QD_ERR_INVALID.  A row joins its runs of on cells with the open emissions above them
 * (a union-find over the open slots) and emits the open emissions that found no on neighbour, by end_bin ascending, so the order of
 * emission is the order of the list.  *found is in/out and keeps counting past cap; record number *found goes to list[*found] while
 * that is below cap.  _finish closes what is open at the last window folded, in the same order, with bit 1 of flags set, and leaves
 * the state as _init does.  Any partition of a range into folds followed by _finish gives exactly the list of the definition; n == 0
 * folds are fine.
 * QD_ERR_INVALID: width 0, NULL state, thresholds or found, an inadmissible threshold, min_len == 0, min_cells == 0, list == NULL with
 * cap > 0, norms NULL with n > 0. */
int qd_emissions_init  (uint64_t *state, uint32_t width);
int qd_emissions_fold  (uint64_t *state, uint32_t width, const float *thresholds, uint64_t min_len, uint64_t min_cells, uint64_t at,
                        const float *norms, uint64_t n, qd_emission *list, uint64_t cap, uint64_t *found);
int qd_emissions_finish(uint64_t *state, uint32_t width, uint64_t min_len, uint64_t min_cells, qd_emission *list, uint64_t cap,
                        uint64_t *found);
/* The emission list of windows [first_window, +n_windows) of a QD_EPI_NORMS_F32 plan; src, src_mem, src_first, src_count and `stream`
 * as for qd_plan_bursts (device, host and pinned sources), and so are the refusals and a cascade's short read.  `list` (cap records,
 * 8-byte aligned) is of out_mem memory (host, pinned or device); `found` and `thresholds` are host memory, and the call returns after
 * everything is complete.  A list that is not device memory goes through a workspace of cap x 56 bytes that is copied down once
 * (min(found, cap) records of it).  The windows go batch by batch through the plan's own kernel into a device carrier; a batch is
 * labelled in spans of at most 2^20 / W windows, and the open emissions are carried from span to span and from batch to batch on the
 * device.  A fold leaves qd_plan_get_stats alone.
 * QD_ERR_INVALID: any epilogue other than QD_EPI_NORMS_F32, thresholds or found NULL, an inadmissible threshold, min_len == 0,
 * min_cells == 0, list NULL with cap > 0, an unknown memory kind.  QD_ERR_UNSUPPORTED: a plan created with shards (run one range on one
 * device; an emission crosses the seam), a list workspace above QD_EMISSIONS_MAX_WORKSPACE, a width above QD_EMISSIONS_MAX_WIDTH.
 * QD_ERR_SHORT: a range past the sink's loop (the outputs are not touched), and for a cascade a range past qd_plan_complete_windows:
 * the complete part is listed, and the open emissions close at the last complete window.  n_windows == 0: QD_OK with *found = 0 and
 * the list untouched. */
int qd_plan_emissions  (qd_plan *plan, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                        uint64_t first_window, uint64_t n_windows, const float *thresholds, uint64_t min_len, uint64_t min_cells,
                        qd_emission *list, uint64_t cap, uint64_t *found, int out_mem, void *stream);

/* ------------------------------------------------------------------ cut list: shift, lowpass and decimate many stream ranges in one call
 * The step behind the emission list: the IQ of each thing in the capture, moved to DC, filtered and decimated, all cuts in one call.
 * Cut.  With D = decimate, T = taps, c = T - T/2 and valid = count D + T, the bytes of a cut are what the reference writes into
 * buf[..count] on read_at(first, buf) of the chain  from F -> [shift shift_hz] -> lowpass -decimate D (size T) lowpass_hz  over the whole
 * described stream (n_samples samples at sample_rate):
 *   out[i] = sum_{j < jmax(i)} x[first D + i D + c + j] taps[j],  jmax(i) = min(T, valid - (i D + c)),
 * ascending j, two separately rounded products and two adds per term, no FMA (qd_lowpass_block's arithmetic); x is the unpacked source
 * sample times the reference's NCO multiplier of its ABSOLUTE index (qd_shift's arithmetic; no multiply at all with shift_hz == 0); taps
 * is qd_lowpass_design(lowpass_hz, sample_rate, T).  The block's own tail truncation is part of the definition: the last ceil(c / D)
 * outputs of a cut see a shortened filter, as the last outputs of a `write` block do; a caller who wants clean samples asks for that
 * many more and drops them (qd_cut_of_emission adds them).  The SOURCE SPAN of a cut is samples [first D, first D + valid).
 * NCO.  The exact product is split on the absolute row grid of 512 samples, as qd_shift splits it, and the second-order form is used for
 * a cut iff fabs(ratio) * (double)(first D + valid) > 268435456.0: qd_shift's rule for a call over exactly that span.  So a cut's bytes
 * depend on its six fields and the stream and on nothing else - not on its place in the list, its neighbours, tiles, batches,
 * chunk_bytes or memory kinds - and equal qd_unpack -> qd_shift(abs_off = first D) -> qd_lowpass_block(valid) byte for byte.
 * QD_MODE_FAST does not exist for cuts. */
typedef struct qd_cut {
    int64_t  shift_hz;        /* 0: no Shift stage at all (bit-exact path) */
    uint64_t lowpass_hz, decimate, taps;
    uint64_t first, count;    /* output samples [first, first + count) of the chain's stream */
} qd_cut;                     /* 48 bytes */
#define QD_CUT_MAX_DECIMATE 1024u
#define QD_CUT_MAX_TAPS     4096u

/* Validation, the same in both calls below and all of it ahead of any device call.  Cuts are checked in list order and the first
 * offender is named in qd_last_error by its index; for one cut the order is: decimate 0, taps < 2, |shift_hz| >= sample_rate / 2 in
 * integer division as Shift::new asserts (QD_ERR_PANIC, the plan's codes); decimate > QD_CUT_MAX_DECIMATE, taps > QD_CUT_MAX_TAPS,
 * count > 2^31 (QD_ERR_UNSUPPORTED); first D + valid > n_samples - a cut is one FULL block - (QD_ERR_SHORT; no output byte is touched
 * by the call); a span outside [src_first, src_first + src_count) (QD_ERR_INVALID, qd_cuts_run only).  A cut with count == 0 has no
 * span: only its fields are checked, and it writes nothing.  n_cuts == 0 is fine. */

/* host arithmetic only: offsets[k] = sum of count over cuts before k (offsets[n] = total; may be NULL); the union's hull of the
 * source spans in *src_first / *src_count (0 / 0 without a span); validates as qd_cuts_run does */
int qd_cuts_geometry(uint64_t sample_rate, uint64_t n_samples, const qd_cut *cuts, size_t n_cuts,
                     uint64_t *offsets, uint64_t *src_first, uint64_t *src_count);
/* src: raw bytes of source samples [src_first, +src_count) in `fmt`, as for qd_plan_run (device, host, pinned).  out: total qd_c32
 * of out_mem memory, cut k at element offsets[k], packed.  options: chunk_bytes only (NULL: defaults).  Returns after
 * everything is complete.  Device sources are read in place; of a host or pinned source only the union of the cuts' spans is copied
 * up, in batches of at most chunk_bytes of source (0: 64 MiB; a batch holds at least one tile), a longer cut split at tile
 * boundaries; host outputs come back batch by batch.  QD_ERR_INVALID also for an unknown format or memory kind and for a NULL
 * cuts, src or out that would be read or written. */
int qd_cuts_run(int fmt, uint64_t sample_rate, uint64_t n_samples, const void *src, int src_mem,
                uint64_t src_first, uint64_t src_count, const qd_cut *cuts, size_t n_cuts,
                qd_c32 *out, int out_mem, const qd_plan_options *options, void *stream);

/* Emission -> cut: host arithmetic in integers.  desc is the one-stage QD_EPI_NORMS_F32 desc the list was made from, first_window the
 * first_window of that qd_plan_emissions call.  With sr = sample_rate, D0 = decimate with a lowpass else 1, T0 = taps with a lowpass
 * else 0, R = sr / D0, W = width, S = stride, f0 = shift_hz with a shift else 0, fdiv / cdiv floor / ceiling division of signed integers:
 *   nu = fdiv((lo + hi - W) R + W, 2 W)            the centre of bins lo ... hi at the sink's rate, halves rounded up
 *   s = (f0 - nu) mod sr in [0, sr); hs = sr / 2; s >= hs: s -= sr; then s <= -hs: s = 1 - hs;  shift_hz = s (the emission lands on DC)
 *   lowpass_hz = max(1, cdiv((hi - lo + 1 + 2 guard_bins) R, 2 W))
 *   decimate = clamp(sr / (2 oversample lowpass_hz), 1, max_decimate)     (max_decimate 0: QD_CUT_MAX_DECIMATE)
 *   taps = rule.taps, or with rule.taps == 0 min(QD_CUT_MAX_TAPS, max(40, 8 decimate))
 *   a = (first_window + e.first) S D0;  b = min(n_samples, (first_window + e.last) S D0 + W D0 + T0)
 *   first = max(0, fdiv(a - T, D) - pad);  end = cdiv(max(b - T, 0), D) + pad + cdiv(T - T/2, D)
 *   count = max(0, min(end, fdiv(n_samples - T, D)) - first)
 * QD_ERR_INVALID: NULL, a wrong struct_size of desc or rule, oversample == 0, a non-zero rule.taps < 2, lo > hi or hi >= W, a desc
 * with sample_rate 0, stride 0 or (with a lowpass) decimate 0.  QD_ERR_UNSUPPORTED: sr >= 2^48, or a window index, stride or width
 * that puts b (before the min) at or past 2^62.  Cascade plans have no single (f0, D0) and are out of scope. */
typedef struct qd_cut_rule { uint32_t struct_size, guard_bins, oversample, pad; uint64_t taps, max_decimate; } qd_cut_rule;
int qd_cut_of_emission(const qd_chain_desc *desc, uint64_t first_window, const qd_emission *e, const qd_cut_rule *rule, qd_cut *cut);

/* ------------------------------------------------------------------ symbol list: bucket digits and marks of many short streams in one call
 * The step behind the cut list: every cut's digit string (`bucket -by freq 2`) or blank / non-blank rows (sparkfft, the input of
 * qd_bits_scan), all cuts in one call.  A SEGMENT is elements [first, first + count) of a cf32 buffer, viewed as a stream of len = count.
 * With width W (a power of two) and stride S >= 1, segment k yields one byte per FFT window:
 *   QD_EPI_BUCKET2_U8  n_k = (count - W) / S windows (src/fft.rs:86).  Window r is Radix4 forward over samples [r S, r S + W); first is
 *                      the sequential f32 sum of |X[j]|, ascending j < W/2 in un-shifted bin order, second that for j >= W/2; the byte is
 *                      first < second ? 0 : 1 (a NaN compares false: 1).  The arithmetic of a QD_EPI_BUCKET2_U8 plan.
 *   QD_EPI_MARK_U8     n_k = the trip count of `while i < len - W { ...; i += S }` (src/fft.rs:28,65) = ceil((count - W) / S).  The byte is 0
 *                      when every |X| of the window is < min in f32 (min = range_min with has_range, else 0.08f), else 1; a NaN marks.
 *   windowing == 1     sample j of every window is multiplied by qd_window_design(1, W)[j] as Complex<f32> x f32 ahead of the transform,
 *                      exactly as qd_chain_desc.windowing does.
 * SHORT SEGMENTS: a segment with count <= W has 0 windows and writes nothing.  This is the one departure from the reference, which
 * underflows a u64 there (qd_plan_create answers QD_ERR_PANIC for such a stream): in a list of emissions a short cut is routine and
 * must not fail the whole call.
 * Outputs are packed: segment k's bytes sit at offsets[k], offsets[n] is the total.  A segment's bytes depend on its samples, W, S, the
 * epilogue, min and the window, and on nothing else - not on its place in the list, its neighbours, tiles, batches or memory kinds.
 * Segments may overlap, repeat and leave gaps.
 * Validation, all of it ahead of any device call, in this order: NULL desc or a wrong struct_size, an epilogue other than the two,
 * stride == 0, windowing outside {0, 1} (QD_ERR_INVALID); a width that is not a power of two (QD_ERR_PANIC, qd_plan_create's code and
 * message), a width above 4096 (QD_ERR_UNSUPPORTED); a NULL segment list with n > 0 (QD_ERR_INVALID); then the segments in list order,
 * the first offender named in qd_last_error by its index: count > 2^31 (QD_ERR_UNSUPPORTED), first + count > n_in (QD_ERR_SHORT,
 * qd_symbols_run only; no output byte is touched); last a NULL in / out that would be read / written (QD_ERR_INVALID).  n == 0 is fine. */
typedef struct qd_segment { uint64_t first, count; } qd_segment;
typedef struct qd_symbols_desc {
    uint32_t struct_size; int32_t epilogue;      /* QD_EPI_BUCKET2_U8 or QD_EPI_MARK_U8 */
    uint64_t width, stride;
    int32_t  has_range; float range_min;         /* MARK only */
    int32_t  windowing; int32_t _pad;
    uint64_t iq_bytes;                           /* qd_cuts_symbols only: device workspace for the cuts' IQ; 0: 1 GiB */
} qd_symbols_desc;
#define QD_SYMBOLS_MAX_WIDTH 4096u
/* host arithmetic only: offsets[k] = windows of the segments before k, offsets[n] the total (offsets may be NULL: validation alone) */
int qd_symbols_geometry(const qd_symbols_desc *desc, const qd_segment *segments, size_t n, uint64_t *offsets /* n + 1, may be NULL */);
/* in: n_in qd_c32 of in_mem memory (device, host, pinned); out: offsets[n] bytes of out_mem memory.  Device buffers are read and written
 * in place; of a host buffer the hull of the segments goes up and the bytes come down once.  Returns after everything is complete.
 * QD_ERR_INVALID also for an unknown memory kind. */
int qd_symbols_run(const qd_symbols_desc *desc, const qd_c32 *in, int in_mem, uint64_t n_in,
                   const qd_segment *segments, size_t n, uint8_t *out, int out_mem, void *stream);
/* qd_cuts_run and qd_symbols_run in one call: cut k is segment k, its bytes go at the offsets qd_symbols_geometry gives for the cuts'
 * counts, and they equal qd_cuts_run into a buffer followed by qd_symbols_run over it byte for byte.  The IQ never leaves the device: it
 * goes into a device workspace of at most iq_bytes, the cuts taken in list order in groups of whole cuts that fit; a single cut above
 * the cap is QD_ERR_UNSUPPORTED (lower its count or raise iq_bytes).  qd_cuts_run's validation runs unchanged and first, then the
 * desc's; options is chunk_bytes only, as there.  A host out comes down once per group. */
int qd_cuts_symbols(int fmt, uint64_t sample_rate, uint64_t n_samples, const void *src, int src_mem,
                    uint64_t src_first, uint64_t src_count, const qd_cut *cuts, size_t n_cuts,
                    const qd_symbols_desc *desc, uint8_t *out, int out_mem, const qd_plan_options *options, void *stream);

/* Host-side figures of the most recent host-resident run of the plan (qd_plan_run with host buffers, or one shard of
 * qd_plan_run_sharded): the survey's qd_plan_stats. */
typedef struct {
    double   wall_ms;            /* whole call */
    double   stage_ms;           /* host time in the pageable <-> pinned staging copies (0 for QD_MEM_HOST_PINNED) */
    uint64_t bytes_h2d, bytes_d2h;
    uint32_t chunks;
    uint32_t _pad;
} qd_plan_stats;
int qd_plan_get_stats(const qd_plan *plan, qd_plan_stats *stats);

/* Pinned host memory for QD_MEM_HOST_PINNED: allocate, or register memory the caller already has (an mmap'ed file). */
int qd_host_alloc(size_t bytes, void **ptr);
int qd_host_free(void *ptr);
int qd_host_register(void *ptr, size_t bytes);
int qd_host_unregister(void *ptr);

/* HIP-event timing of the chain kernel of the most recent device-resident qd_plan_run,
 * taken on the stream it was launched on.  Enable before the run; the query synchronises. */
int qd_plan_set_timing(qd_plan *plan, int enabled);
int qd_plan_last_kernel_ms(qd_plan *plan, float *ms);

/* Device buffers for callers that keep a stream resident in HBM — e.g. `gen ... | lowpass | sparkfft`
 * (src/gen.rs + BASELINE configs[3]): the samples are generated on the device by qd_gen and never cross PCIe.
 * Plain hipMalloc / hipFree / hipMemcpy behind the ABI so that a host without a HIP toolchain can use
 * qd_plan_run's device path.  qd_device_copy is synchronous; *_mem are qd_mem values. */
int qd_device_alloc(size_t bytes, void **ptr);
int qd_device_free(void *ptr);
int qd_device_copy(void *dst, int dst_mem, const void *src, int src_mem, size_t bytes);

/* Fill a device (or host) buffer with Gen's samples, src/gen.rs:35-47 (device-side source
 * for `gen ... sparkfft` chains; A9). */
int qd_gen(const int64_t *cos_hz, size_t n_cos, uint64_t sample_rate, uint64_t first, size_t n,
           qd_c32 *out, int mem);

#ifdef __cplusplus
}
#endif
#endif
