// quadrs_hip.hip — C ABI (include/quadrs_hip.h) + host-side planning for the gfx950 engine.
//
// Host responsibilities (all O(plan), none per-sample): validate the chain the way the
// reference's constructors do, design the taps with the platform libm (src/filter.rs:86-105 —
// the reference does this on the host too), lay out twiddles, build the NCO tables on the
// device, pick the tile geometry, launch.  Per-sample work lives in qd_chain.h / qd_device.h.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <map>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <numeric>
#include <optional>
#include <thread>
#include <algorithm>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <tuple>
#include <string>
#include <vector>

#include "../../include/quadrs_hip.h"
#include "qd_chain.h"
#include "qd_cascade.h"
#include "qd_registry.h"
#include "qd_summary.h"
#include "qd_pool.h"
#include "qd_density.h"
#include "qd_mean.h"
#include "qd_power.h"
#include "qd_spread.h"
#include "qd_bands.h"
#include "qd_bursts.h"
#include "qd_emissions.h"
#include "qd_cuts.h"
#include "qd_symbols.h"
#include "qd_paint.h"

using namespace qd;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) return fail(QD_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e__)); \
    } while (0)

constexpr double kPi64 = 3.14159265358979323846264338327950288;
constexpr float kPi32 = 3.14159265358979323846264338327950288f;

// Tuning / ablation knobs read from the environment exist in development builds only (-DQD_DEVELOP:
// libquadrs_hip_dev.so, used by scripts/); the shipped library takes its policy from qd_plan_options.
#ifdef QD_DEVELOP
const char *dev_env(const char *name) { return getenv(name); }
#else
const char *dev_env(const char *) { return nullptr; }
#endif

uint32_t ilog2(uint64_t v) { uint32_t l = 0; while ((1ull << l) < v) ++l; return l; }
bool is_pow2(uint64_t v) { return v && !(v & (v - 1)); }

int spl_of(int fmt) { return fmt == QD_FMT_CF32 ? 2 : 4; }
int bps_of(int fmt) { return fmt == QD_FMT_CF32 ? 8 : (fmt == QD_FMT_CS16 ? 4 : 2); }

// ------------------------------------------------------------------ small kernels

// Row bases: (cos, sin) of the exact product (row*ROW) * ratio, nf itself and fl(cos + sin) (qd_nco.h, nco_row_entry).
// (n_off: the row grid of a stream that starts n_off samples into the plan's — the interleaved launches of overlapping lowpass-free windows)
__global__ void k_rowtab(double ratio, uint32_t row_len, uint64_t row0, uint64_t n_rows, uint64_t n_off, RowBase *out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    out[i] = nco_row_entry((double)((row0 + i) * (uint64_t)row_len + n_off), ratio);
}

// Lane table: the lane entries (c, c + s, s - c) of (c, s) = (cos, sin) of the exact product j * ratio (qd_nco.h, nco_lane_entry)
__global__ void k_jtab(double ratio, uint32_t n, LaneEntry *out) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    out[j] = nco_lane_entry((double)j, ratio);
}

// FileFormat::to_cf32 per sample (src/lib.rs:231-255)
__global__ void k_unpack(int fmt, const uint8_t *src, size_t n, float2 *out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float2 v;
        switch (fmt) {
        case 0: v = *reinterpret_cast<const float2 *>(src + i * 8); break;
        case 1: { uint16_t w = *reinterpret_cast<const uint16_t *>(src + i * 2); v = make_float2(unpack_cs8(w & 0xff), unpack_cs8(w >> 8)); break; }
        case 2: { uint16_t w = *reinterpret_cast<const uint16_t *>(src + i * 2); v = make_float2(unpack_cu8(w & 0xff), unpack_cu8(w >> 8)); break; }
        default: { uint32_t w = *reinterpret_cast<const uint32_t *>(src + i * 4); v = make_float2(unpack_cs16(w & 0xffffu), unpack_cs16(w >> 16)); break; }
        }
        out[i] = v;
    }
}

// Shift::read_at's loop over an arbitrary block (src/shift.rs:48-52), rows of 512 samples.
__global__ __launch_bounds__(256) void k_shift(float2 *buf, uint64_t abs_off, uint64_t n, double ratio,
                                                const RowBase *rowtab, uint64_t row0, uint64_t n_rows,
                                                const LaneEntry *jtab, int second_order) {
    constexpr uint32_t ROW = 512;
    const uint32_t tid = threadIdx.x;
    LaneRot lr[2];
    for (int u = 0; u < 2; ++u) {
        uint32_t j = tid * 2 + u;
        lr[u] = nco_lane_rot((double)j, jtab[j]);
    }
    for (uint64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const RowBase rb = rowtab[r];
        for (int u = 0; u < 2; ++u) {
            uint64_t idx = (row0 + r) * ROW + tid * 2 + u;
            if (idx >= abs_off && idx < abs_off + n) {
                float2 m = second_order ? nco_mul<true>(rb, lr[u], ratio) : nco_mul<false>(rb, lr[u], ratio);
                buf[idx - abs_off] = cmul(buf[idx - abs_off], m);
            }
        }
    }
}

// LowPass::read_at on a fetched block (src/filter.rs:68-83,107-124): one lane per kept output.
__global__ void k_lowpass_block(const float *__restrict__ taps, uint32_t T, uint64_t D, const float2 *__restrict__ raw,
                                uint64_t valid, float2 *out, uint64_t out_n) {
    const uint64_t c = T - T / 2;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < out_n; k += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t base = k * D + c;
        uint64_t jmax = valid - base < T ? valid - base : T;
        float ar = 0.f, ai = 0.f;
        for (uint64_t j = 0; j < jmax; ++j) {
            float2 x = raw[base + j];
            float h = taps[j];
            ar = ar + x.x * h;
            ai = ai + x.y * h;
        }
        out[k] = make_float2(ar, ai);
    }
}

// Gen::read_at (src/gen.rs:35-47)
__global__ void k_gen(const int64_t *cos_hz, uint32_t n_cos, uint64_t sample_rate, uint64_t first, size_t n, float2 *out) {
    const double tau = kPi64 * 2.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double base = (double)(first + i) * tau / (double)sample_rate;
        float vr = 0.f, vi = 0.f;
        for (uint32_t k = 0; k < n_cos; ++k) {
            double f = (double)cos_hz[k] * base;
            double s, c;
            sincos(f, &s, &c);
            vr = vr + (float)c;
            vi = vi + (float)s;
        }
        out[i] = make_float2(vr, vi);
    }
}

// take_fft at a width that is not a power of two (src/ffts.rs:25: FftPlanner::plan_fft_forward takes any length; the
// egui slider offers 4..4096, src/eui/mod.rs:157).  Bluestein's chirp-z form: X[k] = c[k] * sum_n (x[n] c[n]) b[k-n],
// c[n] = e^{-i pi n^2 / W}, b = conj(c) — a circular convolution of length M >= 2W-1 (a power of two), done in LDS as
// forward radix-2 DIF (natural in, bit-reversed out) -> pointwise product with the precomputed spectrum of b (stored
// bit-reversed, 1/M folded in) -> inverse radix-2 DIT (bit-reversed in, natural out): no permutation pass.
// One workgroup per output row.  rustfft's own result for such lengths depends on the planner's decomposition and the
// host's SIMD code path, so there is no bit pattern to match (PARITY UNPINNED).  The convolution is therefore carried in
// f64 (the f32 window product of src/ffts.rs:64-68 first, exactly as the reference forms it): the bins come out as the
// mathematically exact DFT of the windowed f32 samples rounded once to f32 — an f32 Bluestein would sit 5-10x further from
// the exact answer than rustfft's mixed-radix paths do on smooth lengths.  Cost: ~1 ms for 2048 rows at M = 8192.
__device__ __forceinline__ double2 zmul(double2 a, double2 b) {
    return make_double2(__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.x, b.y, a.y * b.x));
}
// The loader (FMT, NCO): a row behind `from [shift]` is unpacked and shifted while it is loaded, with the chain kernels' operations —
// unpack_*, nco_mul over the absolute sample index (rows of 512 samples, as k_shift), cmul_pk.  <0, 0> loads cf32 as it always did.
struct BlueSrc {
    const uint8_t *in; uint64_t in_first;      // raw bytes of source sample in_first
    double ratio; const RowBase *rowtab; uint64_t rowtab_row0; const LaneEntry *jtab;     // NCO != 0 only
};
template <int FMT, int NCO>
__global__ __launch_bounds__(256) void k_bluestein(const BlueSrc src, const uint64_t *__restrict__ offs,
                                                   const float *__restrict__ win, uint32_t W, uint32_t M, uint32_t logM,
                                                   const double2 *__restrict__ chirp, const double2 *__restrict__ Bbr,
                                                   const double2 *__restrict__ tw, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_b[];
    double2 *buf = reinterpret_cast<double2 *>(smem_b);
    const uint32_t tid = threadIdx.x;
    const uint64_t row = blockIdx.x;
    const uint64_t n0 = offs[row];
    for (uint32_t n = tid; n < M; n += 256) {
        double2 v = make_double2(0.0, 0.0);
        if (n < W) {
            const uint64_t na = n0 + n;
            const uint8_t *sp = src.in + (na - src.in_first) * (uint64_t)FmtTraits<FMT>::BPS;
            float2 xv;
            if constexpr (FMT == 0) xv = *reinterpret_cast<const float2 *>(sp);
            else if constexpr (FMT == 1) { const uint32_t w = *reinterpret_cast<const uint16_t *>(sp); xv = make_float2(unpack_cs8(w & 0xff), unpack_cs8(w >> 8)); }
            else if constexpr (FMT == 2) { const uint32_t w = *reinterpret_cast<const uint16_t *>(sp); xv = make_float2(unpack_cu8(w & 0xff), unpack_cu8(w >> 8)); }
            else { const uint32_t w = *reinterpret_cast<const uint32_t *>(sp); xv = make_float2(unpack_cs16(w & 0xffffu), unpack_cs16(w >> 16)); }
            if constexpr (NCO != 0) {
                const uint32_t j = (uint32_t)(na & 511u);
                const RowBase rb = src.rowtab[(na >> 9) - src.rowtab_row0];
                const LaneRot lr = nco_lane_rot((double)j, src.jtab[j]);
                xv = cmul_pk(xv, nco_mul<NCO == 2>(rb, lr, src.ratio));        // buf[i] *= mul (src/shift.rs:51)
            }
            if (win) xv = cscale(xv, win[n]);         // *sample *= w_val (src/ffts.rs:64-68), Complex<f32> * f32, f32-rounded
            v = zmul(make_double2((double)xv.x, (double)xv.y), chirp[n]);
        }
        buf[n] = v;
    }
    __syncthreads();
    for (uint32_t sh = logM; sh-- > 0;) {             // DIF, half-span h = 2^sh
        const uint32_t h = 1u << sh;
        for (uint32_t t = tid; t < M / 2; t += 256) {
            const uint32_t j = t & (h - 1), i = ((t >> sh) << (sh + 1)) | j;
            const double2 u = buf[i], v = buf[i + h];
            buf[i] = make_double2(u.x + v.x, u.y + v.y);
            buf[i + h] = zmul(make_double2(u.x - v.x, u.y - v.y), tw[j << (logM - 1 - sh)]);
        }
        __syncthreads();
    }
    for (uint32_t r = tid; r < M; r += 256) buf[r] = zmul(buf[r], Bbr[r]);
    __syncthreads();
    for (uint32_t sh = 0; sh < logM; ++sh) {          // DIT with conjugate twiddles
        const uint32_t h = 1u << sh;
        for (uint32_t t = tid; t < M / 2; t += 256) {
            const uint32_t j = t & (h - 1), i = ((t >> sh) << (sh + 1)) | j;
            const double2 w = tw[j << (logM - 1 - sh)];
            const double2 u = buf[i], v = zmul(buf[i + h], make_double2(w.x, -w.y));
            buf[i] = make_double2(u.x + v.x, u.y + v.y);
            buf[i + h] = make_double2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
    const uint32_t half = W / 2;                       // skip(W/2).chain(take(W/2)), src/ffts.rs:72-78
    for (uint32_t k = tid; k < W; k += 256) {
        const double2 y = zmul(buf[k], chirp[k]);
        const uint32_t pos = k >= half ? k - half : k + (W - half);
        out[row * W + pos] = norm_ref(make_float2((float)y.x, (float)y.y));     // the FFT result is Complex<f32>; norm() = hypotf
    }
}

// ------------------------------------------------------------------ host arithmetic taken over from the reference

// src/filter.rs:86-105 with cutoff from :126-128,:31 — f32 throughout, platform libm
void design_taps(uint64_t frequency, uint64_t sample_rate, size_t size, float *out) {
    float cutoff = (float)((double)frequency / (double)sample_rate);
    float sz1 = (float)size - 1.0f;
    for (size_t i = 0; i < size; ++i) {
        float fi = (float)i;
        float a1 = (2.0f * kPi32) * fi / sz1;
        float a2 = (4.0f * kPi32) * fi / sz1;
        float window = 0.42f - 0.5f * std::cos(a1) + 0.08f * std::cos(a2);
        float x = 2.0f * cutoff * (fi - sz1 / 2.0f);
        float xp = x * kPi32;
        float wave = std::sin(xp) / xp;
        out[i] = wave * window;
    }
    float sum = 0.0f;
    for (size_t i = 0; i < size; ++i) sum += out[i];
    for (size_t i = 0; i < size; ++i) out[i] = out[i] / sum;
}

// rustfft twiddles::compute_twiddle, Forward
float2 compute_twiddle(size_t index, size_t fft_len) {
    double constant = -2.0 * kPi64 / (double)fft_len;
    double angle = constant * (double)index;
    return make_float2((float)std::cos(angle), (float)std::sin(angle));
}

struct FftLayout {
    uint32_t base_len = 1, log_base = 0, layers = 0;
    std::vector<float2> tw;
};

// Radix4::new: exponent 0..3 -> base 1,2,4,8; else odd -> 8, even -> 16
FftLayout fft_layout(uint64_t W) {
    FftLayout L;
    uint32_t e = ilog2(W);
    uint32_t be = e <= 3 ? e : ((e & 1) ? 3 : 4);
    L.log_base = be; L.base_len = 1u << be; L.layers = (e - be) / 2;
    size_t cross = L.base_len;
    while (cross < W) {
        size_t cols = cross;
        cross *= 4;
        for (size_t i = 0; i < cols; ++i)
            for (size_t k = 1; k < 4; ++k) L.tw.push_back(compute_twiddle(i * k, cross));
    }
    return L;
}


#ifdef QD_DEV_FAST   // development builds: cf32 only, to keep hipcc turnaround short
#define QD_FMT_CASES(X) case 0: return X(0);
#else
#define QD_FMT_CASES(X) case 0: return X(0); case 1: return X(1); case 2: return X(2); case 3: return X(3);
#endif

// ---- generic kernels (DynGeo): every shape; chunked prefetch of 4 rows; aligned / unaligned slab
// Register budget of the runtime-geometry kernels: four waves per SIMD (128 VGPRs).  Round 3's builds spilled there once a shift was in
// the chain (up to 74 VGPRs / 108 bytes of scratch per lane on the cs16 and second-order instantiations, reloaded behind vmcnt(0)
// drains in the tile loop).  Round 4: the lane constants are re-read from the (L2-resident) lane table at the top of every tile
// instead of held across it (k_chain kReloadLane) — no scratch at four waves for the first-order NCO; the second-order kernels (streams
// past 2^28 rad of phase, which get a plan-time build anyway) are budgeted for three.  Budgeting ALL shifted kernels for three waves
// removed the scratch too but cost 6-18 % on 256 MiB streams (profiles/r04/generic_rate.log).  tests/test_abi_cpu.py audits every kernel.
// The three-multiplication rotation keeps a fourth double per sample slot (LaneRot): with cs16's four slots a lane and its two-dword
// unpack the first-order kernels no longer fit four waves either (6-14 VGPRs of scratch), so cs16 with a shift is budgeted for three.
constexpr int dyn_lb(int nco, int fmt = 0) { return (nco == 2 || (nco == 1 && fmt == 3)) ? 3 : 4; }
template <int F, int NCO, bool FI, class G = DynGeo>
chain_fn pick_dyn(bool aligned) {
    return aligned ? k_chain<F, NCO, G, FI, 4, false, true, dyn_lb(NCO, F)> : k_chain<F, NCO, G, FI, 4, false, false, dyn_lb(NCO, F)>;
}

// (windowed plans behind a lowpass: the WinGeo instantiations; without a lowpass the DynGeo kernels test ChainParams::window themselves)
template <int F>
chain_fn pick_fmt(int nco, bool fir, bool aligned, bool windowed) {
    if (windowed && fir) {
        switch (nco) {
        case 0: return pick_dyn<F, 0, true, WinGeo>(aligned);
        case 1: return pick_dyn<F, 1, true, WinGeo>(aligned);
        default: return pick_dyn<F, 2, true, WinGeo>(aligned);
        }
    }
    switch (nco) {
    case 0: return fir ? pick_dyn<F, 0, true>(aligned) : pick_dyn<F, 0, false>(aligned);
    case 1: return fir ? pick_dyn<F, 1, true>(aligned) : pick_dyn<F, 1, false>(aligned);
    default: return fir ? pick_dyn<F, 2, true>(aligned) : pick_dyn<F, 2, false>(aligned);
    }
}

chain_fn pick_generic(int fmt, int nco, bool fir, bool aligned, bool windowed = false) {
#define QD_X(F) pick_fmt<F>(nco, fir, aligned, windowed)
    switch (fmt) { QD_FMT_CASES(QD_X) }
#undef QD_X
    return nullptr;
}

// ---- row mode (QD_EPI_ROWS_F32): the per-sample runtime-geometry kernel over irregular rows (RowGeo, qd_chain.h)
template <int F>
chain_fn pick_rows_fmt(int nco, bool fir) {
    switch (nco) {
    case 0: return fir ? k_chain<F, 0, RowGeo, true, 4, false, false, dyn_lb(0)> : k_chain<F, 0, RowGeo, false, 4, false, false, dyn_lb(0)>;
    case 1: return fir ? k_chain<F, 1, RowGeo, true, 4, false, false, dyn_lb(1)> : k_chain<F, 1, RowGeo, false, 4, false, false, dyn_lb(1)>;
    default: return fir ? k_chain<F, 2, RowGeo, true, 4, false, false, dyn_lb(2)> : k_chain<F, 2, RowGeo, false, 4, false, false, dyn_lb(2)>;
    }
}
chain_fn pick_rows(int fmt, int nco, bool fir) {
#define QD_X(F) pick_rows_fmt<F>(nco, fir)
    switch (fmt) { QD_FMT_CASES(QD_X) }
#undef QD_X
    return nullptr;
}

// ---- k_bluestein's loaders
typedef void (*blue_fn)(const BlueSrc, const uint64_t *, const float *, uint32_t, uint32_t, uint32_t, const double2 *, const double2 *, const double2 *, float *);
template <int F>
blue_fn pick_blue_fmt(int nco) { return nco == 0 ? k_bluestein<F, 0> : (nco == 1 ? k_bluestein<F, 1> : k_bluestein<F, 2>); }
blue_fn pick_blue(int fmt, int nco) {
#define QD_X(F) pick_blue_fmt<F>(nco)
    switch (fmt) { QD_FMT_CASES(QD_X) }
#undef QD_X
    return nullptr;
}

// ---- chains without a lowpass, windows side by side: the wave-local kernel (k_spark, qd_chain.h); runtime width, tiles of 1024 samples
template <int F, int TS>
chain_fn pick_spark_ts(int nco) {
    constexpr int NCH = TS / (int)SparkTraits<F>::CH;
    switch (nco) {                              // chains with a shift: register budget of three (two) waves per SIMD, see spark_lb
    case 0: return k_spark<F, 0, DynGeo, NCH, 4>;
    case 1: return k_spark<F, 1, DynGeo, NCH, (TS == 512 ? 3 : 2)>;
    default: return k_spark<F, 2, DynGeo, NCH, 2>;
    }
}
// waves per SIMD the built-in kernel is register-budgeted for (= workgroups per CU): without a shift 128 VGPRs hold everything;
// with one, the lane constants of the row quarters (16 doubles), the NCO's f64 temporaries and the next tile's prefetch beside the
// sixteen-point butterflies need ~150 (tiles of 512 samples) / ~190 (1024): budgeted at 4 they spill 9-85 registers to scratch
int spark_lb(uint32_t ts, int nco) { return nco == 0 ? 4 : (nco == 1 && ts == 512 ? 3 : 2); }
// tile sizes of the built-in (runtime-width) kernels: 1024 samples per wave, which fills the lanes of the sixteen-point base
// butterflies too; chains WITH a shift take 512 up to W = 512 — their lane constants (16 doubles) and the NCO's f64 temporaries on top
// of 1024 samples of prefetch do not fit 128 registers (61-85 spilled), with 512 they do
uint32_t spark_tile(uint32_t W, int nco) { return (nco != 0 && W <= 512) ? 512u : 1024u; }
chain_fn pick_spark(int fmt, int nco, uint32_t ts) {
#define QD_X(F) (ts == 512 ? pick_spark_ts<F, 512>(nco) : pick_spark_ts<F, 1024>(nco))
    switch (fmt) { QD_FMT_CASES(QD_X) }
#undef QD_X
    return nullptr;
}

// ---- shape-specialised kernels (FixedGeo): the chain shapes of BASELINE.json / the README.
// Same source as the generic kernel with W,S,D,T,G as compile-time constants.
const FixedEntry kFixed[] = {
    // configs[1]  "shift 280000 | lowpass -power 20 -decimate 16 2000000 | sparkfft -width 128"   (README.md:57-63)
    // round 3: row-aligned phase 1 (bit 3) WITH non-temporal stream loads (bit 8): 0.232 -> 0.212 ms on one box, 0.233 -> 0.227 on another
    // (profiles/r03/sweep_cfg2_nt.log; round 2 measured the row-aligned phase 1 alone 1.5 % slower, and it still is without nt)
    // + bit 16: the tile's first and last row — the ones the neighbouring tile reads as well — keep the default cache policy (L2 hits
    //   for the second reader), the seven rows in between go non-temporal: 0.200 -> 0.191 ms (profiles/r03/sweep_nt_inner.log)
    QD_FIXED_FB(0, 1, 128, 128, 16, 40, 2, 9, true, 4, 1, 1, 65800, "cfg2"),
    QD_FIXED_FB(0, 2, 128, 128, 16, 40, 2, 9, true, 4, 1, 1, 65800, "cfg2"),
    // north_star target sentence: 200-tap FIR decimate 32 -> 128-pt FFT
    // packed lane-per-output FIR on a 16-byte-row tile (FixedGeo FLAGS_ bit 2, PAD 2): half the VALU instructions of the FIR
    // + row-aligned fast phase 1 (bit 3): buffer loads with a per-tile descriptor, compile-time row offsets
    // + deferred FFT (bit 6, two FFT slots): the previous tile's FFT + epilogue on a wave the FIR leaves idle
    // + nt stream loads (bit 8): the slab is read once; the non-temporal policy measured 1.0-1.2 % over the default on three boxes
    //   (profiles/r03/sweep_cfg3p_load_policy.log; sc0 / sc1 on top of it: nothing)
    // + bit 16: first and last row of the tile (shared with the neighbouring tiles) at the default policy: another 1.0 %
    QD_FIXED_FB(0, 1, 128, 128, 32, 200, 1, 9, true, 4, 2, 2, 65868, "cfg3p"),
    QD_FIXED_FB(0, 2, 128, 128, 32, 200, 1, 9, true, 4, 2, 2, 65868, "cfg3p"),
    // README.md:90-94 / configs[2] / configs[4] (64-pt windows, stride 16, 400 taps): the STREAMING three-stage kernel
    // (k_chain_pipe3s, FLAGS 32 | 256 | 32768 | 131072): eight producer waves, the shared-FIR waves and four FFT waves work one step
    // apart on a contiguous run of tiles per workgroup; shifted samples and decimated outputs are carried from tile to tile in LDS
    // rings, so a step shifts and filters only what is NEW (a 12-window tile of the plain three-stage kernel repeated 31 % of its
    // phase 1 and 25 % of its FIR).  cf32 (cfg5, 16 GiB per GPU): one-tile-per-CU kernel 7.50 ms -> three-stage 6.71 -> streaming,
    // 14-window steps 5.7 ms; cs8 (cfg3): 25.6 -> 22 ms (12-window steps: 16 would need 174 KiB of LDS).  Identical bytes
    // (profiles/r03/sweep_stream.log).  nt = 512: rows of 512 producer threads; the launch adds 512 consumer threads.
    { 0, 1, 64, 16, 32, 400, 14, 4, 512, 2, 1, 164128,
      qd::k_chain_pipe3s<0, 1, qd::FixedGeo<64, 16, 32, 400, 14, 8, 1, 2, 1, 164128>, 7, 4>, "fsk5" },
    { 0, 2, 64, 16, 32, 400, 14, 4, 512, 2, 1, 164128,
      qd::k_chain_pipe3s<0, 2, qd::FixedGeo<64, 16, 32, 400, 14, 8, 1, 2, 1, 164128>, 7, 4>, "fsk5" },
#ifndef QD_DEV_FAST
    // cs8 input (HackRF) of the same chain: four producer waves (rows of 256 threads x 4 samples = 1024 samples, seven per step) so that
    // 14-window steps start on row boundaries like the cf32 form's (rows of 2048 samples admit 12 or 16 windows, and 16 do not fit)
    { 1, 1, 64, 16, 32, 400, 14, 4, 256, 2, 1, 164128,
      qd::k_chain_pipe3s<1, 1, qd::FixedGeo<64, 16, 32, 400, 14, 8, 1, 2, 1, 164128>, 7, 4, 256>, "cfg3" },
    { 1, 2, 64, 16, 32, 400, 14, 4, 256, 2, 1, 164128,
      qd::k_chain_pipe3s<1, 2, qd::FixedGeo<64, 16, 32, 400, 14, 8, 1, 2, 1, 164128>, 7, 4, 256>, "cfg3" },
#endif
    // configs[3]  512-tap FIR decimate 8 -> 1024-pt FFT (no shift)
    // 70 KiB tile: one workgroup per CU, so give it 1024 threads (16 waves/CU); 5 rows of 2048 samples
    // FLAGS 128 (kGeoPackedTile): the two-outputs-per-lane FIR as straight-line packed code, truncated outputs as in-chain
    // snapshots (no helper wave): 37.1 -> 24.9 ms
    // + FLAGS 64 with two FFT slots: the previous window's FFT + epilogue on four of the eight waves the FIR leaves idle -> 23.9 ms
    // + FLAGS 8: row-aligned phase 1 (a window is four rows of 2048 samples + 512) -> 23.3 ms
    // round 3, FLAGS 8192: HALF-window tiles — the raw buffer holds the input of 512 outputs, a window is filtered in two passes into
    // one FFT slot; 512 threads (4 FIR waves + the four-wave deferred FFT), 74 KiB, so TWO workgroups share a CU and one's phase 1 +
    // barriers (8 k of its 29 k cycles per window) run under the other's FIR: 23.1 -> 22.0 ms, now at the package power cap too
    // (1390 W; the clock went from 2.32 to 2.19 GHz — profiles/r03/sweep_cfg4_half.log)
    { 0, 0, 1024, 1024, 8, 512, 1, 4, 512, 2, 2, 8392,
      qd::k_chain<0, 0, qd::FixedGeo<1024, 1024, 8, 512, 1, 4, 2, 2, 2, 8392>, true, 5, true, true, 4, 512>, "cfg4" },
};

const FixedEntry *find_fixed(int fmt, int nco, uint32_t W, uint32_t S, uint32_t D, uint32_t T) {
    for (const FixedEntry &e : kFixed)
        if (e.fmt == fmt && e.nco == nco && e.W == W && e.S == S && e.D == D && e.T == T) return &e;
    return nullptr;
}

// ---- plan-time specialisation (hiprtc): any chain shape gets a FixedGeo build of the same kernel source.
// The headers are read from <dir of this .so>/csrc (the in-tree layout); compiled modules are cached per
// process and on disk (below).  qd_plan_options.kernel_policy decides whether a plan builds: QD_KERNEL_NO_PLAN_TIME /
// QD_KERNEL_GENERIC never; by default a cached build is always used, and a new one is compiled (~0.3-1 s) for
// streams of 1 GiB and more, for tile hints and for QD_MODE_FAST (QD_KERNEL_SPECIALISE: always).
struct JitKey {
    int fmt, nco, fir, rch, whole, lb, nt; uint32_t W, S, D, T, G; uint32_t firb = 8, firr = 1; int noslp = 0; uint32_t pad = 1, batch = 1, flags = 0;
    int epi = 0;                   // kernels that take the sink as a template argument (k_spark2)
    bool operator<(const JitKey &o) const {
        return std::tie(fmt, nco, fir, rch, whole, lb, nt, W, S, D, T, G, firb, firr, noslp, pad, batch, flags, epi) <
               std::tie(o.fmt, o.nco, o.fir, o.rch, o.whole, o.lb, o.nt, o.W, o.S, o.D, o.T, o.G, o.firb, o.firr, o.noslp, o.pad, o.batch, o.flags, o.epi);
    }
};
std::mutex g_jit_mu;
// A hipFunction_t belongs to the module hipModuleLoadData loaded on the device that was current then: one entry per (device,
// key).  The on-disk code object is shared, only the load is repeated per device (one-process multi-device plans,
// qd_plan_options.shard_device[]; that path is unexercised until a multi-GPU box is available — DESIGN.md section 8).
std::map<std::pair<int, JitKey>, hipFunction_t> g_jit_cache;
// builds that FAILED in this process (a hiprtc error, a static_assert of the kernel): remembered with their message, so that every later plan of the shape falls back at once instead of paying the compile again
std::map<std::pair<int, JitKey>, std::string> g_jit_failed;

std::string csrc_dir() {
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void *>(&csrc_dir), &info) || !info.dli_fname) return "";
    std::string path(info.dli_fname);
    size_t slash = path.rfind('/');
    return (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/csrc";
}

// ---- on-disk cache of plan-time builds: a compile costs ~0.3-1 s, which a single pass over anything smaller than tens
// of GiB never repays; a cached code object loads in ~1 ms.  Directory: $QD_JIT_CACHE ("0" / "off" disables), else
// $XDG_CACHE_HOME/quadrs_hip, else $HOME/.cache/quadrs_hip.  File name: FNV-1a of (kernel name, options, the kernel
// headers' contents); file = "QDJIT1\n<lowered name>\n" + code object.  Every failure just means "not cached".
uint64_t fnv1a(const void *data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
bool read_file(const std::string &path, std::vector<char> *out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    if (n < 0) { fclose(f); return false; }
    out->resize((size_t)n);
    const bool ok = n == 0 || fread(out->data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}
std::string jit_cache_dir() {
    std::string d;
    if (const char *e = getenv("QD_JIT_CACHE")) {
        if (!*e || !strcmp(e, "0") || !strcmp(e, "off")) return "";
        d = e;
    } else if (const char *x = getenv("XDG_CACHE_HOME")) { if (*x) d = std::string(x) + "/quadrs_hip"; }
    if (d.empty()) { const char *h = getenv("HOME"); if (!h || !*h) return ""; d = std::string(h) + "/.cache/quadrs_hip"; }
    for (size_t i = 1; i <= d.size(); ++i)                       // mkdir -p; errors surface as "cannot write" later
        if (i == d.size() || d[i] == '/') (void)mkdir(d.substr(0, i).c_str(), 0755);
    return d;
}

// returns nullptr (and leaves a message in *why) when specialisation is not possible; with may_compile false only the
// in-process and on-disk caches are consulted
hipFunction_t jit_chain_kernel(const JitKey &k, std::string *why, bool may_compile = true) {
    std::lock_guard<std::mutex> lock(g_jit_mu);
    int jit_dev = 0;
    (void)hipGetDevice(&jit_dev);
    const std::pair<int, JitKey> dk(jit_dev, k);
    auto it = g_jit_cache.find(dk);
    if (it != g_jit_cache.end()) return it->second;
    if (auto bad = g_jit_failed.find(dk); bad != g_jit_failed.end()) { *why = bad->second; return nullptr; }
    const std::string dir = csrc_dir();
    std::vector<char> hdrs[4];            // everything a plan-time build includes: the cache key hashes their contents
    const char *const hdr_names[4] = {"/qd_chain.h", "/qd_device.h", "/qd_geometry.h", "/qd_nco.h"};
    for (int i = 0; i < 4; ++i)
        if (!read_file(dir + hdr_names[i], &hdrs[i])) {
            *why = "kernel headers not found next to the library (" + dir + ")";
            return nullptr;
        }
    // "<family><fmt, [nco,] FixedGeo<...>, <the family's own trailing arguments>>"
    char geo[160], tail[64], name[512];
    snprintf(geo, sizeof geo, "qd::FixedGeo<%u, %u, %u, %u, %u, %u, %u, %u, %u, %u>", k.W, k.S, k.D, k.T, k.G, k.firb, k.firr, k.pad, k.batch, k.flags);
    const Family fam = family_of(k.flags);
    switch (fam) {
    case kFamSpark0: case kFamSpark2: snprintf(tail, sizeof tail, "%d, %d", k.lb, k.epi); break;                  // the sink is a template argument
    case kFamSpark: snprintf(tail, sizeof tail, "%d, %d, %d", k.rch, k.lb, k.epi); break;                          // rch = chunks per tile
    case kFamPipe3s: snprintf(tail, sizeof tail, "%d, %d, %d", k.rch, k.lb, k.nt); break;                          // rch = rows per step, nt = producer threads
    case kFamPipe3: snprintf(tail, sizeof tail, "%d, %d", k.rch, k.lb); break;
    default: snprintf(tail, sizeof tail, "%s, %d, %s, true, %d, %d", k.fir ? "true" : "false", k.rch, k.whole ? "true" : "false", k.lb, k.nt); break;
    }
    if (fam == kFamSpark0) snprintf(name, sizeof name, "%s<%d, %s, %s>", family_name(k.flags), k.fmt, geo, tail);      // (no shift: no NCO argument)
    else snprintf(name, sizeof name, "%s<%d, %d, %s, %s>", family_name(k.flags), k.fmt, k.nco, geo, tail);
    const std::string src = std::string("#include \"qd_chain.h\"\ntemplate __global__ void ") + name + "(const qd::ChainParams);\n";
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "qd_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) { *why = "hiprtcCreateProgram failed"; return nullptr; }
    hiprtcAddNameExpression(prog, name);
    const std::string inc = "-I" + dir;
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", inc.c_str(),
                          "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"};      // see build.py: the tile queue's claim stays one plain atomic
    std::vector<const char *> optv(opts, opts + sizeof opts / sizeof opts[0]);
#ifdef QD_STAMP
    optv.push_back("-DQD_STAMP");
#endif
#ifdef QD_DEVELOP
    optv.push_back("-DQD_DEVELOP");
#endif
#ifdef QD_WGTIME
    optv.push_back("-DQD_WGTIME");
#endif
    if (k.noslp || dev_env("QD_JIT_NOSLP")) optv.push_back("-fno-slp-vectorize");   // scalar f32 accumulate chains of the long-filter policy
    std::vector<std::string> extra;                          // development: QD_JIT_FLAGS="-mllvm -foo ..." appended verbatim
    if (const char *e = dev_env("QD_JIT_FLAGS")) {
        std::string cur;
        for (const char *c = e;; ++c) {
            if (*c == ' ' || *c == 0) { if (!cur.empty()) extra.push_back(cur); cur.clear(); if (!*c) break; }
            else cur.push_back(*c);
        }
        for (const std::string &x : extra) optv.push_back(x.c_str());
    }
    // cache lookup (the -I path is excluded from the key: the headers' contents are in it)
    std::string cache_file;
    {
        uint64_t h = fnv1a(name, strlen(name));
        h = fnv1a(src.data(), src.size(), h);
        int rtc_major = 0, rtc_minor = 0;                      // a code object does not outlive the compiler that made it
        (void)hiprtcVersion(&rtc_major, &rtc_minor);
        h = fnv1a(&rtc_major, sizeof rtc_major, h);
        h = fnv1a(&rtc_minor, sizeof rtc_minor, h);
        for (const char *o : optv) if (o != inc.c_str()) h = fnv1a(o, strlen(o) + 1, h);
        for (const std::vector<char> &hd : hdrs) h = fnv1a(hd.data(), hd.size(), h);
        const std::string cdir = dev_env("QD_JIT_DUMP") ? std::string() : jit_cache_dir();
        if (!cdir.empty()) { char fn[64]; snprintf(fn, sizeof fn, "/%016llx.co", (unsigned long long)h); cache_file = cdir + fn; }
    }
    if (!cache_file.empty()) {
        std::vector<char> blob;
        if (read_file(cache_file, &blob) && blob.size() > 8 && !memcmp(blob.data(), "QDJIT1\n", 7)) {
            const char *nm = blob.data() + 7, *end = static_cast<const char *>(memchr(nm, '\n', blob.size() - 7));
            if (end) {
                const std::string lowered(nm, end);
                hipModule_t mod; hipFunction_t fn = nullptr;
                if (hipModuleLoadData(&mod, end + 1) == hipSuccess && hipModuleGetFunction(&fn, mod, lowered.c_str()) == hipSuccess) {
                    hiprtcDestroyProgram(&prog);
                    g_jit_cache[dk] = fn;
                    return fn;
                }
            }
        }
    }
    if (!may_compile) { *why = "not cached and the stream is too small to repay a plan-time build"; hiprtcDestroyProgram(&prog); return nullptr; }
    hiprtcResult r = hiprtcCompileProgram(prog, (int)optv.size(), optv.data());
    if (r != HIPRTC_SUCCESS) {
        size_t ls = 0; hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, 0); if (ls) hiprtcGetProgramLog(prog, &log[0]);
        *why = "hiprtc: " + log.substr(0, 300);
        g_jit_failed[dk] = *why;
        hiprtcDestroyProgram(&prog);
        return nullptr;
    }
    const char *lowered = nullptr;
    hiprtcGetLoweredName(prog, name, &lowered);
    size_t cs = 0; hiprtcGetCodeSize(prog, &cs);
    std::vector<char> code(cs);
    hiprtcGetCode(prog, code.data());
    if (const char *dump = dev_env("QD_JIT_DUMP")) {          // development: keep the code object for llvm-objdump
        if (FILE *f = fopen(dump, "wb")) { fwrite(code.data(), 1, code.size(), f); fclose(f); }
    }
    hipModule_t mod; hipFunction_t fn = nullptr;
    if (hipModuleLoadData(&mod, code.data()) != hipSuccess || !lowered || hipModuleGetFunction(&fn, mod, lowered) != hipSuccess) {
        *why = "hipModuleLoadData / GetFunction failed";
        hiprtcDestroyProgram(&prog);
        return nullptr;
    }
    if (!cache_file.empty()) {                               // publish atomically: write aside, then rename
        char tmpn[32]; snprintf(tmpn, sizeof tmpn, ".tmp%d", (int)getpid());
        const std::string tmp = cache_file + tmpn;
        if (FILE *f = fopen(tmp.c_str(), "wb")) {
            bool ok = fwrite("QDJIT1\n", 1, 7, f) == 7 && fputs(lowered, f) >= 0 && fputc('\n', f) != EOF &&
                      fwrite(code.data(), 1, code.size(), f) == code.size();
            ok = fclose(f) == 0 && ok;
            if (!ok || rename(tmp.c_str(), cache_file.c_str()) != 0) (void)remove(tmp.c_str());
        }
    }
    hiprtcDestroyProgram(&prog);
    g_jit_cache[dk] = fn;
    return fn;
}

struct Geometry {
    uint32_t G = 1, Dp = 1, lds_raw_elems = 0;
    size_t lds_bytes = 0;        // dynamic LDS that fits the main kernel AND the generic kernels (the unaligned-tail launch)
    size_t lds_main = 0;         // the main kernel's own need when it is smaller (half-window tiles): its launch size, and what bounds workgroups per CU
};

// Dynamic LDS of a chain kernel with this tiling: its family's layout (qd_geometry.h) plus the historical slack, and the generic
// kernels' layout, which runs inside the same allocation for the unaligned slab tail — the larger of the two.
size_t lds_for(uint32_t G, uint64_t W, uint64_t S, uint64_t D, uint64_t T, uint32_t *raw_elems, uint32_t pad_per_row = 1, uint32_t batch = 1,
               bool lut8 = true, uint32_t flags = 0, size_t *main_only = nullptr, int stream_spl = 2 /* samples per lane and row load (streaming kernel) */,
               int stream_nt = 512 /* its producer threads */) {
    const FixedRules g = fixed_rules(W, S, D, T, G, 8, 1, pad_per_row, batch, flags);
    // *raw_elems is what the runtime-geometry kernels read (ChainParams::lds_raw_elems): THEIR raw tile, whatever the main kernel's
    if (raw_elems) *raw_elems = (uint32_t)generic_raw_elems(g);
    uint64_t main_b = 0;
    // (a wave-local plan sizes the generic chain kernels here, its own LDS is spark_lds_bytes)
    switch (family_of(flags & ~kGeoSpark)) {
    case kFamPipe3s: {
        const Pipe3sRules k = pipe3s_rules((uint64_t)stream_spl, (uint64_t)stream_nt, g);
        main_b = k.kLdsBytes + (k.kWrite ? kStreamWriteLdsSlack : kStreamLdsSlack - k.FBX_ALIGN * 8);
        break;
    }
    case kFamPipe3: main_b = pipe3_lds_bytes(g) + kPipe3LdsSlack; break;
    default: main_b = chain_lds_bytes(g, lut8); break;
    }
    if (main_only) *main_only = (size_t)main_b;       // what the MAIN kernel needs (half-window tiles: well under the generic kernels' full tile)
    return (size_t)std::max(main_b, generic_lds_bytes(g, lut8));
}

constexpr size_t kLdsMax = 160 * 1024;

}  // namespace

// ------------------------------------------------------------------ plan

// One NCO row table (device): RowBase of the rows [row0, row0 + rows) of `row_len` samples.  A table is only ever
// rewritten (k_rowtab into the same buffer) or regrown after the stream that last read it has drained.
struct RowTab {
    RowBase *d = nullptr;
    uint64_t cap = 0, row0 = 0, rows = 0, off = 0;
    double ratio = 0.0;                      // the NCO ratio the rows were made for
};
// tables one launch context needs: the main kernel's rows and, for plans whose main kernel is not 256 threads wide,
// rows laid out for the 256-thread per-sample kernel that takes the windows at an unaligned slab end
struct NcoTabs {
    RowTab main, tail;
    std::vector<RowTab> phase;               // interleaved launches with a shift: one row grid per launch (offset phi S)
    unsigned long long *work = nullptr;      // the launch context's tile-queue counters (ChainParams::work), zero between launches
    void *cmp_tmp = nullptr;                 // two-stage plans: the carrier of the decimated samples stage A writes and stage B reads
    size_t cmp_tmp_bytes = 0;
    // One launch context = one set of tile-queue counters, row tables and carrier, so launches that use it are ORDERED even when
    // they come on different streams: launch_windows waits for the context's previous launch first (hipStreamWaitEvent, device
    // side) and records `done` behind every launch, the failed ones included.  Two kernels of one context therefore never claim
    // tiles from the same counters at the same time, and `done` transitively covers every earlier reader of its buffers.
    hipEvent_t done = nullptr;
    bool launched = false;
};

struct qd_plan {
    qd_chain_desc d{};
    qd_plan_options opt{};
    int device = 0;
    bool has_shift = false, has_fir = false;
    uint32_t W = 0, logW = 0, S = 0, D = 1, T = 0;
    uint32_t blk_len = 0, blk_subs = 1;     // QD_EPI_CF32_BLOCKS: read_at block length and sub-windows per block
    uint32_t tile_extra = 0;                // ... and extra raw samples per tile (see ChainParams)
    uint64_t dec_len = 0, n_windows = 0, out_rate = 0;
    double ratio = 0.0;
    std::vector<float> taps_h;
    float *taps_d = nullptr;
    FftLayout fft;
    float2 *tw_d = nullptr;
    Geometry geo;
    chain_fn fn = nullptr, fn_unaligned = nullptr;
    const FixedEntry *fixed = nullptr;
    bool spark = false;                  // the wave-local kernel of chains without a lowpass (k_spark) is this plan's main kernel
    uint32_t spark_ts = 0;               // ... its tile: samples per wave (512, 1024 or 2048)
    uint32_t spark_R = 0;                // ... overlapping windows as W / S interleaved launches of side-by-side windows (stride divides width); <= 1: one launch
    uint32_t phase_unit = 1;             // ... window ranges that start on multiples of it start on a load vector
    hipFunction_t jit_fn = nullptr;      // plan-time specialised kernel (hiprtc), replaces fn for aligned launches
    int wg_per_cu = 1, n_cu = 256, prefetch_mode = 2, nco = 0, nt = kThreads;      // nt: threads that share a row of phase 1 (row = nt * SPL samples)
    int launch_nt = kThreads;            // workgroup size of the main kernel: nt, plus the consumer waves of the three-stage kernels
    uint32_t kflags = 0;                 // FixedGeo FLAGS_ of the main kernel
    uint32_t dbg = 0;                    // development builds: ablation bits, read once at plan creation
    // NCO tables: lane tables per plan, row tables per launch context (device path; one per slot of the host ring)
    LaneEntry *jtab_d = nullptr, *jtab256_d = nullptr;
    NcoTabs tabs_dev, tabs_slot[2];
    // take_fft mode (generic kernels): per-window start offsets and an f32 window, both on the device
    const uint64_t *row_offsets_d = nullptr;
    const float *window_d = nullptr;
    float *win_own_d = nullptr;               // qd_chain_desc.windowing == 1: the plan's own copy of blackman_harris(width); window_d points at it
    // QD_EPI_ROWS_F32 (qd_plan_take_fft): blk_len is the row width W (any), W / S the row-mode kernel's power-of-two width and LDS pitch
    bool rows = false, rows_blue = false;     // rows_blue: W is not a power of two (k_bluestein; behind a lowpass over the rows' read_at blocks)
    RowTab rows_tab512;                       // k_bluestein's loader behind a shift: NCO rows of 512 samples
    // timing
    bool timing = false, ev_made = false, ev_recorded = false;
    hipEvent_t ev0{}, ev1{};
    // host streaming
    void *pin_in[2] = {nullptr, nullptr}, *pin_out[2] = {nullptr, nullptr};
    void *dev_in[2] = {nullptr, nullptr}, *dev_out[2] = {nullptr, nullptr};
    size_t stage_in_bytes = 0, stage_out_bytes = 0, pin_in_bytes = 0, pin_out_bytes = 0;
    hipStream_t streams[2] = {nullptr, nullptr};
    qd_plan_stats stats{};
    // composite plans (a window whose FIR input W*D + T exceeds the 160 KiB LDS tile, stride == width): stage A filters and decimates the
    // stream in read_at blocks of W outputs (the write sink's kernels: per-block truncation == the sink's per-window truncation,
    // src/filter.rs:68-83), stage B transforms the W-point windows of that decimated stream; the launch context's `cmp_tmp` carries it
    qd_plan *cmp_a = nullptr, *cmp_b = nullptr;
    // cascade plans (qd_plan_create_stages, qd_cascade.h): [shift] lowpass [shift] [lowpass [shift]].  W, S, n_windows, ratio are the
    // sink's; D = D1 D2 and T = T2 D1 + T1 are the EFFECTIVE source step and span, so that W D + T / S D (src_range, shards, host chunks)
    // are the source figures of a window
    bool casc = false;
    uint32_t c_D1 = 1, c_T1 = 0, c_D2 = 1, c_T2 = 0, c_n2 = 0, c_M = 0, c_flags = 0, c_inter = 0, c_src = 0;
    double c_ratio[3] = {0, 0, 0};
    uint64_t c_complete = 0;              // leading windows whose read_exact_at succeeds (qd_plan_complete_windows)
    size_t c_lds = 0;
    int c_wg_per_cu = 1;
    float *c_h1 = nullptr, *c_h2 = nullptr;
    LaneEntry *c_jtab = nullptr;
    // the stage list the plan was made from (qd_plan_create_stages; routed plans too) and each lowpass stage's taps
    std::vector<qd_stage> stages;
    std::vector<std::vector<float>> stage_taps;
    // sharded plans (options.n_shards > 1): one child plan per shard, created on that shard's device
    std::vector<qd_plan *> shards;
    std::vector<qd_shard_info> shard_info;
    std::mutex mu;
};
// the kernel a committed chain plan launches: its flags' family where a shape-specialised kernel won, the runtime-geometry k_chain otherwise
// (the flag bits of k_spark2 and k_spark0 — 20, 21 — only ever come from plan-time builds: no table entry carries them)
static Family plan_family(const qd_plan *p) { return (p->jit_fn || p->fixed || p->spark) ? family_of(p->kflags) : kFamChain; }
// ... and whether that kernel wants its launches on the row grid
static bool plan_on_rows(const qd_plan *p) { return (p->jit_fn || p->fixed || p->spark) && row_aligned(p->kflags); }

namespace {

uint64_t out_bytes_per_window(const qd_plan *p) {
    switch (p->d.epilogue) {
    case QD_EPI_NORMS_F32: return (uint64_t)p->W * 4;
    case QD_EPI_GLYPH_U8: return p->W;
    case QD_EPI_CF32_BLOCKS: return (uint64_t)p->blk_len * 8;
    case QD_EPI_ROWS_F32: return (uint64_t)p->blk_len * 4;
    default: return 1;
    }
}

// take_fft's slice rules against the viewed stream's len() (src/ffts.rs:27-48), shared by qd_take_fft, qd_rows_geometry and qd_plan_take_fft
int rows_slice(uint64_t len, uint64_t W, int has_slice, uint64_t *start, uint64_t *end, uint64_t output_len) {
    if (!has_slice) {                                                             // src/ffts.rs:27-30
        if (len < W) return fail(QD_ERR_PANIC, "len < width underflows (src/ffts.rs:29)");
        *start = 0; *end = len - W;
    }
    if (!(*end > *start)) return fail(QD_ERR_PANIC, "Invalid slice: end (%llu) must be greater than start (%llu)", (unsigned long long)*end, (unsigned long long)*start);
    if (!(*end < len)) return fail(QD_ERR_PANIC, "Slice end (%llu) exceeds sample length (%llu)", (unsigned long long)*end, (unsigned long long)len);
    const uint64_t visible = *end - *start;
    if (!(visible > output_len)) return fail(QD_ERR_INVALID, "Visible samples (%llu) must be greater than output length (%llu)", (unsigned long long)visible, (unsigned long long)output_len);
    return QD_OK;
}
// row i's offset exactly as the reference forms it (f64 step, round half away from zero, saturating cast; src/ffts.rs:50,60)
uint64_t rows_offset(uint64_t start, uint64_t end, uint64_t output_len, uint64_t i) {
    const double step = (double)(end - start) / (double)output_len;
    const double r = std::round(step * (double)i);
    const uint64_t ri = !(r > 0) ? 0 : (r >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)r);
    return start + ri;
}
// generate_blackman_harris_window, src/ffts.rs:110-119 (host f32 arithmetic like the reference)
void blackman_harris(size_t W, std::vector<float> *win) {
    win->resize(W);
    const float tau = 6.28318530717958647692528676655900577f;
    for (size_t i = 0; i < W; ++i) {
        float x = tau * (float)i / (float)(W - 1);
        (*win)[i] = 0.35875f - 0.48829f * std::cos(x) + 0.14128f * std::cos(2.0f * x) - 0.01168f * std::cos(3.0f * x);
    }
}

// the sink's windows over a stream of `len` samples: the reference's loop count (src/fft.rs:28,65; the bucket sink's :86)
uint64_t sink_windows(int epilogue, uint64_t len, uint64_t W, uint64_t S) {
    const uint64_t lim = len >= W ? len - W : 0;
    return epilogue == QD_EPI_BUCKET2_U8 ? lim / S : (lim == 0 ? 0 : (lim - 1) / S + 1);
}

// the only place plan options are checked and defaulted
int check_options(const qd_plan_options *options, qd_plan_options *out) {
    qd_plan_options opt{};
    opt.struct_size = sizeof opt;
    if (options) {
        if (options->struct_size != sizeof(qd_plan_options)) return fail(QD_ERR_INVALID, "qd_plan_options size mismatch");
        opt = *options;
        if (opt.kernel_policy < QD_KERNEL_AUTO || opt.kernel_policy > QD_KERNEL_NO_PLAN_TIME) return fail(QD_ERR_INVALID, "unknown kernel_policy %d", opt.kernel_policy);
        if (opt.nco_order < 0 || opt.nco_order > 2) return fail(QD_ERR_INVALID, "nco_order must be 0, 1 or 2");
        if (opt.copy_threads > 64) return fail(QD_ERR_INVALID, "copy_threads > 64");
        if (opt.chunk_bytes && (opt.chunk_bytes < (1u << 16) || opt.chunk_bytes > (1ull << 34))) return fail(QD_ERR_INVALID, "chunk_bytes outside [64 KiB, 16 GiB]");
        if (opt.n_shards > QD_MAX_SHARDS) return fail(QD_ERR_INVALID, "n_shards > %d", QD_MAX_SHARDS);
    }
    *out = opt;
    return QD_OK;
}

// the sink's fields of a chain description (the stages are checked by stages_geo)
int check_sink(const qd_chain_desc &d) {
    if (d.format < 0 || d.format > 3) return fail(QD_ERR_INVALID, "unknown format %d", d.format);
    if (d.epilogue < 0 || d.epilogue > QD_EPI_ROWS_F32) return fail(QD_ERR_INVALID, "unknown epilogue %d", d.epilogue);
    if (d.mode != QD_MODE_EXACT && d.mode != QD_MODE_FAST) return fail(QD_ERR_INVALID, "unknown mode %d", d.mode);
    if (d.epilogue == QD_EPI_ROWS_F32) {               // take_fft: FftPlanner takes any length (src/ffts.rs:25); stride and range are ignored
        if (d.width < 1 || d.width > (1u << 20)) return fail(QD_ERR_UNSUPPORTED, "take_fft width %llu", (unsigned long long)d.width);
        return QD_OK;
    }
    if (!is_pow2(d.width))
        return fail(QD_ERR_PANIC, "Radix4 requires a power-of-two width (rustfft API contract), got %llu", (unsigned long long)d.width);
    if (d.width > (1u << 20)) return fail(QD_ERR_UNSUPPORTED, "width too large");
    if (d.stride == 0) return fail(QD_ERR_INVALID, "stride 0 never terminates in the reference (src/fft.rs:65)");
    if (d.stride > 0xffffffffull) return fail(QD_ERR_UNSUPPORTED, "stride too large");
    return QD_OK;
}

// One NCO row table: rows of ROW samples at `ratio` (on the grid offset by n_off samples) covering samples [n_lo, n_hi).
int ensure_rowtab(RowTab *t, double ratio, uint32_t ROW, uint64_t n_lo, uint64_t n_hi, hipStream_t st, uint64_t n_off = 0) {
    const uint64_t r_lo = n_lo / ROW, r_hi = (n_hi + ROW - 1) / ROW;
    if (t->d && t->off == n_off && t->ratio == ratio && r_lo >= t->row0 && r_hi <= t->row0 + t->rows) return QD_OK;
    // The table is about to be rewritten: whatever read it last must have finished.  launch_windows has already ordered `st` behind
    // the context's previous launch (NcoTabs::done — an event, not the earlier caller's stream handle, which may be destroyed by
    // now), so k_rowtab on `st` runs after every earlier reader.
    const uint64_t rows = r_hi - r_lo;
    if (rows > t->cap) {
        if (t->d) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(t->d)); t->d = nullptr; t->cap = 0; }
        const uint64_t cap = rows + rows / 8 + 16;            // chunks of a run differ by a row or two: grow once
        HIPCHK(hipMalloc(&t->d, cap * sizeof(RowBase)));
        t->cap = cap;
    }
    t->row0 = r_lo; t->rows = rows; t->off = n_off; t->ratio = ratio;
    hipLaunchKernelGGL(k_rowtab, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, st, ratio, ROW, r_lo, rows, n_off, t->d);
    HIPCHK(hipGetLastError());
    return QD_OK;
}

// the chain kernels' tables: the plan's ratio, and a row beyond the last sample's
int ensure_rowtab_for(qd_plan *p, uint32_t ROW, RowTab *t, uint64_t n_lo, uint64_t n_hi, hipStream_t st, uint64_t n_off = 0) {
    return ensure_rowtab(t, p->ratio, ROW, n_lo, n_hi + ROW, st, n_off);
}

int ensure_work(NcoTabs *tabs) {
    if (tabs->work) return QD_OK;
    HIPCHK(hipMalloc(&tabs->work, 9 * 16 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(tabs->work, 0, 9 * 16 * sizeof(unsigned long long)));       // the kernel leaves them zero again
    return QD_OK;
}

void free_rowtab(RowTab *t) {
    if (t->d) (void)hipFree(t->d);
    *t = RowTab{};
}

// What a chain kernel's parameters take from the PLAN (geometry, constants, device tables); the caller adds the call's slab, window range,
// output and row table.
void plan_params(const qd_plan *p, ChainParams *Pp) {
    ChainParams &P = *Pp;
    P.W = p->W; P.logW = p->logW; P.S = p->S; P.D = p->D; P.T = p->T;
    const uint32_t c = p->T - p->T / 2;
    P.G = p->geo.G; P.Dp = p->geo.Dp;
    P.dmagic = p->D > 1 ? (uint32_t)((1ull << 32) / p->D + 1) : 0;
    P.dshift = is_pow2(p->D) ? ilog2(p->D) : 0xffffffffu;
    P.a0 = c / p->D; P.b0 = c % p->D;
    uint32_t tfast = p->D + p->T / 2;
    P.T_fast = tfast < p->T ? tfast : p->T;
    P.a1 = (c + P.T_fast) / p->D; P.b1 = (c + P.T_fast) % p->D;
    P.base_len = p->fft.base_len; P.log_base = p->fft.log_base; P.layers = p->fft.layers;
    P.epi = (uint32_t)p->d.epilogue;
    P.lds_raw_elems = p->geo.lds_raw_elems;
    P.rmin = p->d.has_range ? p->d.range_min : 0.08f;     // src/fft.rs:22-23
    P.rmax = p->d.has_range ? p->d.range_max : 1.0f;
    P.gstep = (P.rmax - P.rmin) / 7.0f;                   // src/fft.rs:45, f32 like the reference
    P.rgstep = 1.0f / P.gstep;                            // glyph_code's short form (qd_device.h)
    P.root2 = (float)std::sqrt(0.5);
    P.tw16_1 = compute_twiddle(1, 16); P.tw16_2 = compute_twiddle(2, 16); P.tw16_3 = compute_twiddle(3, 16);
    P.ratio = p->ratio;
    P.jtab = p->jtab_d; P.taps = p->taps_d; P.tw = p->tw_d;
    P.row_offsets = p->row_offsets_d; P.window = p->window_d;
    P.blk_len = p->blk_len ? p->blk_len : p->W; P.blk_sub_mask = p->blk_subs - 1;
    P.tile_extra = p->tile_extra;
    P.dbg = p->dbg;                                       // 0 except in development builds (QD_DEBUG_SKIP at plan creation)
}

// Overlapping windows without a lowpass or a shift, stride S dividing the width (qd_plan::spark_R = W / S): launch phi covers the windows
// w = phi (mod R) of the range — side by side in the stream that starts phi * S samples later — and writes every R-th output row.
// (Running the R launches over one 8 ... 128 MiB stretch of the stream after the other, so that the re-reads hit the memory-side cache,
// was measured and is slower at every size: profiles/r04/phase_chunk.log.)
int launch_spark_phases(qd_plan *p, NcoTabs *tabs, const void *src_d, uint64_t src_first, uint64_t src_count, uint64_t first_window,
                        uint64_t n_windows, uint64_t out_window0, void *out_d, hipStream_t st) {
    const int bps = bps_of(p->d.format);
    const uint64_t R = p->spark_R, W = p->W, S = p->S, obw = out_bytes_per_window(p);
    ChainParams P{};
    plan_params(p, &P);
    P.S = p->W;                                 // each launch's own geometry: windows side by side
    P.lds_dyn = (uint32_t)p->geo.lds_main;
    P.out_row_stride = (uint32_t)R;
    const uint64_t cap = (uint64_t)p->n_cu * p->wg_per_cu, last = first_window + n_windows - 1;
    for (uint64_t phi = 0; phi < R; ++phi) {
        if (last < phi) break;
        const uint64_t k_lo = first_window > phi ? (first_window - phi + R - 1) / R : 0, k_hi = (last - phi) / R;
        if (k_hi < k_lo) continue;
        const uint64_t n_phi = k_hi - k_lo + 1, shift_samples = phi * S;
        if (k_lo * W + shift_samples < src_first || (k_hi * W + shift_samples + W) > src_first + src_count)
            return fail(QD_ERR_INVALID, "src slab [%llu,+%llu) does not cover the samples of windows [%llu,+%llu)", (unsigned long long)src_first,
                        (unsigned long long)src_count, (unsigned long long)first_window, (unsigned long long)n_windows);
        P.src = static_cast<const uint8_t *>(src_d) + shift_samples * bps;      // sample n of this launch is sample n + phi S of the stream
        P.src_first = src_first; P.src_count = src_count - shift_samples;
        if (p->has_shift) {
            // the NCO row grid of THIS launch's stream: rows of 512 samples that start phi S samples into the plan's (the caller has checked
            // that the launch's first window sits on it); the lane table does not depend on where a row starts
            if (tabs->phase.size() < R) tabs->phase.resize(R);
            const int rc = ensure_rowtab_for(p, kSparkRow, &tabs->phase[phi], k_lo * W, (k_hi + 1) * W + (uint64_t)P.G * W, st, shift_samples);
            if (rc) return rc;
            P.rowtab = tabs->phase[phi].d; P.rowtab_row0 = tabs->phase[phi].row0;
        }
        P.first_window = k_lo; P.n_windows = n_phi; P.out_window0 = k_lo;
        P.out = static_cast<uint8_t *>(out_d) + ((k_lo * R + phi) - out_window0) * obw;
        const uint64_t n_tiles = (n_phi + P.G - 1) / P.G, wgs = (n_tiles + 3) / 4;
        const uint32_t grid = (uint32_t)(wgs < cap ? wgs : cap);
        void *args[] = {&P};
        HIPCHK(hipModuleLaunchKernel(p->jit_fn, grid, 1, 1, (unsigned)p->launch_nt, 1, 1, (unsigned)p->geo.lds_main, st, args, nullptr));
    }
    return QD_OK;
}

// windows [first_window, +n_windows) of a cascade plan (qd_cascade.h); the caller has clipped them to the complete windows
// (the write sink's kernel windows are sub-blocks: the source, inter and outer ranges are those of the read_at blocks they lie in)
int launch_cascade(qd_plan *p, NcoTabs *tabs, const void *src_d, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                   uint64_t out_window0, void *out_d, hipStream_t st) {
    const uint64_t last = first_window + n_windows - 1, l2 = (p->c_flags & kCascL2) ? p->c_D2 : 1;
    // windows [w_lo, w_hi] of the sink (blocks of the write sink), each window_len outer outputs, step apart
    const uint64_t subs = p->blk_subs, w_lo = first_window / subs, w_hi = last / subs;
    const uint64_t step = p->blk_len ? p->blk_len : p->S, window_len = p->blk_len ? p->blk_len : p->W;
    const uint64_t need0 = w_lo * step * p->D, need1 = w_hi * step * p->D + window_len * p->D + p->T;
    if (need0 < src_first || need1 > src_first + src_count)
        return fail(QD_ERR_INVALID, "src slab [%llu,+%llu) does not cover samples [%llu,%llu) needed by windows [%llu,+%llu)",
                    (unsigned long long)src_first, (unsigned long long)src_count, (unsigned long long)need0,
                    (unsigned long long)need1, (unsigned long long)first_window, (unsigned long long)n_windows);
    CascadeParams P{};
    plan_params(p, &P.c);
    P.c.src = static_cast<const uint8_t *>(src_d);
    P.c.src_first = src_first; P.c.src_count = src_count;
    P.c.first_window = first_window; P.c.n_windows = n_windows; P.c.out_window0 = out_window0;
    P.c.out = out_d;
    P.h1 = p->c_h1; P.h2 = p->c_h2 ? p->c_h2 : p->c_h1; P.jtab = p->c_jtab;
    P.ratio0 = p->c_ratio[0]; P.ratio1 = p->c_ratio[1]; P.ratio2 = p->c_ratio[2];
    P.S = p->S;
    P.D1 = p->c_D1; P.T1 = p->c_T1; P.D2 = p->c_D2; P.T2 = p->c_T2;
    P.n2 = p->c_n2; P.M = p->c_M; P.inter_elems = p->c_inter; P.src_elems = p->c_src;
    P.dmagic1 = p->c_D1 % 2 == 0 ? (uint32_t)((1ull << 32) / p->c_D1 + 1) : 0u;
    P.dmagic2 = (p->c_flags & kCascL2) && p->c_D2 % 2 == 0 ? (uint32_t)((1ull << 32) / p->c_D2 + 1) : 0u;
    P.phi2 = (p->c_flags & kCascL2) ? (p->c_D2 - (p->c_T2 - p->c_T2 / 2) % p->c_D2) % p->c_D2 : 0u;
    P.flags = p->c_flags;
    // row tables of the NCOs over this launch's range, on `st` (ordered behind the context's previous launch, see NcoTabs)
    if (tabs->phase.size() < 3) tabs->phase.resize(3);
    const uint64_t lo[3] = {need0, w_lo * step * l2, w_lo * step}, hi[3] = {need1, w_hi * step * l2 + p->c_n2, w_hi * step + window_len};
    const uint32_t sflag[3] = {kCascS0, kCascS1, kCascS2};
    for (int k = 0; k < 3; ++k) {
        if (!(p->c_flags & sflag[k])) continue;
        const int rc = ensure_rowtab(&tabs->phase[k], p->c_ratio[k], kCascadeRow, lo[k], hi[k], st);      // rows of its own stage's index
        if (rc) return rc;
        P.rows[k] = tabs->phase[k].d; P.row0[k] = tabs->phase[k].row0;
    }
    const uint64_t cap = (uint64_t)p->n_cu * p->c_wg_per_cu;
    const uint32_t grid = (uint32_t)(n_windows < cap ? n_windows : cap);
    if (p->blk_len) {
        switch (p->d.format) {
        case QD_FMT_CF32: hipLaunchKernelGGL(k_cascade_write<0>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        case QD_FMT_CS8: hipLaunchKernelGGL(k_cascade_write<1>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        case QD_FMT_CU8: hipLaunchKernelGGL(k_cascade_write<2>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        default: hipLaunchKernelGGL(k_cascade_write<3>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        }
    } else {
        switch (p->d.format) {
        case QD_FMT_CF32: hipLaunchKernelGGL(k_cascade<0>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        case QD_FMT_CS8: hipLaunchKernelGGL(k_cascade<1>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        case QD_FMT_CU8: hipLaunchKernelGGL(k_cascade<2>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        default: hipLaunchKernelGGL(k_cascade<3>, dim3(grid), dim3(kCascadeThreads), p->c_lds, st, P); break;
        }
    }
    HIPCHK(hipGetLastError());
    return QD_OK;
}

int launch_chain(qd_plan *p, NcoTabs *tabs, const void *src_d, uint64_t src_first, uint64_t src_count, uint64_t first_window,
                 uint64_t n_windows, uint64_t out_window0, void *out_d, hipStream_t st) {
    const int fmt = p->d.format;
    const int spl = spl_of(fmt), bps = bps_of(fmt);
    uint64_t need0 = first_window * p->S * p->D;
    uint64_t need1 = (first_window + n_windows - 1) * p->S * p->D + (uint64_t)p->W * p->D + p->T;
    if (!p->row_offsets_d && (need0 < src_first || need1 > src_first + src_count))
        return fail(QD_ERR_INVALID, "src slab [%llu,+%llu) does not cover samples [%llu,%llu) needed by windows [%llu,+%llu)",
                    (unsigned long long)src_first, (unsigned long long)src_count, (unsigned long long)need0,
                    (unsigned long long)need1, (unsigned long long)first_window, (unsigned long long)n_windows);
    int rc = QD_OK;
    bool phases_unaligned = false;
    if (p->spark_R > 1) {
        // interleaved launches of side-by-side windows; a slab that does not start on a load vector goes to the per-sample kernel as ever
        // (with a shift every launch's first window must sit on its NCO row grid: first_window a multiple of R * 512 / W)
        const uint64_t row_w = p->W < kSparkRow ? kSparkRow / p->W : 1;
        if (p->jit_fn && !p->row_offsets_d && (reinterpret_cast<uintptr_t>(src_d) % (spl * bps)) == 0 && (src_first % spl) == 0 &&
            (!p->has_shift || first_window % ((uint64_t)p->spark_R * row_w) == 0))
            return launch_spark_phases(p, tabs, src_d, src_first, src_count, first_window, n_windows, out_window0, out_d, st);
        phases_unaligned = true;
    }
    if (p->has_shift) {
        // row-aligned phase 1: rows of a short last tile's missing windows (and a half-window pass's read-ahead) get table entries too
        // (the streaming kernel parks one more step of rows behind a run's last tile)
        const uint64_t extra = plan_on_rows(p) ? (uint64_t)p->geo.G * p->S * p->D * (plan_family(p) == kFamPipe3s ? 2 : 1) + p->T : 0;
        rc = ensure_rowtab_for(p, p->nt * spl_of(fmt), &tabs->main, need0, need1 + extra, st);
        if (rc) return rc;
    }

    ChainParams P{};
    plan_params(p, &P);
    P.src = static_cast<const uint8_t *>(src_d);
    P.src_first = src_first; P.src_count = src_count;
    P.out_window0 = out_window0;
    P.rowtab = tabs->main.d; P.rowtab_row0 = tabs->main.row0;
    P.out = out_d;
#if defined(QD_STAMP) || defined(QD_WGTIME)
    constexpr size_t kStampWords = 256 + 4 * 4096;
    static unsigned long long *stamps_d = nullptr;
    if (!stamps_d) { HIPCHK(hipMalloc(&stamps_d, kStampWords * 8)); }
    HIPCHK(hipMemsetAsync(stamps_d, 0, kStampWords * 8, st));
    P.stamps = stamps_d;
#endif

    // The aligned kernels issue whole-vector loads: the slab must start on a vector boundary and a
    // window whose last vector would straddle the slab end goes to the per-sample kernel instead.
    const int vec_bytes = spl * bps;
    const bool vec_ok = (reinterpret_cast<uintptr_t>(src_d) % vec_bytes) == 0 && (src_first % spl) == 0 &&
                        src_count * (uint64_t)bps >= (uint64_t)vec_bytes;
    uint64_t n_aligned = 0;
    // row-aligned phase 1 with G S D (not S D) a multiple of the row: the launch's first window must sit on a row boundary too
    bool fast_misaligned = plan_on_rows(p) && ((first_window * p->S * p->D) % ((uint64_t)p->nt * spl)) != 0;
    // the wave-local kernel: tiles start on NCO rows when the chain shifts, on load vectors otherwise; irregular rows (take_fft) never run on it
    if (p->spark) fast_misaligned = phases_unaligned || p->row_offsets_d != nullptr || ((first_window * p->S) % (p->has_shift ? (uint64_t)kSparkRow : (uint64_t)spl)) != 0;
    if (plan_family(p) == kFamSpark0) fast_misaligned = p->row_offsets_d != nullptr;      // a window per lane: any window start (S BPS is a multiple of 4)
    if (vec_ok && !fast_misaligned) {
        // windows [first_window, first_window + n_aligned): need-end rounded up to a vector fits in the slab
        const uint64_t step = (uint64_t)p->S * p->D, rpw = (uint64_t)p->W * p->D + p->T;
        const uint64_t usable = (src_count / spl) * spl + src_first;     // end of the last whole vector
        n_aligned = n_windows;
        while (n_aligned > 0 && (first_window + n_aligned - 1) * step + rpw > usable) --n_aligned;
        // The fast phase 1 (FixedGeo FLAGS_ bit 3) loads and parks a compile-time number of rows per tile, whatever the tile's
        // window count: a short LAST tile (n_windows not a multiple of G) costs it a few rows nobody reads — the buffer
        // descriptor's range check covers the slab end, the row table is extended below — instead of a second launch of the
        // per-sample kernel for one window (cfg2: 65 535 windows in tiles of two; ~8 us of a 0.21 ms step).
    }
    const bool tail_tables = n_aligned < n_windows && p->nt != kThreads && p->has_shift;
    if (tail_tables) {
        const uint64_t t0 = (first_window + n_aligned) * p->S * p->D;
        rc = ensure_rowtab_for(p, kThreads * spl, &tabs->tail, t0, need1, st);
        if (rc) return rc;
    }
    const uint64_t cap = (uint64_t)p->n_cu * p->wg_per_cu;
    for (int part = 0; part < 2; ++part) {
        const uint64_t w_begin = part == 0 ? first_window : first_window + n_aligned;
        const uint64_t w_count = part == 0 ? n_aligned : n_windows - n_aligned;
        if (w_count == 0) continue;
        P.first_window = w_begin; P.n_windows = w_count;
        if (part == 1 && tail_tables) { P.rowtab = tabs->tail.d; P.rowtab_row0 = tabs->tail.row0; P.jtab = p->jtab256_d; }
        const uint64_t n_tiles = (w_count + P.G - 1) / P.G;
        uint32_t grid = (uint32_t)(n_tiles < cap ? n_tiles : cap);
        if (part == 0 && p->spark) { const uint64_t wgs = (n_tiles + 3) / 4; grid = (uint32_t)(wgs < cap ? wgs : cap); }      // a tile per WAVE, four waves per workgroup
        // dynamic tile queue for the main launch (static strided walk for the short unaligned tail and for tiny grids)
        P.work = nullptr;
        if (part == 0 && !p->spark && (grid & 7u) == 0 && n_tiles >= 4ull * grid) { rc = ensure_work(tabs); if (rc) return rc; P.work = tabs->work; }
        P.lds_dyn = (uint32_t)(part == 0 && p->geo.lds_main ? p->geo.lds_main : p->geo.lds_bytes);
        if (part == 0 && p->jit_fn && !p->row_offsets_d) {
            void *args[] = {&P};
            HIPCHK(hipModuleLaunchKernel(p->jit_fn, grid, 1, 1, (unsigned)p->launch_nt, 1, 1, (unsigned)(p->geo.lds_main ? p->geo.lds_main : p->geo.lds_bytes), st, args, nullptr));
        } else {
            hipLaunchKernelGGL(part == 0 ? p->fn : p->fn_unaligned, dim3(grid), dim3(part == 0 ? p->launch_nt : kThreads), part == 0 && p->geo.lds_main ? p->geo.lds_main : p->geo.lds_bytes, st, P);
            HIPCHK(hipGetLastError());
        }
    }
#ifdef QD_WGTIME
    {
        std::vector<unsigned long long> h(kStampWords);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(h.data(), P.stamps, kStampWords * 8, hipMemcpyDeviceToHost));
        std::vector<double> dur, endt; unsigned long long t_first = ~0ull, t_last = 0; double per_xcc[16] = {0}; int n_xcc[16] = {0};
        for (int b = 0; b < 4096; ++b) { const unsigned long long *w = &h[256 + 4 * b]; if (!w[3]) continue; t_first = std::min(t_first, w[0]); t_last = std::max(t_last, w[1]); }
        for (int b = 0; b < 4096; ++b) {
            const unsigned long long *w = &h[256 + 4 * b]; if (!w[3]) continue;
            dur.push_back((w[1] - w[0]) * 0.01); endt.push_back((w[1] - t_first) * 0.01); per_xcc[w[2] & 15] += (w[1] - t_first) * 0.01; n_xcc[w[2] & 15]++;
        }
        std::sort(dur.begin(), dur.end()); std::sort(endt.begin(), endt.end());
        if (!dur.empty()) {
            fprintf(stderr, "[wgtime] %zu workgroups, kernel span %.1f us; workgroup run time us: min %.1f median %.1f max %.1f; finish time us: min %.1f p10 %.1f median %.1f p90 %.1f max %.1f\n",
                    dur.size(), (t_last - t_first) * 0.01, dur.front(), dur[dur.size() / 2], dur.back(), endt.front(), endt[endt.size() / 10], endt[endt.size() / 2], endt[endt.size() * 9 / 10], endt.back());
            fprintf(stderr, "[wgtime] mean finish time per XCD:");
            for (int x = 0; x < 16; ++x) if (n_xcc[x]) fprintf(stderr, " xcc%d(%d wgs)=%.1f", x, n_xcc[x], per_xcc[x] / n_xcc[x]);
            fprintf(stderr, "\n");
        }
    }
#endif
#ifdef QD_STAMP
    {
        unsigned long long h[160];
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(h, P.stamps, sizeof h, hipMemcpyDeviceToHost));
        static const char *names[8] = {"phase1", "bar1", "fir", "bar2", "fft", "bar3", "epilogue", "bar4"};
        double tiles = (double)h[128];
        unsigned grid_wgs = (unsigned)(((n_windows + P.G - 1) / P.G) < cap ? ((n_windows + P.G - 1) / P.G) : cap);
        fprintf(stderr, "[stamps] tiles/launch %.0f (wgs %u): cycles per tile per wave:", tiles, grid_wgs);
        for (int w = 0; w < 16; ++w) {
            if (w >= 4 && h[w * 8] == 0) continue;                 // workgroups with fewer waves
            fprintf(stderr, "\n   wave%d:", w);
            double tot = 0;
            for (int k = 0; k < 8; ++k) { fprintf(stderr, " %s=%.0f", names[k], h[w * 8 + k] / tiles); tot += h[w * 8 + k] / tiles; }
            fprintf(stderr, "  total=%.0f", tot);
        }
        fprintf(stderr, "\n   wave1 phase-1 split per tile: wait_data=%.0f issue_prefetch=%.0f wait_rowbase=%.0f process=%.0f\n", h[129] / tiles, h[130] / tiles, h[131] / tiles, h[132] / tiles);
        fprintf(stderr, "   wave0 phase-1 split per tile: wait_data=%.0f issue_prefetch=%.0f wait_rowbase=%.0f process=%.0f\n", h[133] / tiles, h[134] / tiles, h[135] / tiles, h[136] / tiles);
    }
#endif
    return QD_OK;
}

int launch_windows(qd_plan *p, NcoTabs *ctx, const void *src_d, uint64_t src_first, uint64_t src_count, uint64_t first_window,
                   uint64_t n_windows, uint64_t out_window0, void *out_d, hipStream_t st);

// windows [w0, +nw) of a two-stage plan: stage A filters their read_at blocks into the context's carrier, stage B transforms them.
// Each stage runs on its own plan's launch context of the same role (device path or host ring slot) as `ctx`.
int launch_composite(qd_plan *p, NcoTabs *ctx, const void *src_d, uint64_t src_first, uint64_t src_count, uint64_t w0, uint64_t nw,
                     uint64_t out_window0, void *out_d, hipStream_t st) {
    qd_plan *a = p->cmp_a, *b = p->cmp_b;
    const uint64_t W = p->W;
    const size_t need = (size_t)(nw * W + 16) * 8;
    if (need > ctx->cmp_tmp_bytes) {
        if (ctx->cmp_tmp) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(ctx->cmp_tmp)); ctx->cmp_tmp = nullptr; ctx->cmp_tmp_bytes = 0; }
        HIPCHK(hipMalloc(&ctx->cmp_tmp, need));
        ctx->cmp_tmp_bytes = need;
    }
    NcoTabs *ca = &a->tabs_dev, *cb = &b->tabs_dev;
    if (ctx != &p->tabs_dev) { const ptrdiff_t k = ctx - p->tabs_slot; ca = &a->tabs_slot[k]; cb = &b->tabs_slot[k]; }
    const int rc = launch_windows(a, ca, src_d, src_first, src_count, w0 * a->blk_subs, nw * a->blk_subs, w0 * a->blk_subs, ctx->cmp_tmp, st);
    if (rc) return rc;
    return launch_windows(b, cb, ctx->cmp_tmp, w0 * W, nw * W, w0, nw, out_window0, out_d, st);
}

// The one way device-resident windows of any plan are launched: windows [first_window, +n_windows) of a slab holding source samples
// [src_first, +src_count) into out_d, which holds the windows from out_window0 on.  It keeps the launch-context protocol of NcoTabs
// and the plan's timing events for every kind of plan; the kind's body does the rest.
int launch_windows(qd_plan *p, NcoTabs *ctx, const void *src_d, uint64_t src_first, uint64_t src_count, uint64_t first_window,
                   uint64_t n_windows, uint64_t out_window0, void *out_d, hipStream_t st) {
    if (n_windows == 0) return QD_OK;
    if (!ctx->done) HIPCHK(hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming));
    // ALWAYS wait: a stream handle compared with the previous caller's may be a new stream at a recycled address (the old one destroyed
    // with its kernels still running); a wait on an event recorded in the same stream costs nothing
    if (ctx->launched) HIPCHK(hipStreamWaitEvent(st, ctx->done, 0));
    if (p->timing && !p->ev_made) { HIPCHK(hipEventCreate(&p->ev0)); HIPCHK(hipEventCreate(&p->ev1)); p->ev_made = true; }
    if (p->timing) HIPCHK(hipEventRecord(p->ev0, st));
    const int rc = p->cmp_a ? launch_composite(p, ctx, src_d, src_first, src_count, first_window, n_windows, out_window0, out_d, st)
                 : p->casc ? launch_cascade(p, ctx, src_d, src_first, src_count, first_window, n_windows, out_window0, out_d, st)
                 : launch_chain(p, ctx, src_d, src_first, src_count, first_window, n_windows, out_window0, out_d, st);
    // whatever the body enqueued before it returned, an error included, is now behind `done`
    HIPCHK(hipEventRecord(ctx->done, st));
    ctx->launched = true;
    if (p->timing) { HIPCHK(hipEventRecord(p->ev1, st)); p->ev_recorded = true; }
    return rc;
}

void free_streaming(qd_plan *p) {
    for (int i = 0; i < 2; ++i) {
        if (p->pin_in[i]) (void)hipHostFree(p->pin_in[i]);
        if (p->pin_out[i]) (void)hipHostFree(p->pin_out[i]);
        if (p->dev_in[i]) (void)hipFree(p->dev_in[i]);
        if (p->dev_out[i]) (void)hipFree(p->dev_out[i]);
        if (p->streams[i]) (void)hipStreamDestroy(p->streams[i]);
        p->pin_in[i] = p->pin_out[i] = p->dev_in[i] = p->dev_out[i] = nullptr;
        p->streams[i] = nullptr;
    }
    p->stage_in_bytes = p->stage_out_bytes = p->pin_in_bytes = p->pin_out_bytes = 0;
}


// ---- choosing a one-stage chain plan's main kernel.  chain_candidates lists, for the plan's chain class, the ways its kernel can be
// had, best first; plan_init takes the first whose kernel it can have (a plan-time build may not be: not cached and too small a stream
// to compile for, or the build failed — failures are memoised, so the order of the builds is part of the behaviour) and commits it.
struct Candidate {
    enum Source { kTable, kBuiltinSpark, kBuild, kGeneric } src = kGeneric;
    // tiling: windows per tile, threads that share a row of phase 1, LDS pad per row, tiles per FFT batch, FixedGeo FLAGS_, the
    // register budget a build targets (waves per SIMD), scalar accumulate chains (-fno-slp-vectorize), FIR knobs
    uint32_t G = 1; int nt = kThreads; uint32_t pad = 1, batch = 1, flags = 0; int lb = 4, noslp = 0; uint32_t firr = 1, firb = 8;
    // the wave-local kernels of chains without a lowpass (qd_plan::spark_ts / spark_R; the lane table in LDS)
    uint32_t spark_ts = 0, spark_R = 0; bool spark_jt_lds = false;
    const FixedEntry *fixed = nullptr;      // kTable
    JitKey key{};                           // kBuild
    bool required = false;                  // kBuild: failure is an error, not a step down the list (tile hints)
    int wg_regs = 0;                        // workgroups per CU its register budget admits (0: no bound of its own)
};

bool lut8_of(int fmt) { return fmt == QD_FMT_CS8 || fmt == QD_FMT_CU8; }
constexpr uint64_t kWholeRows = 10;      // rows per tile (per step) up to which a build prefetches whole tiles: what every recipe aims for

// the plain tiling: windows per tile of the generic kernels and of the plain plan-time build (256 threads, pad 1, batch 1, flags 0)
uint32_t plain_tiles(const qd_plan *p, uint32_t T_lds) {
    const bool lut8 = lut8_of(p->d.format);
    auto fits = [&](uint32_t g, size_t cap) { return lds_for(g, p->W, p->S, p->D, T_lds, nullptr, 1, 1, lut8) <= cap; };
    uint32_t G = 1;
    while (G < 64 && (uint64_t)G * p->W < 256 && fits(G * 2, 40 * 1024)) G *= 2;
    while (G < 64 && (uint64_t)G * p->W < 1024 && fits(G * 2, 36 * 1024)) G *= 2;
    // chains without a lowpass (every sample is an FFT input), windows of 128 points and more: 2048 samples per tile while four
    // workgroups still share a CU — fewer barriers per sample (16 GiB cf32, profiles/r03/nofir_rate.log: W = 128 7.16 -> 6.74 ms,
    // W = 256 10.50 -> 9.57, cs16 W = 512 10.18 -> 9.07; 4096 samples per tile: 9.04 at W = 128; W = 64 loses with 32 windows: 8.23 -> 9.65)
    if (!p->has_fir && p->S >= p->W && p->W >= 128) while (G < 64 && (uint64_t)G * p->W < 2048 && fits(G * 2, 40 * 1024)) G *= 2;
    if (p->n_windows && G > p->n_windows) { while (G > 1 && G / 2 >= p->n_windows) G /= 2; }
    return G;
}

// the plan-time build of a chain kernel (k_chain and its three-stage forms) with this tiling; `capped`: its register budget
// bounds the workgroups per CU (lb waves per SIMD)
Candidate chain_build(const qd_plan *p, Candidate c, bool capped) {
    const uint64_t spl = spl_of(p->d.format), ROW = (uint64_t)c.nt * spl, step = (uint64_t)p->S * p->D;
    const FixedRules g = fixed_rules(p->W, p->S, p->D, p->T, c.G, c.firb, c.firr, c.pad, c.batch, c.flags);
    const Family fam = family_of(c.flags);
    // a run may start at any window, so a tile starts on a row boundary only if S*D is a multiple of ROW
    const bool tiles_on_rows = step % ROW == 0 || (row_aligned(c.flags) && (c.G * step) % ROW == 0);
    uint64_t rows = g.rows(c.nt, spl) + (tiles_on_rows ? 0 : 1);       // (half-window tiles: rows of ONE pass)
    if (fam == kFamPipe3s) rows = pipe3s_rules(spl, c.nt, g).RN;      // rows per step of the streaming kernel
    // the unrolled FIR's scalar accumulate chains must stay scalar (the three-stage kernel's FIR is the packed asm form)
    const int noslp = c.noslp || ((c.flags & kGeoUnrolledFir) && fam != kFamPipe3 && fam != kFamPipe3s);
    c.src = Candidate::kBuild;
    c.key = JitKey{p->d.format, p->nco, p->has_fir ? 1 : 0, rows <= kWholeRows ? (int)rows : 4, rows <= kWholeRows ? 1 : 0, c.lb, c.nt,
                   p->W, p->S, p->D, p->T, c.G, c.firb, c.firr, noslp, c.pad, c.batch, c.flags};
    c.wg_regs = capped ? std::max(1, c.lb * 4 * 64 / family_threads(c.nt, c.flags)) : 0;
    return c;
}

// ---- kernel variant from GEOMETRY (plan-time builds): the variants of the built-in cfg3' / cfg4 kernels as recipes for a shape
// (profiles/r03/shape_sweep.log).  Which tiling to try is decided here; whether a kernel can run it is asked of
// the kernels' own rules (qd_geometry.h), so the build takes the path asked for.  Returns false for shapes without a recipe.
bool geometry_recipe(const qd_plan *p, uint32_t T_lds, Candidate *r) {
    const uint32_t W = p->W, S = p->S, D = p->D, T = p->T;
    const uint64_t spl = spl_of(p->d.format);
    const bool lut8 = lut8_of(p->d.format);
    r->pad = 2;
    auto rules = [&](uint32_t g, uint32_t flags, uint32_t batch = 1, uint32_t firr = 1, uint32_t firb = 8, uint32_t stride = 0) {
        return fixed_rules(W, stride ? stride : S, D, T, g, firb, firr, 2, batch, flags);
    };
    if (p->d.epilogue == QD_EPI_CF32_BLOCKS) {
        // The `write` sink (N1: shift -> lowpass -> decimated cf32 in read_at blocks): the streaming kernel with producers and FIR waves
        // only — a step is one sub-block of W = min(block, 256) outputs on as many FIR lanes, which store their outputs themselves;
        // truncation is relative to the block (ChainParams::blk_len).
        if (!(is_pow2(W) && W <= 256 && p->blk_len % W == 0 && is_pow2(p->blk_subs))) return false;
        const uint32_t fl = kGeoNoSplit | kGeoNtLoads | kGeoPipe3 | kGeoStream | kGeoWriteSink;
        for (int snt : {512, 256}) {
            const Pipe3sRules k = pipe3s_rules(spl, snt, rules(1, fl));
            if (!k.ok || k.RN > kWholeRows) continue;
            if (lds_for(1, W, S, D, T, nullptr, 2, 1, lut8, fl, nullptr, (int)spl, snt) > kLdsMax ||        // the kernel's own layout (its T, no tile_extra) ...
                lds_for(1, W, S, D, T_lds, nullptr, 1, 1, lut8) > kLdsMax) continue;                        // ... and the generic kernels' tile for an unaligned tail
            r->G = 1; r->nt = snt; r->flags = fl;
            return true;
        }
        return false;
    }
    if (S < W) {
        // Overlapping windows with a long filter (>= 8 taps per input sample): the three-stage kernel (shared FIR on 16-byte rows, at most
        // 256 outputs per tile, tiles on rows of 512 producer threads), streaming where its geometry holds.  cfg5: 7.50 -> 6.71 ms.
        const uint32_t fl3 = kGeoUnrolledFir | kGeoPipe3, fls = fl3 | kGeoStream;
        if ((uint64_t)T < 8ull * D || !rules(1, fl3).kUnrolledShared) return false;
        const uint64_t step = (uint64_t)S * D;
        // (1) the STREAMING form (k_chain_pipe3s): the step of G S new outputs with the most outputs the rings leave room for (the FIR is
        // bound by one wave's pass over the T taps), rows of 512 producer threads or of 256 where that admits a larger step (8-bit
        // formats)
        uint32_t best_s = 0; int best_nt = 512;
        for (int snt : {512, 256}) {
            const uint32_t su = (uint32_t)(snt * spl / ct_gcd(snt * spl, step));      // steps start on rows when G is a multiple of this
            for (uint32_t g = su; g <= 64; g += su) {
                const Pipe3sRules k = pipe3s_rules(spl, snt, rules(g, fls));
                if (!k.ok || k.RN > kWholeRows) continue;
                if (lds_for(g, W, S, D, T_lds, nullptr, 2, 1, lut8, fls, nullptr, (int)spl, snt) > kLdsMax) break;
                if (p->n_windows < g) break;
                if (g > best_s) { best_s = g; best_nt = snt; }
            }
        }
        if (best_s) { r->G = best_s; r->nt = best_nt; r->flags = fls | kGeoNtLoads; return true; }
        // (2) the tile-at-a-time three-stage kernel, where the streaming form's geometry fails
        const uint32_t g_unit = (uint32_t)(512 * spl / ct_gcd(512 * spl, step));             // tiles start on rows when G is a multiple of this
        uint32_t best = 0;
        for (uint32_t g = g_unit; g <= 64; g += g_unit) {
            const FixedRules t = rules(g, fl3);
            const uint64_t rows = t.rows(512, spl);
            if (rows > kWholeRows || !t.pipe3_geometry_ok(spl, rows)) break;
            if (lds_for(g, W, S, D, T_lds, nullptr, 2, 1, lut8, fl3) > kLdsMax) break;
            if (p->n_windows < g) break;
            best = g;
        }
        if (best) { r->G = best; r->nt = 512; r->flags = fl3; return true; }
        return false;
    }
    // fast phase 1: tiles start on a row boundary and a whole tile is prefetched
    auto on_rows = [&](const FixedRules &t, int nt) { const uint64_t rows = t.rows(nt, spl); return t.fast_p1_ok(nt, spl, rows, rows <= kWholeRows, true); };
    if (T < 64 || !is_pow2(D)) return false;      // the recipes below were measured on filters of 64 taps and more, power-of-two decimation
    const uint32_t fl_tile = kGeoPackedTile | kGeoDeferFft;
    // Two outcomes of the recipe below are kept as they have always been, although the kernels' rules say otherwise (changing them
    // changes which kernel a plan runs, which wants a measurement of its own):
    //  * the stride's parity is not asked about (the rules are asked with the stride rounded down to even): an odd stride S >= W builds
    //    with the register-tiled FIR falling back to one output per lane (kFirTile4 needs an even stride);
    //  * half-window tiles are asked for from W = 1024 up, but from W = 2048 the deferred FFT they need has no wave to run on
    //    (defer_fft_ok: W / 4 + 64 <= 512 lanes), so that build fails its static_assert and the plan steps down the candidate list.
    if (W >= 512 && (uint64_t)T >= 4ull * D && rules(1, fl_tile, 2, 2, 4, S & ~1u).kPackedTile) {
        // one long window per tile (cfg4's recipe): two outputs per lane as straight-line packed code with in-chain
        // snapshots, the previous window's FFT + epilogue on idle waves, as many threads as the FIR has lanes for
        // half-window tiles (two passes per window, two workgroups per CU) where a pass is a whole number of rows of 512 threads
        const uint32_t fl_half = fl_tile | kGeoHalfTile | kGeoFastP1 | kGeoNtLoads, fl_rows = fl_tile | kGeoFastP1 | kGeoNtLoads | kGeoNtInner;
        const FixedRules h = rules(1, fl_half, 2, 2, 4);
        const bool half_ok = W >= 1024 && h.kHalfTile && on_rows(h, 512);
        const int nt = half_ok ? 512 : (W >= 1024 ? 1024 : 512);
        const uint32_t fl = half_ok ? fl_half : (on_rows(rules(1, fl_rows, 2, 2, 4), nt) ? fl_rows : fl_tile);
        if (lds_for(1, W, S, D, T_lds, nullptr, 2, 2, lut8, fl) > kLdsMax) return false;
        r->G = 1; r->nt = nt; r->batch = 2; r->flags = fl; r->firr = 2; r->firb = 4;
        return true;
    }
    if (W <= 256) {
        // 64..256 outputs per tile of 256 threads (cfg3' recipe): packed lane-per-output FIR on a 16-byte-row tile; where the
        // FIR leaves a wave idle, the previous tile's FFT + epilogue runs there
        const uint32_t g = W >= 128 ? 1u : 128u / W;
        const FixedRules d2 = rules(g, kGeoNoSplit | kGeoDeferFft, 2);
        if (!d2.kPairFir) return false;
        const bool defer = d2.defer_fft_ok(true, 256);
        const uint32_t bt = defer ? 2u : 1u, fl_base = kGeoNoSplit | (defer ? kGeoDeferFft : 0u), fl_rows = fl_base | kGeoFastP1 | kGeoNtLoads | kGeoNtInner;
        const uint32_t fl = on_rows(rules(g, fl_rows, bt), 256) ? fl_rows : fl_base;
        if (p->n_windows < g || lds_for(g, W, S, D, T_lds, nullptr, 2, bt, lut8, fl) > kLdsMax / 2) return false;      // at least two workgroups per CU
        r->G = g; r->nt = 256; r->batch = bt; r->flags = fl;
        return true;
    }
    return false;
}

// The candidates of a chain plan without a tile hint, best first; every list ends in a kernel that is always to be had.
std::vector<Candidate> chain_candidates_of(const qd_plan *p, uint32_t T_lds, bool windowed) {
    const qd_chain_desc &d = p->d;
    const int policy = p->opt.kernel_policy, spl = spl_of(d.format), bps = bps_of(d.format);
    const uint32_t W = p->W, S = p->S;
    const bool write_sink = d.epilogue == QD_EPI_CF32_BLOCKS;
    // plan-time builds: QD_KERNEL_NO_PLAN_TIME / QD_KERNEL_GENERIC never
    const bool jit_ok = policy != QD_KERNEL_GENERIC && policy != QD_KERNEL_NO_PLAN_TIME;
    Candidate plain;
    plain.G = plain_tiles(p, T_lds);
    Candidate generic = plain;
    generic.wg_regs = dyn_lb(p->nco, d.format);
    // shape-specialised built-in kernels (kFixed): exact arithmetic; QD_MODE_FAST prefers a fused build of the shape's recipe
    const FixedEntry *fixed = (p->has_fir && !write_sink && policy != QD_KERNEL_GENERIC && !windowed) ? find_fixed(d.format, p->nco, W, S, p->D, p->T) : nullptr;
    const bool fast = d.mode == QD_MODE_FAST && p->has_fir && jit_ok && !write_sink;
    Candidate recipe;
    const bool has_recipe = jit_ok && p->has_fir && (!fixed || fast) && geometry_recipe(p, T_lds, &recipe);
    Candidate table;
    if (fixed) {
        table.src = Candidate::kTable; table.fixed = fixed;
        table.G = fixed->G; table.nt = fixed->nt; table.pad = (uint32_t)fixed->pad; table.batch = (uint32_t)fixed->batch;
        table.flags = (uint32_t)fixed->flags; table.lb = fixed->lb; table.wg_regs = std::max(1, fixed->lb * 256 / fixed->nt);
        if (!has_recipe) return {table};
    }
    if (has_recipe) {
        if (fast) recipe.flags |= kGeoFastFma;
        // no fused build to be had: the exact built-in kernel with ITS tiling, not the plain one
        if (fixed) return {chain_build(p, recipe, true), table};
        // (the write sink's only other kernel is the generic one)
        if (write_sink) return {chain_build(p, recipe, true), generic};
        return {chain_build(p, recipe, true), chain_build(p, plain, false), generic};
    }
    if (jit_ok && !write_sink && p->has_fir && (uint64_t)p->T >= 8ull * p->D) {
        // FIR-dominated shapes (>= 8 taps per input sample): a tile's FIR phase is latency-bound — one wave walks all T taps however
        // few outputs the tile has — so take the largest tile with <= 512 FIR outputs that LDS allows, 512 threads, a 256-VGPR budget
        // and scalar accumulate chains (measured 1.3-2.9x over the small-tile default on six such shapes, scripts/policy_probe.py;
        // DESIGN.md section 7); 16-byte aligned LDS rows (pad 2): ds_read_b128 sample pairs in the tap loop (FixedGeo::kPad)
        auto outs = [&](uint32_t g) { return S < W ? (uint64_t)(g - 1) * S + W : (uint64_t)g * W; };
        Candidate lf;
        lf.nt = 512; lf.pad = 2; lf.lb = 2; lf.noslp = 1;
        while (lf.G < 64 && outs(lf.G + 1) <= 512 && lds_for(lf.G + 1, W, S, p->D, T_lds, nullptr, 2, 1, lut8_of(d.format)) <= kLdsMax) ++lf.G;
        if (p->n_windows && lf.G > p->n_windows) lf.G = (uint32_t)p->n_windows;
        return {chain_build(p, lf, true), chain_build(p, plain, false), generic};
    }
    // chains without a lowpass: the wave-local kernels (qd_chain.h).  Their row tables and lane table are laid out for NCO rows of
    // 512 samples.  Plan-time builds: cached ones always, a new one for streams of 1 GiB and more.
    auto spark = [&](uint32_t ts, uint32_t flags, int lb) {
        Candidate c;
        c.src = Candidate::kBuiltinSpark; c.spark_ts = ts; c.G = ts / W; c.nt = (int)(kSparkRow / spl); c.flags = kGeoSpark | flags; c.lb = c.wg_regs = lb;
        return c;
    };
    auto spark_build = [&](Candidate c, int nco, uint32_t key_S, int rch) {      // (their keys are not chain_build's)
        c.src = Candidate::kBuild;
        c.key = JitKey{d.format, nco, 0, rch, 1, c.lb, kThreads, W, key_S, 1, 0, c.G, 8, 1, 0, 1, 1, c.flags, d.epilogue};
        return c;
    };
    const bool pow2_spark2 = W == 128 || W == 256 || W == 512 || W == 1024;
    // width 16 or 64 columns: the plan-time kernel that runs the base butterflies out of the row registers (k_spark2);
    // tile = 64 lanes x 2 columns x base rows
    auto spark2 = [&](bool ov_shift) {
        const uint32_t fbase = (ilog2(W) & 1) ? 8u : 16u;
        const int lb2 = p->has_shift ? (fbase == 8 ? 3 : 2) : (fbase == 8 ? 4 : 3);
        Candidate c = spark(128u * fbase, kGeoSparkReg, lb2);
        c.spark_R = ov_shift ? W / S : 0;
        // (the kernel's own geometry is windows side by side: S = W also where the plan's windows overlap with a shift, see spark_R)
        return spark_build(c, p->nco, ov_shift ? W : S, 0);
    };
    // the built-in k_spark with the width a compile-time constant (one base butterfly instead of five; with a shift the lane constants
    // come out of an LDS copy of the lane table: four waves per SIMD at either tile size); rch = chunks per tile
    auto spark_jit = [&](uint32_t R) {
        Candidate c = spark(spark_tile(W, p->nco), 0, 4);
        c.spark_R = R; c.spark_jt_lds = p->has_shift;
        return spark_build(c, p->nco, W, (int)(c.spark_ts / (64u * (uint32_t)spl)));
    };
    const bool spark_ok = !p->has_fir && W <= kSparkMaxW && !write_sink && policy != QD_KERNEL_GENERIC && !windowed;
    if (spark_ok && S == W) {
        const uint32_t ts = spark_tile(W, p->nco);
        if (!jit_ok) return {spark(ts, 0, spark_lb(ts, p->nco))};
        if (!pow2_spark2) return {spark_jit(0), spark(ts, 0, spark_lb(ts, p->nco))};
        return {spark2(false), spark_jit(0), spark(ts, 0, spark_lb(ts, p->nco))};
    }
    // OVERLAPPING windows (`sparkfft -width 4 -stride 2`: README example 1), plan-time builds only: W = 128 ... 1024 in ONE launch of
    // k_spark2 built for the stride (the overlap comes out of the caches; with a shift, the S = W build in interleaved launches);
    // W = 2 ... 8 without a shift on k_spark0, a window per lane, no LDS (W = 16 is bit-exact too but 2x slower: quarter-filled stores);
    // where the stride divides the width, R = W / S launches of k_spark over the windows phi, phi + R, ... (side by side in the stream
    // shifted by phi S), each writing every R-th output row (the lean norms and glyph sinks)
    if (spark_ok && S < W && jit_ok && ((uint64_t)S * bps) % 4 == 0) {
        const bool direct = !p->has_shift && W >= 2 && W <= 8 && ((uint64_t)W * bps) % 4 == 0;
        const bool one_launch = !p->has_shift && pow2_spark2;
        const bool lean_sink = d.epilogue == QD_EPI_NORMS_F32 || d.epilogue == QD_EPI_GLYPH_U8;
        const bool phases = W % S == 0 && W / S <= 32 && lean_sink && W >= (uint32_t)spl;
        if (direct || one_launch || phases) {
            std::vector<Candidate> list;
            if (pow2_spark2 && (!p->has_shift || lean_sink)) list.push_back(spark2(p->has_shift));
            if (direct) {
                Candidate c = spark(spark_tile(W, p->nco), kGeoSparkDirect, 4);
                c.G = 64;
                list.push_back(spark_build(c, 0, S, 0));
            }
            if (phases) list.push_back(spark_jit(W / S));
            list.push_back(chain_build(p, plain, false));
            list.push_back(generic);
            return list;
        }
    }
    if (jit_ok && !write_sink) return {chain_build(p, plain, false), generic};
    return {generic};
}

// A windowed plan (qd_chain_desc.windowing): the unwindowed list without the table and wave-local kernels, filtered down to the plan-time
// builds of k_chain — which get the variant bit kGeoWindow — and the generic kernel, which tests ChainParams::window.
std::vector<Candidate> chain_candidates(const qd_plan *p, uint32_t T_lds) {
    const bool windowed = p->d.windowing != 0 && p->d.epilogue != QD_EPI_CF32_BLOCKS;
    std::vector<Candidate> list = chain_candidates_of(p, T_lds, windowed);
    if (!windowed) return list;
    std::vector<Candidate> out;
    for (Candidate c : list) {
        if (c.src == Candidate::kGeneric) { out.push_back(c); continue; }
        if (c.src != Candidate::kBuild || family_of(c.flags) != kFamChain) continue;
        c.flags |= kGeoWindow; c.key.flags |= kGeoWindow;
        out.push_back(c);
    }
    return out;
}

// Commits the chosen candidate to the plan: tiling, LDS sizes, kernels (jit_fn: the plan-time build, when it is one).
int commit_candidate(qd_plan *p, const Candidate &c, hipFunction_t jit_fn, uint32_t T_lds) {
    const int fmt = p->d.format;
    p->fixed = c.fixed;
    p->jit_fn = jit_fn;
    p->spark = (c.flags & kGeoSpark) != 0;
    const Family fam = family_of(c.flags);
    p->spark_ts = c.spark_ts; p->spark_R = c.spark_R;
    p->geo.G = c.G; p->nt = c.nt; p->kflags = c.flags;
    p->launch_nt = family_threads(c.nt, c.flags);
    // the generic kernels (pad 1, batch 1) fit inside the same allocation; the streaming write kernel is laid out for T, the generic
    // kernels' tile (an unaligned tail) for T + tile_extra
    const bool ws = (c.flags & kGeoWriteSink) != 0;
    uint32_t raw_elems = 0;
    p->geo.lds_bytes = lds_for(c.G, p->W, p->S, p->D, ws ? p->T : T_lds, &raw_elems, c.pad, c.batch, lut8_of(fmt), c.flags, &p->geo.lds_main, spl_of(fmt), c.nt);
    if (ws) p->geo.lds_bytes = std::max(p->geo.lds_bytes, lds_for(c.G, p->W, p->S, p->D, T_lds, &raw_elems, 1, 1, lut8_of(fmt)));
    if (!(c.flags & kGeoHalfTile) && fam != kFamPipe3 && fam != kFamPipe3s) p->geo.lds_main = p->geo.lds_bytes;      // (only those are smaller than the generic layout on purpose)
    if (p->spark) p->geo.lds_main = (size_t)spark_lds_bytes(p->W, c.spark_ts, (fam == kFamSpark2 && p->has_shift) || c.spark_jt_lds);   // plan-time builds with a shift: + the NCO lane table
    if (fam == kFamSpark0) p->geo.lds_main = 16;                         // k_spark0 uses no LDS (a token size: 0 means "the generic layout's")
    p->geo.lds_raw_elems = raw_elems;
    p->geo.Dp = p->D + ((p->D % 2 == 0) ? 1 : 0);
    if ((uint64_t)raw_elems * p->D >= (1ull << 32)) return fail(QD_ERR_UNSUPPORTED, "tile too large");
    // (a k_spark2 plan's built-in kernel is the runtime-width k_spark of its tile: take_fft's row-offset launches run it)
    const bool windowed = p->d.windowing != 0 && p->d.epilogue != QD_EPI_CF32_BLOCKS;
    p->fn = c.fixed ? c.fixed->fn : (p->spark ? pick_spark(fmt, p->nco, c.spark_ts) : pick_generic(fmt, p->nco, p->has_fir, true, windowed));
    p->fn_unaligned = pick_generic(fmt, p->nco, p->has_fir, false, windowed);
    if (!p->fn || !p->fn_unaligned) return fail(QD_ERR_UNSUPPORTED, "no kernel built for this format (QD_DEV_FAST build?)");
    return QD_OK;
}

}  // namespace

extern "C" {

const char *qd_last_error(void) { return g_err.c_str(); }
const char *qd_version(void) { return "quadrs-hip 0.1 (gfx950)"; }

int qd_device_count(int *count) {
    if (!count) return fail(QD_ERR_INVALID, "count is NULL");
    HIPCHK(hipGetDeviceCount(count));
    return QD_OK;
}

int qd_set_device(int device) {
    HIPCHK(hipSetDevice(device));
    return QD_OK;
}

uint64_t qd_pair_bytes(int fmt) {
    switch (fmt) {
    case QD_FMT_CF32: return 8;
    case QD_FMT_CS8: case QD_FMT_CU8: return 2;
    case QD_FMT_CS16: return 4;
    }
    return 0;
}

double qd_shift_ratio(int64_t frequency, uint64_t sample_rate) {
    return (kPi64 * 2.0) * (double)frequency / (double)sample_rate;   // src/shift.rs:28, src/lib.rs:23
}

int qd_lowpass_design(uint64_t frequency, uint64_t sample_rate, size_t size, float *taps) {
    if (!taps) return fail(QD_ERR_INVALID, "taps is NULL");
    design_taps(frequency, sample_rate, size, taps);
    return QD_OK;
}

int qd_window_design(int windowing, size_t W, float *w) {
    if (!w) return fail(QD_ERR_INVALID, "w is NULL");
    if (windowing != 0 && windowing != 1) return fail(QD_ERR_INVALID, "unknown windowing %d", windowing);
    if (windowing == 0) { for (size_t i = 0; i < W; ++i) w[i] = 1.0f; return QD_OK; }
    std::vector<float> win;
    blackman_harris(W, &win);
    if (W) memcpy(w, win.data(), W * sizeof(float));
    return QD_OK;
}

// bits::scan, src/bits.rs:3-55 (host arithmetic, f64)
int qd_bits_scan(const uint8_t *marks, size_t n, double scale, uint8_t *bits, size_t cap, size_t *produced, double *error) {
    if (produced) *produced = 0;
    if (error) *error = 0.0;
    if ((!marks && n) || (!bits && cap) || !produced || !error) return fail(QD_ERR_INVALID, "qd_bits_scan: NULL argument");
    if (!std::isfinite(scale) || !(scale > 0.0)) return fail(QD_ERR_INVALID, "qd_bits_scan: scale must be finite and > 0");
    auto as_u64 = [](double v) { return v >= 18446744073709551616.0 ? UINT64_MAX : (v > 0.0 ? (uint64_t)v : 0ull); };      // Rust `as u64`: saturating
    const uint64_t half = as_u64(std::round(scale / 2.0));                   // f64::round: halves away from zero, like std::round
    // run_of (:40-55): the index where the first stretch of more than `half` consecutive values != val began, else the length
    auto run_of = [&](size_t from, bool val) -> size_t {
        uint64_t bad = 0;
        for (size_t i = from; i < n; ++i) {
            bad = ((marks[i] != 0) != val) ? bad + 1 : 0;
            if (bad > half) return i + 1 - (size_t)bad - from;
        }
        return n - from;
    };
    size_t i = 0;
    uint64_t count = 0;
    bool bit = false, stuck = false;
    double err = 0.0;
    while (i != n) {
        const size_t found = run_of(i, bit);
        i += found;
        if (found <= half) {
            // :13-15 `continue`s without flipping `bit`: before the end of the data the next run_of starts on the stretch that stopped
            // this one and returns 0, for ever
            if (i != n) { stuck = true; break; }
            continue;
        }
        const double b = (double)found / scale, rounded = std::round(b);
        err += std::fabs(b - rounded);
        const uint64_t emit = as_u64(rounded);
        for (uint64_t k = 0; k < emit && count + k < cap; ++k) bits[count + k] = bit ? 1 : 0;
        count = emit > UINT64_MAX - count ? UINT64_MAX : count + emit;
        bit = !bit;
    }
    *error = err;
    *produced = count > (uint64_t)SIZE_MAX ? SIZE_MAX : (size_t)count;
    if (count > cap) return fail(QD_ERR_INVALID, "qd_bits_scan: %llu bits do not fit cap %zu", (unsigned long long)count, cap);
    if (stuck) return fail(QD_ERR_PANIC, "bits::scan never terminates here (src/bits.rs:9-15): a run of at most half = %llu ends at mark %zu of %zu and the loop continues without flipping",
                           (unsigned long long)half, i, n);
    return QD_OK;
}

int qd_plan_destroy(qd_plan *p);
constexpr int kNeedComposite = 1000;       // plan_init -> qd_plan_create_ex: build the two-stage plan (never leaves the library)

static int plan_init(qd_plan *p, const qd_chain_desc &d, uint64_t len, uint64_t rate) {
    (void)hipGetDevice(&p->device);
    p->has_shift = d.has_shift != 0;
    p->has_fir = d.has_lowpass != 0;
    p->W = (uint32_t)d.width; p->logW = ilog2(d.width); p->S = (uint32_t)d.stride;
    if (d.epilogue == QD_EPI_CF32_BLOCKS) {          // tiles are sub-blocks of <= 256 outputs of a read_at block of d.width
        p->blk_len = (uint32_t)d.width;
        p->W = p->blk_len < 256 ? p->blk_len : 256;
        const uint32_t c = (uint32_t)(d.taps - d.taps / 2);
        p->tile_extra = c > d.decimate ? c - (uint32_t)d.decimate : 0;
        // a sub-block's FIR input (W D + T + extra samples) must fit the LDS tile: long decimations take shorter sub-blocks
        while (p->W > 1 && lds_for(1, p->W, p->W, (uint64_t)d.decimate, d.taps + p->tile_extra, nullptr, 1, 1, lut8_of(d.format)) > kLdsMax) p->W /= 2;
        p->logW = ilog2(p->W); p->S = p->W;
        p->blk_subs = p->blk_len / p->W;
    }
    p->D = p->has_fir ? (uint32_t)d.decimate : 1;
    p->T = p->has_fir ? (uint32_t)d.taps : 0;
    p->dec_len = len; p->out_rate = rate;
    if (d.epilogue == QD_EPI_CF32_BLOCKS) p->n_windows = (d.n_samples - d.taps) / (d.width * d.decimate);   // full read_at blocks
    else p->n_windows = sink_windows(d.epilogue, len, d.width, d.stride);
    p->ratio = p->has_shift ? qd_shift_ratio(d.shift_hz, d.sample_rate) : 0.0;

    // |place| = n*|ratio| over the whole stream decides the NCO order once per plan: the dropped
    // second-order term is r^2/2 with |r| <= ulp(place)/2; below 2^28 rad that is <= 1.1e-16, inside the
    // scheme's ~4e-16 error budget, above it the second-order kernel is used
    p->nco = !p->has_shift ? 0 : ((std::fabs(p->ratio) * (double)d.n_samples > 268435456.0) ? 2 : 1);
    if (p->has_shift && (p->opt.nco_order == 1 || p->opt.nco_order == 2)) p->nco = p->opt.nco_order;
    if (const char *e = dev_env("QD_DEBUG_SKIP")) p->dbg = (uint32_t)atoi(e);     // development builds: timing-only ablation
    const int policy = p->opt.kernel_policy;

    const uint32_t T_lds = p->T + p->tile_extra;     // LDS sizing sees the extended tile
    if (lds_for(1, p->W, p->S, p->D, T_lds, nullptr, 1, 1, lut8_of(d.format)) > kLdsMax) {
        // LowPass::read_at allocates whatever buf.len() * D + T asks for (src/filter.rs:68-69); one workgroup's LDS does not.  Windows that
        // lie side by side run as a two-stage (composite) plan instead — qd_plan_create_ex builds it on this status
        if (p->has_fir && d.epilogue != QD_EPI_CF32_BLOCKS && p->S == p->W) return kNeedComposite;
        return fail(QD_ERR_UNSUPPORTED, "one window (W*D+T = %llu samples) exceeds the 160 KiB LDS tile and the windows overlap or leave gaps (stride != width)",
                    (unsigned long long)((uint64_t)d.width * (d.has_lowpass ? d.decimate : 1) + (d.has_lowpass ? d.taps : 0)));
    }
    // qd_plan_options.tile_hint = {G, NT, FIRR, FIRB, LB, PAD}: force a plan-time build with this tiling instead of the table /
    // heuristics (LB = waves per SIMD the build is register-budgeted for: 4 -> 128 VGPRs, 2 -> 256; PAD = LDS pad elements per row)
    // [6] = tiles per FFT batch (FixedGeo::kBatch) | kernel variant flags << 8, [7] = workgroups per CU (0: as many as LDS / registers
    // admit, at most 4)
    const uint32_t *h = p->opt.tile_hint;
    const bool hinted = h[0] || h[1];
    Candidate hint;
    if (hinted) {
        hint.G = h[0]; hint.nt = (int)h[1]; hint.firr = h[2] ? h[2] : 1u; hint.firb = h[3] ? h[3] : 8u; hint.lb = (int)(h[4] ? h[4] : 4u);
        hint.pad = h[5] ? h[5] : 1u; hint.batch = (h[6] & 0xffu) ? (h[6] & 0xffu) : 1u; hint.flags = h[6] >> 8;
        hint.required = true;
        if (!(p->has_fir && d.epilogue != QD_EPI_CF32_BLOCKS && hint.lb >= 1 && hint.lb <= 8 && hint.G >= 1 &&
              (hint.nt == 256 || hint.nt == 512 || hint.nt == 1024) && (hint.pad == 1 || hint.pad == 2) && hint.batch <= 64 && h[7] <= 8 &&
              (hint.flags & ~kHintGeoBits) == 0 &&      // a removed (reserved) variant bit is refused here, before any build
              lds_for(hint.G, p->W, p->S, p->D, T_lds, nullptr, hint.pad, hint.batch, lut8_of(d.format), hint.flags, nullptr, spl_of(d.format), hint.nt) <= kLdsMax))
            return fail(QD_ERR_INVALID, "tile_hint {%u,%u,%u,%u,%u,%u,%u,%u} does not fit this chain", hint.G, (uint32_t)hint.nt, hint.firr, hint.firb,
                        (uint32_t)hint.lb, hint.pad, hint.batch, h[7]);
    }
    // Plan-time specialisation (qd_plan_options.kernel_policy): a cached build is always used; a NEW build only when forced, for tile
    // hints and QD_MODE_FAST, or when the stream is at least 1 GiB
    const uint64_t in_bytes = (uint64_t)d.n_samples * bps_of(d.format);
    const bool may_compile = policy == QD_KERNEL_SPECIALISE || hinted || in_bytes >= (1ull << 30) || d.mode == QD_MODE_FAST;
    if (p->has_fir) { p->taps_h.resize(p->T); design_taps(d.lowpass_hz, d.sample_rate, p->T, p->taps_h.data()); }
    if (hinted && d.windowing) {
        if (family_of(hint.flags) != kFamChain) return fail(QD_ERR_UNSUPPORTED, "tile_hint: only k_chain builds apply the plan's window");
        hint.flags |= kGeoWindow;
    }
    const std::vector<Candidate> cands = hinted ? std::vector<Candidate>{chain_build(p, hint, true)} : chain_candidates(p, T_lds);
    const Candidate *won = nullptr;
    std::string why;
    for (const Candidate &c : cands) {
        hipFunction_t fn = nullptr;
        if (c.src == Candidate::kBuild && !(fn = jit_chain_kernel(c.key, &why, may_compile))) {
            if (c.required) return fail(QD_ERR_UNSUPPORTED, "tile_hint build failed: %s", why.c_str());
            continue;
        }
        const int rc = commit_candidate(p, c, fn, T_lds);
        if (rc) return rc;
        won = &c;
        break;
    }
    if (!won) return fail(QD_ERR_UNSUPPORTED, "no kernel for this chain");      // (every list ends in a kernel that is always to be had)

    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) == hipSuccess) p->n_cu = prop.multiProcessorCount;
    // workgroups per CU: what LDS, the CU's 2048 threads and the kernel's register budget admit, at most 4
    const int by_lds = (int)(kLdsMax / (p->geo.lds_main ? p->geo.lds_main : p->geo.lds_bytes));
    p->wg_per_cu = std::min(4, std::max(1, by_lds));
    if (won->wg_regs) p->wg_per_cu = std::min(p->wg_per_cu, won->wg_regs);
    if (p->launch_nt > kThreads) p->wg_per_cu = std::min(p->wg_per_cu, 2048 / p->launch_nt);
    if (hinted && h[7] && (int)h[7] < p->wg_per_cu) p->wg_per_cu = (int)h[7];
    if (const char *e = dev_env("QD_WG_PER_CU")) { int v = atoi(e); if (v >= 1 && v <= 8) p->wg_per_cu = v; }      // development builds
    // Dynamic-LDS limit: the kernels are process-global objects shared by every plan, so the attribute is set to the
    // hardware maximum (160 KiB), never to one plan's tile — a later plan with a smaller tile must not lower the limit
    // under a live plan with a larger one (tests/test_gpu_robustness.py::test_two_live_plans_with_different_lds).
    if (p->jit_fn) {
        // the tiling (G, threads, LDS layout) was chosen for THIS kernel: the generic kernels cannot run in it, so no silent fallback
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(p->jit_fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax); e != hipSuccess)
            return fail(QD_ERR_HIP, "hipFuncSetAttribute(plan-time kernel, max dynamic LDS %zu): %s", kLdsMax, hipGetErrorString(e));
    }
    for (chain_fn f : {p->fn, p->fn_unaligned}) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(f), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
        if (e != hipSuccess)
            return fail(QD_ERR_HIP, "hipFuncSetAttribute(max dynamic LDS %zu): %s", kLdsMax, hipGetErrorString(e));
    }

    // constant tables
    p->fft = fft_layout(d.width);
    if (!p->fft.tw.empty()) {
        HIPCHK(hipMalloc(&p->tw_d, p->fft.tw.size() * sizeof(float2)));
        HIPCHK(hipMemcpy(p->tw_d, p->fft.tw.data(), p->fft.tw.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (p->has_fir) {
        HIPCHK(hipMalloc(&p->taps_d, p->T * sizeof(float)));
        HIPCHK(hipMemcpy(p->taps_d, p->taps_h.data(), p->T * sizeof(float), hipMemcpyHostToDevice));
    }
    if (p->has_shift) {
        const uint32_t ROW = p->nt * spl_of(d.format);
        HIPCHK(hipMalloc(&p->jtab_d, ROW * sizeof(LaneEntry)));
        hipLaunchKernelGGL(k_jtab, dim3((ROW + 255) / 256), dim3(256), 0, 0, p->ratio, ROW, p->jtab_d);
        HIPCHK(hipGetLastError());
        if (p->nt != kThreads) {
            const uint32_t ROW256 = kThreads * spl_of(d.format);
            HIPCHK(hipMalloc(&p->jtab256_d, ROW256 * sizeof(LaneEntry)));
            hipLaunchKernelGGL(k_jtab, dim3((ROW256 + 255) / 256), dim3(256), 0, 0, p->ratio, ROW256, p->jtab256_d);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipDeviceSynchronize());
    }
    return QD_OK;
}


namespace {
struct DeviceGuard {                       // hipSetDevice is per host thread: run a plan on the device it was made on
    int prev = -1; bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// Equal, contiguous, tile-aligned window ranges (quadrs_amd/shard.py::partition states the same rule for the
// one-process-per-GPU path): shard g owns the source samples from its first window's start up to the next shard's
// first window's start, and reads `halo` samples beyond that.
void partition_windows(uint64_t n_windows, uint32_t n_shards, uint64_t step, uint64_t rpw, uint32_t tile, std::vector<qd_shard_info> *out) {
    out->assign(n_shards, qd_shard_info{});
    uint64_t per = (n_windows + n_shards - 1) / n_shards;
    per = (per + tile - 1) / tile * tile;
    const uint64_t total_end = n_windows ? (n_windows - 1) * step + rpw : 0;
    for (uint32_t g = 0; g < n_shards; ++g) {
        qd_shard_info &s = (*out)[g];
        s.w0 = std::min<uint64_t>(n_windows, (uint64_t)g * per);
        s.w1 = std::min<uint64_t>(n_windows, (uint64_t)(g + 1) * per);
        uint64_t own_first = s.w0 * step;
        uint64_t own_end = (g + 1 < n_shards && s.w1 < n_windows) ? s.w1 * step : total_end;
        if (s.w1 == s.w0) { own_first = total_end; own_end = total_end; }
        const uint64_t need_end = s.w1 > s.w0 ? (s.w1 - 1) * step + rpw : own_first;
        s.own_first = own_first;
        s.own_count = own_end > own_first ? own_end - own_first : 0;
        s.halo = need_end > own_end ? need_end - own_end : 0;
    }
}
}  // namespace

// ------------------------------------------------------------------ plan creation: stage lists, cascades

namespace {
constexpr uint32_t kCascadeMaxInter = 8192;     // intermediate samples per window (W D2 + T2): the kernel's LDS envelope
constexpr uint32_t kCascadeMaxSub = 8192;       // source samples per sub-tile
constexpr uint32_t kCascadeMaxT1 = 4096;
constexpr uint64_t kCascadeMaxBlockSpan = 1ull << 31;     // write sink: source samples per read_at block ((B D2 + T2) D1 + T1)
constexpr uint32_t kCascadeMaxK = 512;                    // write sink: outputs per sub-block

struct StageGeo {
    bool routed = false;                        // [shift] [lowpass]: the one-stage plan
    int s0 = -1, l1 = -1, s1 = -1, l2 = -1, s2 = -1;     // stage indexes of the cascade shape
    uint64_t len = 0, rate = 0;                 // Samples::len() / sample_rate() the sink sees
    std::vector<uint64_t> in_rate;              // input rate of every stage
    uint64_t n_windows = 0, complete = 0;
    uint32_t D1 = 1, T1 = 0, D2 = 1, T2 = 0, n2 = 0;
    double ratio = 0.0;                         // the first shift's
};

// the reference's constructors and len() asserts, stage by stage at each stage's rate, then the shape
int stages_geo(const qd_chain_desc *desc, const qd_stage *st, size_t n, StageGeo *g) {
    if (!desc || (n && !st)) return fail(QD_ERR_INVALID, "desc/stages is NULL");
    if (desc->struct_size != sizeof(qd_chain_desc)) return fail(QD_ERR_INVALID, "qd_chain_desc size mismatch");
    const qd_chain_desc &d = *desc;
    if (d.has_shift || d.has_lowpass) return fail(QD_ERR_INVALID, "a stage list carries the shift / lowpass stages: has_shift = has_lowpass = 0");
    if (n > QD_MAX_STAGES) return fail(QD_ERR_INVALID, "%zu stages > QD_MAX_STAGES (%d)", n, QD_MAX_STAGES);
    if (const int rc = check_sink(d)) return rc;
    uint64_t len = d.n_samples, rate = d.sample_rate;
    g->in_rate.assign(n, 0);
    std::string shape;
    bool seen_shift = false;
    for (size_t i = 0; i < n; ++i) {
        const qd_stage &q = st[i];
        g->in_rate[i] = rate;
        if (q.kind == QD_STAGE_SHIFT) {
            const int64_t af = q.shift_hz < 0 ? -q.shift_hz : q.shift_hz;
            if (rate == 0 || !(af < (int64_t)(rate / 2)))
                return fail(QD_ERR_PANIC, "stage %zu: frequency must be under half the sample rate %llu (src/shift.rs:20-24)", i, (unsigned long long)rate);
            if (!seen_shift) g->ratio = qd_shift_ratio(q.shift_hz, rate);     // the FIRST shift's, whatever its value (0 Hz included)
            seen_shift = true;
            shape += 'S';
        } else if (q.kind == QD_STAGE_LOWPASS) {
            if (q.decimate == 0) return fail(QD_ERR_PANIC, "stage %zu: decimate 0 divides by zero (src/filter.rs:47)", i);
            if (q.taps < 2) return fail(QD_ERR_PANIC, "stage %zu: lowpass size < 2 underflows (src/filter.rs:74)", i);
            if (q.taps > 65536 || q.decimate > 65536) return fail(QD_ERR_UNSUPPORTED, "stage %zu: taps/decimate too large", i);
            if (len < q.taps) return fail(QD_ERR_PANIC, "stage %zu: inner.len() %llu < filter.len() %llu (src/filter.rs:46)", i, (unsigned long long)len,
                                          (unsigned long long)q.taps);
            len = 1 + (len - q.taps) / q.decimate;     // LowPass::len, src/filter.rs:47
            rate = rate / q.decimate;                  // src/filter.rs:51
            shape += 'L';
        } else {
            return fail(QD_ERR_INVALID, "stage %zu: unknown kind %d", i, q.kind);
        }
    }
    if (d.epilogue != QD_EPI_CF32_BLOCKS && len < d.width)
        return fail(QD_ERR_PANIC, "len %llu < width %llu: u64 underflow at src/fft.rs:28,86", (unsigned long long)len, (unsigned long long)d.width);
    g->len = len; g->rate = rate;
    g->n_windows = d.epilogue == QD_EPI_ROWS_F32 ? 0 : sink_windows(d.epilogue, len, d.width, d.stride);
    g->routed = shape.empty() || shape == "S" || shape == "L" || shape == "SL";
    size_t k = 0;
    auto take = [&](char c) { if (k < shape.size() && shape[k] == c) return (int)k++; return -1; };
    g->s0 = take('S'); g->l1 = take('L'); g->s1 = take('S');
    if (g->l1 >= 0) { g->l2 = take('L'); if (g->l2 >= 0) g->s2 = take('S'); }
    if (g->l1 >= 0) { g->D1 = (uint32_t)st[g->l1].decimate; g->T1 = (uint32_t)st[g->l1].taps; }
    if (g->routed) return QD_OK;
    if (d.epilogue == QD_EPI_ROWS_F32)
        return fail(QD_ERR_UNSUPPORTED, "QD_EPI_ROWS_F32 behind a cascade (%s) is not built: the caller pulls the rows through the stages into qd_take_fft", shape.c_str());
    if (g->l1 < 0 || k != shape.size())
        return fail(QD_ERR_UNSUPPORTED, "stage list %s is not a fused shape ([shift] lowpass [shift] [lowpass [shift]]): the caller runs it stage by stage",
                    shape.c_str());
    if (g->l2 >= 0) { g->D2 = (uint32_t)st[g->l2].decimate; g->T2 = (uint32_t)st[g->l2].taps; }
    if (d.epilogue == QD_EPI_CF32_BLOCKS) {
        // the write sink: read_at blocks of B = width outer outputs, side by side whatever the stride (src/lib.rs:178-213), run as
        // sub-blocks (k_cascade_write): a sub-block of one output reads T2 inter samples, a block's source span is indexed in 32 bits
        if (g->T1 > kCascadeMaxT1) return fail(QD_ERR_UNSUPPORTED, "cascade: a first stage of %u taps exceeds the kernel's sub-tile (%u taps)", g->T1, kCascadeMaxT1);
        if (g->T2 > kCascadeMaxInter)
            return fail(QD_ERR_UNSUPPORTED, "cascade write: a second stage of %u taps exceeds one sub-block's intermediate budget (%u)", g->T2, kCascadeMaxInter);
        const uint64_t n2 = g->l2 >= 0 ? d.width * g->D2 + g->T2 : d.width, span = n2 * g->D1 + g->T1;
        if (span > kCascadeMaxBlockSpan)
            return fail(QD_ERR_UNSUPPORTED, "cascade write: a block's source span of %llu samples exceeds %llu", (unsigned long long)span,
                        (unsigned long long)kCascadeMaxBlockSpan);
        g->n2 = (uint32_t)n2;
        // full blocks: block b reads source samples [b B D2 D1, + span), every nested read returns its full length while they exist
        g->n_windows = g->complete = d.n_samples >= span ? (d.n_samples - span) / (d.width * g->D2 * g->D1) + 1 : 0;
        return QD_OK;
    }
    const uint64_t n2 = g->l2 >= 0 ? d.width * g->D2 + g->T2 : d.width;
    if (n2 > kCascadeMaxInter)
        return fail(QD_ERR_UNSUPPORTED, "cascade: a window's intermediate block of %llu samples exceeds the kernel's LDS budget (%u)", (unsigned long long)n2,
                    kCascadeMaxInter);
    if (g->T1 > kCascadeMaxT1) return fail(QD_ERR_UNSUPPORTED, "cascade: a first stage of %u taps exceeds the kernel's sub-tile (%u taps)", g->T1, kCascadeMaxT1);
    g->n2 = (uint32_t)n2;
    // window w reads source samples [w S D2 D1, + n2 D1 + T1): complete while they exist (src/samples.rs:17-27)
    const uint64_t span = n2 * g->D1 + g->T1, step = d.stride * g->D2 * g->D1;
    const uint64_t fit = d.n_samples >= span ? (d.n_samples - span) / step + 1 : 0;
    g->complete = fit < g->n_windows ? fit : g->n_windows;
    return QD_OK;
}

// the device half of a cascade plan: tables, taps, launch figures
int cascade_init(qd_plan *p, const StageGeo &g, const qd_stage *st) {
    const qd_chain_desc &d = p->d;
    (void)hipGetDevice(&p->device);
    p->casc = true;
    p->W = (uint32_t)d.width; p->logW = ilog2(d.width); p->S = (uint32_t)d.stride;
    p->c_D1 = g.D1; p->c_T1 = g.T1; p->c_D2 = g.D2; p->c_T2 = g.T2; p->c_n2 = g.n2;
    p->D = g.D1 * g.D2; p->T = g.T2 * g.D1 + g.T1;
    p->dec_len = g.len; p->out_rate = g.rate; p->n_windows = g.n_windows; p->c_complete = g.complete;
    p->ratio = g.ratio;
    p->geo.G = 1;
    p->c_flags = (g.s0 >= 0 ? kCascS0 : 0) | (g.s1 >= 0 ? kCascS1 : 0) | (g.l2 >= 0 ? kCascL2 : 0) | (g.s2 >= 0 ? kCascS2 : 0);
    const int sidx[3] = {g.s0, g.s1, g.s2};
    for (int k = 0; k < 3; ++k) p->c_ratio[k] = sidx[k] >= 0 ? qd_shift_ratio(st[sidx[k]].shift_hz, g.in_rate[sidx[k]]) : 0.0;
    // LDS: inter block | source sub-tile (>= the FFT buffer).  Sub-tiles of up to 512 FIR1 outputs.
    const bool l2 = g.l2 >= 0, write = d.epilogue == QD_EPI_CF32_BLOCKS;
    auto lds_of = [&](uint64_t n_inter, uint32_t M, uint32_t *inter, uint32_t *src) {
        const uint64_t ns = (uint64_t)(M - 1) * g.D1 + g.T1;
        uint64_t ie = n_inter ? n_inter + ((l2 && g.D2 % 2 == 0) ? n_inter / g.D2 + 1 : 0) + 1 : 0;
        uint64_t se = ns + (g.D1 % 2 == 0 ? ns / g.D1 + 1 : 0) + 1;
        if (!write && se < p->W) se = p->W;
        ie = (ie + 3) & ~3ull; se = (se + 3) & ~3ull;         // row bases on a 32-byte boundary
        *inter = (uint32_t)ie; *src = (uint32_t)se;
        return (size_t)((ie + se) * 8);
    };
    auto sub_tile = [&](uint64_t n_inter, uint64_t n_fir1) {   // the largest M (<= 512) whose sub-tile and LDS fit
        uint32_t M = n_fir1 < 512 ? (uint32_t)n_fir1 : 512;
        while (M > 1 && ((uint64_t)(M - 1) * g.D1 + g.T1 > kCascadeMaxSub || lds_of(n_inter, M, &p->c_inter, &p->c_src) > kLdsMax)) M = (M + 1) / 2;
        p->c_M = M;
        p->c_lds = lds_of(n_inter, M, &p->c_inter, &p->c_src);
        return p->c_lds <= kLdsMax && (uint64_t)(M - 1) * g.D1 + g.T1 <= kCascadeMaxSub;
    };
    bool fits = false;
    if (write) {
        // read_at blocks of B outputs in sub-blocks of K (the kernel's windows): the largest power of two K <= min(B, 512) whose inter
        // samples (K - 1) D2 + T2 fit the budget and whose LDS, with a sub-tile of 64 or more FIR1 outputs, leaves room for four
        // workgroups per CU (the kernel waits on LDS and barriers, not on issue); else the largest K that fits at all (K = 1 always
        // does: stages_geo's envelope)
        const uint32_t B = (uint32_t)d.width, K_max = B < kCascadeMaxK ? B : kCascadeMaxK;
        auto pick = [&](size_t lds_cap, uint32_t M_min) {
            for (uint32_t K = K_max; K >= 1; K /= 2) {
                const uint64_t ni = l2 ? (uint64_t)(K - 1) * g.D2 + g.T2 : 0, n_fir1 = l2 ? ni : K;
                if (ni > kCascadeMaxInter) continue;
                for (uint32_t M = 512; M >= M_min; M /= 2) {
                    if (!sub_tile(ni, M < n_fir1 ? M : n_fir1) || p->c_lds > lds_cap) continue;
                    p->W = K;
                    return true;
                }
            }
            return false;
        };
        fits = pick(kLdsMax / 4, 64) || pick(kLdsMax, 1);
        p->blk_len = B; p->blk_subs = B / p->W;
        p->logW = ilog2(p->W); p->S = p->W;
    } else {
        fits = sub_tile(g.n2, g.n2);
    }
    if (!fits) return fail(QD_ERR_UNSUPPORTED, "cascade: %zu bytes of LDS per workgroup exceed the %zu available", p->c_lds, kLdsMax);
    int by_lds = (int)(kLdsMax / p->c_lds);
    p->c_wg_per_cu = by_lds < 1 ? 1 : (by_lds > 8 ? 8 : by_lds);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) == hipSuccess) p->n_cu = prop.multiProcessorCount;
    for (const void *f : {reinterpret_cast<const void *>(k_cascade<0>), reinterpret_cast<const void *>(k_cascade<1>),
                          reinterpret_cast<const void *>(k_cascade<2>), reinterpret_cast<const void *>(k_cascade<3>),
                          reinterpret_cast<const void *>(k_cascade_write<0>), reinterpret_cast<const void *>(k_cascade_write<1>),
                          reinterpret_cast<const void *>(k_cascade_write<2>), reinterpret_cast<const void *>(k_cascade_write<3>)})
        if (hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax); e != hipSuccess)
            return fail(QD_ERR_HIP, "hipFuncSetAttribute(k_cascade, max dynamic LDS %zu): %s", kLdsMax, hipGetErrorString(e));
    if (!write) p->fft = fft_layout(d.width);          // the write sink has no transform
    if (!p->fft.tw.empty()) {
        HIPCHK(hipMalloc(&p->tw_d, p->fft.tw.size() * sizeof(float2)));
        HIPCHK(hipMemcpy(p->tw_d, p->fft.tw.data(), p->fft.tw.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
    p->taps_h = p->stage_taps[g.l1];
    HIPCHK(hipMalloc(&p->c_h1, g.T1 * sizeof(float)));
    HIPCHK(hipMemcpy(p->c_h1, p->stage_taps[g.l1].data(), g.T1 * sizeof(float), hipMemcpyHostToDevice));
    if (l2) {
        HIPCHK(hipMalloc(&p->c_h2, g.T2 * sizeof(float)));
        HIPCHK(hipMemcpy(p->c_h2, p->stage_taps[g.l2].data(), g.T2 * sizeof(float), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&p->c_jtab, 3 * kCascadeRow * sizeof(LaneEntry)));
    HIPCHK(hipMemset(p->c_jtab, 0, 3 * kCascadeRow * sizeof(LaneEntry)));
    for (int k = 0; k < 3; ++k)
        if (sidx[k] >= 0) {
            hipLaunchKernelGGL(k_jtab, dim3((kCascadeRow + 255) / 256), dim3(256), 0, 0, p->c_ratio[k], kCascadeRow, p->c_jtab + k * kCascadeRow);
            HIPCHK(hipGetLastError());
        }
    HIPCHK(hipDeviceSynchronize());
    return QD_OK;
}

void stage_taps_of(const qd_stage *st, size_t n, const StageGeo &g, std::vector<std::vector<float>> *t) {
    t->assign(n, {});
    for (size_t i = 0; i < n; ++i)
        if (st[i].kind == QD_STAGE_LOWPASS) { (*t)[i].resize(st[i].taps); design_taps(st[i].lowpass_hz, g.in_rate[i], st[i].taps, (*t)[i].data()); }
}
}  // namespace

int qd_stages_geometry(const qd_chain_desc *desc, const qd_stage *stages, size_t n_stages, qd_plan_info *info, uint64_t *complete) {
    if (!info || !complete) return fail(QD_ERR_INVALID, "info/complete is NULL");
    StageGeo g;
    int rc = stages_geo(desc, stages, n_stages, &g);
    if (rc) return rc;
    const qd_chain_desc &d = *desc;
    const bool write = d.epilogue == QD_EPI_CF32_BLOCKS;
    if (write && g.routed) return fail(QD_ERR_UNSUPPORTED, "qd_stages_geometry: the write sink's blocks are the one-stage plan's (qd_plan_get_info)");
    if (g.routed) {                  // the one-stage plan's figures: a single lowpass never fails a read
        g.complete = g.n_windows;
        g.n2 = (uint32_t)d.width;
    }
    memset(info, 0, sizeof *info);
    info->n_windows = g.n_windows;
    info->decimated_len = g.len;
    info->out_sample_rate = g.rate;
    info->out_bytes_per_window = write ? d.width * 8 : (d.epilogue == QD_EPI_NORMS_F32 || d.epilogue == QD_EPI_ROWS_F32) ? d.width * 4 : (d.epilogue == QD_EPI_GLYPH_U8 ? d.width : 1);
    info->raw_per_window = (uint64_t)g.n2 * g.D1 + g.T1;
    info->raw_step = (write ? d.width : d.stride) * g.D2 * g.D1;      // the write sink's blocks lie side by side
    info->ratio = g.ratio;
    *complete = g.complete;
    return QD_OK;
}

namespace {
int create_plan(const qd_chain_desc *desc, const qd_stage *stages, size_t n_stages, const qd_plan_options *options, bool list, qd_plan **out);

// rows per workgroup of the row-mode kernel and its LDS (QD_EPI_ROWS_F32).  A 256-thread workgroup filters and transforms one output
// per lane and pass, so G = 256 / W rows keep every lane busy where rows are short (one for W >= 256) — more would only queue behind
// the same lanes; G is halved while the tile takes more than half the CU's LDS, so that two workgroups still share a CU.
size_t rows_tile(uint32_t Wk, uint32_t S, uint32_t D, uint32_t T, bool lut8, uint32_t *G, uint32_t *raw_elems) {
    uint32_t g = Wk < 256 ? 256 / Wk : 1;
    if (g > 64) g = 64;
    for (;; g /= 2) {
        const FixedRules r = fixed_rules(Wk, S, D, T, g, 8, 1, 1, 1, 0);
        const size_t b = (size_t)generic_lds_bytes(r, lut8);
        if (g == 1 || b <= kLdsMax / 2) { *G = g; *raw_elems = (uint32_t)generic_raw_elems(r); return b; }
    }
}

// QD_EPI_ROWS_F32: the plan behind qd_plan_take_fft.  A power-of-two width runs the row-mode k_chain (unpack -> NCO -> FIR -> window ->
// Radix4 -> |X|); any other width up to 4096 runs k_bluestein — straight off the source without a lowpass, else over the rows'
// read_at blocks, which the same row-mode kernel writes as cf32 (its power-of-two width is then the next one above the row's).
int rows_init(qd_plan *p, const qd_chain_desc &d, uint64_t len, uint64_t rate) {
    (void)hipGetDevice(&p->device);
    if (p->opt.n_shards > 1) return fail(QD_ERR_UNSUPPORTED, "QD_EPI_ROWS_F32 is not sharded");
    p->rows = true;
    p->has_shift = d.has_shift != 0; p->has_fir = d.has_lowpass != 0;
    p->D = p->has_fir ? (uint32_t)d.decimate : 1;
    p->T = p->has_fir ? (uint32_t)d.taps : 0;
    p->dec_len = len; p->out_rate = rate; p->n_windows = 0;
    p->ratio = p->has_shift ? qd_shift_ratio(d.shift_hz, d.sample_rate) : 0.0;
    p->nco = !p->has_shift ? 0 : ((std::fabs(p->ratio) * (double)d.n_samples > 268435456.0) ? 2 : 1);      // as plan_init
    if (p->has_shift && (p->opt.nco_order == 1 || p->opt.nco_order == 2)) p->nco = p->opt.nco_order;
    const bool pow2 = is_pow2(d.width);
    if (!pow2 && d.width > 4096)
        return fail(QD_ERR_UNSUPPORTED, "take_fft width %llu: widths that are not a power of two are built up to 4096 (the reference front end's slider range, src/eui/mod.rs:157)", (unsigned long long)d.width);
    p->rows_blue = !pow2;
    p->blk_len = (uint32_t)d.width;
    p->logW = ilog2(d.width); p->W = 1u << p->logW;
    p->S = p->W + (p->has_fir ? (p->T + p->D - 1) / p->D : 0);
    p->nt = kThreads; p->launch_nt = kThreads;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) == hipSuccess) p->n_cu = prop.multiProcessorCount;
    const int fmt = d.format;
    if (pow2 || p->has_fir) {
        uint32_t raw_elems = 0;
        p->geo.lds_bytes = rows_tile(p->W, p->S, p->D, p->T, lut8_of(fmt), &p->geo.G, &raw_elems);
        if (p->geo.lds_bytes > kLdsMax || (uint64_t)raw_elems * p->D >= (1ull << 32))
            return fail(QD_ERR_UNSUPPORTED, "one row (W*D+T = %llu samples) exceeds the 160 KiB LDS tile", (unsigned long long)((uint64_t)d.width * p->D + p->T));
        p->geo.lds_main = p->geo.lds_bytes; p->geo.lds_raw_elems = raw_elems;
        p->geo.Dp = p->D + ((p->D % 2 == 0) ? 1 : 0);
        p->wg_per_cu = std::min(4, std::max(1, (int)(kLdsMax / p->geo.lds_bytes)));
        p->fn = p->fn_unaligned = pick_rows(fmt, p->nco, p->has_fir);
        if (!p->fn) return fail(QD_ERR_UNSUPPORTED, "no kernel built for this format (QD_DEV_FAST build?)");
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(p->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax); e != hipSuccess)
            return fail(QD_ERR_HIP, "hipFuncSetAttribute(max dynamic LDS %zu): %s", kLdsMax, hipGetErrorString(e));
        p->fft = fft_layout(p->W);
        if (!p->fft.tw.empty()) {
            HIPCHK(hipMalloc(&p->tw_d, p->fft.tw.size() * sizeof(float2)));
            HIPCHK(hipMemcpy(p->tw_d, p->fft.tw.data(), p->fft.tw.size() * sizeof(float2), hipMemcpyHostToDevice));
        }
    }
    if (p->has_fir) {
        p->taps_h.resize(p->T); design_taps(d.lowpass_hz, d.sample_rate, p->T, p->taps_h.data());
        HIPCHK(hipMalloc(&p->taps_d, p->T * sizeof(float)));
        HIPCHK(hipMemcpy(p->taps_d, p->taps_h.data(), p->T * sizeof(float), hipMemcpyHostToDevice));
    }
    if (p->has_shift) {                      // the lane table: entries j < 512 serve k_bluestein's rows of 512 samples as well
        const uint32_t ROW = kThreads * spl_of(fmt);
        HIPCHK(hipMalloc(&p->jtab_d, ROW * sizeof(LaneEntry)));
        hipLaunchKernelGGL(k_jtab, dim3((ROW + 255) / 256), dim3(256), 0, 0, p->ratio, ROW, p->jtab_d);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
    }
    return QD_OK;
}

// qd_chain_desc.windowing == 1: the device copy of blackman_harris(width) that every launch of the plan hands its kernel (plan_params)
int window_init(qd_plan *p) {
    std::vector<float> win;
    blackman_harris(p->d.width, &win);
    HIPCHK(hipMalloc(&p->win_own_d, win.size() * sizeof(float)));
    HIPCHK(hipMemcpy(p->win_own_d, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
    p->window_d = p->win_own_d;
    return QD_OK;
}

// a window larger than the LDS tile, windows side by side (plan_init's kNeedComposite): two plans behind the parent's handle
int composite_init(qd_plan *p, uint64_t rate) {
    if (p->opt.n_shards > 1) return fail(QD_ERR_UNSUPPORTED, "a window larger than the LDS tile runs as a two-stage plan, which is not sharded inside one process");
    const qd_chain_desc &d = p->d;
    qd_plan_options copt = p->opt;
    copt.n_shards = 0;
    memset(copt.tile_hint, 0, sizeof copt.tile_hint);
    qd_chain_desc a = d;                         // stage A: the same source chain into read_at blocks of W decimated samples
    a.stride = d.width; a.epilogue = QD_EPI_CF32_BLOCKS; a.has_range = 0;
    a.windowing = 0;                             // (the write sink has no transform: the window is stage B's)
    int rc = qd_plan_create_ex(&a, &copt, &p->cmp_a);
    if (rc) return rc;
    qd_chain_desc b{};                           // stage B: W-point windows side by side over the decimated stream
    b.struct_size = sizeof b;
    b.format = QD_FMT_CF32; b.sample_rate = rate ? rate : 1;
    b.n_samples = d.epilogue == QD_EPI_BUCKET2_U8 ? (p->n_windows + 1) * d.width : p->n_windows * d.width + 1;      // exactly n_windows windows (src/fft.rs:28,65 / :86)
    b.width = d.width; b.stride = d.width; b.epilogue = d.epilogue; b.mode = d.mode;
    b.has_range = d.has_range; b.range_min = d.range_min; b.range_max = d.range_max;
    b.windowing = d.windowing;
    rc = qd_plan_create_ex(&b, &copt, &p->cmp_b);
    if (rc) return rc;
    p->geo.G = 1;
    if (p->cmp_a->n_windows < p->n_windows || p->cmp_b->n_windows != p->n_windows)
        return fail(QD_ERR_UNSUPPORTED, "two-stage plan: stage window counts disagree (%llu blocks, %llu / %llu windows)", (unsigned long long)p->cmp_a->n_windows,
                    (unsigned long long)p->cmp_b->n_windows, (unsigned long long)p->n_windows);
    return QD_OK;
}

// sharded plans (options.n_shards > 1): the parent describes the whole stream; each shard gets a plan of its own, made from the same
// stage list on that shard's device
int make_shards(qd_plan *p, const qd_chain_desc *desc, const qd_stage *stages, size_t n_stages, bool list) {
    const uint32_t n_shards = p->opt.n_shards > 1 ? p->opt.n_shards : 1;
    const uint64_t step = (uint64_t)(p->blk_len ? p->blk_len : p->S) * p->D, rpw = (uint64_t)(p->blk_len ? p->blk_len : p->W) * p->D + p->T;
    // API windows of the write sink are whole blocks; interleaved launches take any window range, and keep their speed when it starts on a load vector
    uint32_t tile_api = p->blk_len ? 1u : p->geo.G;
    if (p->spark_R > 1) {
        tile_api = (uint32_t)spl_of(p->d.format); while (tile_api > 1 && ((uint64_t)(tile_api / 2) * p->S) % spl_of(p->d.format) == 0) tile_api /= 2;
        if (p->has_shift) tile_api = p->spark_R * (p->W < kSparkRow ? kSparkRow / p->W : 1u);      // ... and with a shift on the launches' NCO row grids
        p->phase_unit = tile_api;
    }
    partition_windows(p->n_windows, n_shards, step, rpw, tile_api, &p->shard_info);
    for (uint32_t g = 0; g < n_shards; ++g) p->shard_info[g].device = n_shards > 1 ? p->opt.shard_device[g] : p->device;
    qd_plan_options copt = p->opt;
    copt.n_shards = 0;
    for (uint32_t g = 0; g < n_shards && n_shards > 1; ++g) {
        DeviceGuard guard(p->opt.shard_device[g]);
        qd_plan *c = nullptr;
        const int rc = create_plan(desc, stages, n_stages, &copt, list, &c);
        if (rc) return rc;
        p->shards.push_back(c);
    }
    return QD_OK;
}

// The one creator behind qd_plan_create_ex and qd_plan_create_stages: a chain given as a stage list (desc's own has_shift /
// has_lowpass clear).  The reference's asserts and the stage list's shape come first (stages_geo), then the options, and every
// argument check before the first HIP call.  A routed list ([shift] [lowpass]) is the one-stage plan — a two-stage plan where a
// window exceeds the LDS tile —, any other fused list a cascade.  `list`: the plan records the list (qd_plan_get_stage_taps).
int create_plan(const qd_chain_desc *desc, const qd_stage *stages, size_t n_stages, const qd_plan_options *options, bool list, qd_plan **out) {
    StageGeo g;
    int rc = stages_geo(desc, stages, n_stages, &g);
    if (rc) return rc;
    qd_plan_options opt;
    rc = check_options(options, &opt);
    if (rc) return rc;
    qd_chain_desc d = *desc;
    if (d.epilogue != QD_EPI_ROWS_F32) {       // (that sink's window is qd_rows_desc's: the field is ignored like stride and range_*)
        if (d.windowing != 0 && d.windowing != 1) return fail(QD_ERR_INVALID, "unknown windowing %d", d.windowing);
        if (d.windowing && d.epilogue == QD_EPI_CF32_BLOCKS) return fail(QD_ERR_INVALID, "QD_EPI_CF32_BLOCKS has no transform to window: windowing must be 0");
    }
    if (g.routed) {                  // the one-stage description holds it: the same plan, kernels and bytes whichever entry point
        if (g.s0 >= 0) { d.has_shift = 1; d.shift_hz = stages[g.s0].shift_hz; }
        if (g.l1 >= 0) { d.has_lowpass = 1; d.lowpass_hz = stages[g.l1].lowpass_hz; d.decimate = stages[g.l1].decimate; d.taps = stages[g.l1].taps; }
        if (d.epilogue == QD_EPI_CF32_BLOCKS && !d.has_lowpass) return fail(QD_ERR_INVALID, "QD_EPI_CF32_BLOCKS needs a lowpass in the chain");
    }
    if (opt.n_shards > 1) {
        int n_dev = 0;
        HIPCHK(hipGetDeviceCount(&n_dev));
        for (uint32_t s = 0; s < opt.n_shards; ++s)
            if (opt.shard_device[s] < 0 || opt.shard_device[s] >= n_dev)
                return fail(QD_ERR_INVALID, "shard %u: device %d does not exist (%d visible)", s, opt.shard_device[s], n_dev);
    }
    qd_plan *p = new qd_plan();
    p->d = d;
    p->opt = opt;
    if (list) {
        p->stages.assign(stages, stages + n_stages);
        stage_taps_of(stages, n_stages, g, &p->stage_taps);
    }
    if (d.epilogue == QD_EPI_ROWS_F32) rc = rows_init(p, d, g.len, g.rate);      // (stages_geo has refused a cascade)
    else if (!g.routed) rc = cascade_init(p, g, stages);
    else if ((rc = plan_init(p, d, g.len, g.rate)) == kNeedComposite) rc = composite_init(p, g.rate);
    if (rc == QD_OK && !p->rows && !p->cmp_a && d.windowing == 1) rc = window_init(p);      // (a two-stage plan's window is stage B's)
    if (rc == QD_OK && !p->rows) rc = make_shards(p, desc, stages, n_stages, list);
    if (rc) { qd_plan_destroy(p); return rc; }
    *out = p;
    return QD_OK;
}
}  // namespace

int qd_plan_create_ex(const qd_chain_desc *desc, const qd_plan_options *options, qd_plan **out) {
    if (!desc || !out) return fail(QD_ERR_INVALID, "desc/plan is NULL");
    if (desc->struct_size != sizeof(qd_chain_desc)) return fail(QD_ERR_INVALID, "qd_chain_desc size mismatch");
    // this entry point has always checked the options, and the write sink's lowpass, before the chain
    qd_plan_options opt;
    if (const int rc = check_options(options, &opt)) return rc;
    if (desc->epilogue == QD_EPI_CF32_BLOCKS && !desc->has_lowpass) return fail(QD_ERR_INVALID, "QD_EPI_CF32_BLOCKS needs a lowpass in the chain");
    qd_chain_desc d = *desc;         // the stage list [shift] [lowpass]
    qd_stage st[2] = {};
    size_t n = 0;
    if (d.has_shift) { st[n].kind = QD_STAGE_SHIFT; st[n++].shift_hz = d.shift_hz; }
    if (d.has_lowpass) { st[n].kind = QD_STAGE_LOWPASS; st[n].lowpass_hz = d.lowpass_hz; st[n].decimate = d.decimate; st[n++].taps = d.taps; }
    d.has_shift = d.has_lowpass = 0;
    return create_plan(&d, st, n, &opt, false, out);
}

int qd_plan_create(const qd_chain_desc *desc, qd_plan **out) { return qd_plan_create_ex(desc, nullptr, out); }

int qd_plan_create_stages(const qd_chain_desc *desc, const qd_stage *stages, size_t n_stages, const qd_plan_options *options, qd_plan **plan) {
    if (!plan) return fail(QD_ERR_INVALID, "plan is NULL");
    return create_plan(desc, stages, n_stages, options, true, plan);
}

int qd_plan_get_stage_taps(const qd_plan *p, uint32_t stage, float *taps, size_t cap) {
    if (!p || !taps) return fail(QD_ERR_INVALID, "plan/taps is NULL");
    if (stage >= p->stages.size() || p->stages[stage].kind != QD_STAGE_LOWPASS)
        return fail(QD_ERR_INVALID, "stage %u is not a lowpass stage of the plan's stage list (%zu stages)", stage, p->stages.size());
    const std::vector<float> &t = p->stage_taps[stage];
    if (cap < t.size()) return fail(QD_ERR_INVALID, "taps buffer too small");
    memcpy(taps, t.data(), t.size() * sizeof(float));
    return QD_OK;
}

int qd_plan_complete_windows(const qd_plan *p, uint64_t *n) {
    if (!p || !n) return fail(QD_ERR_INVALID, "plan/n is NULL");
    if (p->rows) return fail(QD_ERR_INVALID, "a QD_EPI_ROWS_F32 plan has no window loop: its calls are qd_rows_geometry and qd_plan_take_fft");
    *n = p->casc ? p->c_complete : p->n_windows;
    return QD_OK;
}

int qd_plan_destroy(qd_plan *p) {
    if (!p) return QD_OK;
    for (qd_plan *c : p->shards) (void)qd_plan_destroy(c);
    p->shards.clear();
    if (p->cmp_a) (void)qd_plan_destroy(p->cmp_a);
    if (p->cmp_b) (void)qd_plan_destroy(p->cmp_b);
    p->cmp_a = p->cmp_b = nullptr;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();
    free_streaming(p);
    for (void *q : {(void *)p->c_h1, (void *)p->c_h2, (void *)p->c_jtab}) if (q) (void)hipFree(q);
    if (p->taps_d) (void)hipFree(p->taps_d);
    if (p->win_own_d) (void)hipFree(p->win_own_d);
    if (p->tw_d) (void)hipFree(p->tw_d);
    if (p->jtab_d) (void)hipFree(p->jtab_d);
    if (p->jtab256_d) (void)hipFree(p->jtab256_d);
    free_rowtab(&p->rows_tab512);
    for (NcoTabs *t : {&p->tabs_dev, &p->tabs_slot[0], &p->tabs_slot[1]}) { free_rowtab(&t->main); free_rowtab(&t->tail); for (RowTab &q : t->phase) free_rowtab(&q); t->phase.clear(); if (t->work) (void)hipFree(t->work); t->work = nullptr; if (t->cmp_tmp) (void)hipFree(t->cmp_tmp); t->cmp_tmp = nullptr; if (t->done) (void)hipEventDestroy(t->done); t->done = nullptr; t->launched = false; }
    if (p->ev_made) { (void)hipEventDestroy(p->ev0); (void)hipEventDestroy(p->ev1); }
    delete p;
    return QD_OK;
}

int qd_plan_get_info(const qd_plan *p, qd_plan_info *info) {
    if (!p || !info) return fail(QD_ERR_INVALID, "plan/info is NULL");
    memset(info, 0, sizeof *info);
    info->n_windows = p->n_windows;
    info->decimated_len = p->dec_len;
    info->out_sample_rate = p->out_rate;
    info->out_bytes_per_window = out_bytes_per_window(p);
    info->raw_per_window = (uint64_t)(p->blk_len ? p->blk_len : p->W) * p->D + p->T;
    info->raw_step = (uint64_t)(p->blk_len ? p->blk_len : p->S) * p->D;
    info->ratio = p->ratio;
    info->tile_windows = p->spark_R > 1 ? p->phase_unit : p->geo.G;
    if (p->cmp_a) {                                   // two-stage plan: the kernel figures are stage A's (the filter)
        qd_plan_info ia;
        const int rc = qd_plan_get_info(p->cmp_a, &ia);
        if (rc) return rc;
        info->threads = ia.threads; info->lds_bytes = ia.lds_bytes; info->kernel_kind = ia.kernel_kind; info->kernel_flags = ia.kernel_flags;
        return QD_OK;
    }
    if (p->casc) {                                    // cascade plan: runtime-geometry kernel, exact arithmetic whatever the mode
        info->threads = kCascadeThreads; info->lds_bytes = (uint32_t)p->c_lds;
        return QD_OK;
    }
    info->threads = (uint32_t)p->launch_nt;
    info->lds_bytes = (uint32_t)(p->geo.lds_main ? p->geo.lds_main : p->geo.lds_bytes);
    info->kernel_kind = p->jit_fn ? 2u : ((p->fixed || p->spark) ? 1u : 0u);
    info->kernel_flags = (p->jit_fn || p->fixed || p->spark) ? p->kflags : 0u;
    info->_reserved = 0;
    return QD_OK;
}

int qd_plan_kernel_name(const qd_plan *p, char *buf, size_t cap) {
    if (!p || !buf || cap == 0) return fail(QD_ERR_INVALID, "plan/buf is NULL");
    if (p->cmp_a) {
        char a[256], b[256];
        (void)qd_plan_kernel_name(p->cmp_a, a, sizeof a); (void)qd_plan_kernel_name(p->cmp_b, b, sizeof b);
        snprintf(buf, cap, "two stages: %s | %s", a, b);
        return QD_OK;
    }
    if (p->casc && p->blk_len) {
        snprintf(buf, cap, "qd::k_cascade_write<%d>(D1 %u, T1 %u, D2 %u, T2 %u, B %u, K %u, shifts %u%u%u, M %u), %u threads, generic", p->d.format,
                 p->c_D1, p->c_T1, p->c_D2, p->c_T2, p->blk_len, p->W, p->c_flags & kCascS0 ? 1 : 0, p->c_flags & kCascS1 ? 1 : 0,
                 p->c_flags & kCascS2 ? 1 : 0, p->c_M, kCascadeThreads);
        return QD_OK;
    }
    if (p->casc) {
        snprintf(buf, cap, "qd::k_cascade<%d>(D1 %u, T1 %u, D2 %u, T2 %u, W %u, S %u, shifts %u%u%u, M %u), %u threads, generic", p->d.format, p->c_D1, p->c_T1,
                 p->c_D2, p->c_T2, p->W, p->S, p->c_flags & kCascS0 ? 1 : 0, p->c_flags & kCascS1 ? 1 : 0, p->c_flags & kCascS2 ? 1 : 0, p->c_M,
                 kCascadeThreads);
        return QD_OK;
    }
    const int fmt = p->d.format;
    if (p->rows) {
        if (p->rows_blue && !p->has_fir) snprintf(buf, cap, "k_bluestein<fmt %d, nco %d>, 256 threads", fmt, p->nco);
        else snprintf(buf, cap, "qd::k_chain<fmt %d, nco %d, RowGeo>, %d rows per workgroup, %d threads, generic%s", fmt, p->nco, (int)p->geo.G, p->launch_nt,
                      p->rows_blue ? " | k_bluestein<fmt 0, nco 0>" : "");
        return QD_OK;
    }
    char geo[160];
    if (p->jit_fn || p->fixed)
        snprintf(geo, sizeof geo, "FixedGeo<%u, %u, %u, %u, %u, ..., %u>", p->W, p->S, p->D, p->T, p->geo.G, p->kflags);
    else snprintf(geo, sizeof geo, (p->d.windowing && p->has_fir) ? "DynGeo with the plan's window (WinGeo)" : "DynGeo");
    snprintf(buf, cap, "%s<fmt %d, nco %d, %s>, %d threads, %s", kFamilies[plan_family(p)].name, fmt, p->nco, geo, p->launch_nt,
             p->jit_fn ? "plan-time build" : (p->fixed || p->spark ? "built-in" : "generic"));
    return QD_OK;
}

int qd_plan_get_taps(const qd_plan *p, float *taps, size_t cap) {
    if (!p || !taps) return fail(QD_ERR_INVALID, "plan/taps is NULL");
    if (p->cmp_a) return qd_plan_get_taps(p->cmp_a, taps, cap);
    if (cap < p->taps_h.size()) return fail(QD_ERR_INVALID, "taps buffer too small");
    if (!p->taps_h.empty()) memcpy(taps, p->taps_h.data(), p->taps_h.size() * sizeof(float));
    return QD_OK;
}

int qd_plan_src_range(const qd_plan *p, uint64_t first_window, uint64_t n_windows, uint64_t *first, uint64_t *count) {
    if (!p || !first || !count) return fail(QD_ERR_INVALID, "NULL argument");
    if (p->rows) return fail(QD_ERR_INVALID, "a QD_EPI_ROWS_F32 plan has no window loop: its calls are qd_rows_geometry and qd_plan_take_fft");
    const uint64_t step = (uint64_t)(p->blk_len ? p->blk_len : p->S) * p->D;
    const uint64_t rpw = (uint64_t)(p->blk_len ? p->blk_len : p->W) * p->D + p->T;
    *first = first_window * step;
    *count = n_windows ? (n_windows - 1) * step + rpw : 0;
    return QD_OK;
}

int qd_plan_set_timing(qd_plan *p, int enabled) {
    if (!p) return fail(QD_ERR_INVALID, "plan is NULL");
    p->timing = enabled != 0;
    if (p->cmp_a) { p->cmp_a->timing = p->timing; p->cmp_b->timing = p->timing; }
    return QD_OK;
}

int qd_plan_last_kernel_ms(qd_plan *p, float *ms) {
    if (!p || !ms) return fail(QD_ERR_INVALID, "NULL argument");
    if (p->cmp_a) {
        float a = 0.f, b = 0.f;
        int rc = qd_plan_last_kernel_ms(p->cmp_a, &a);
        if (rc == QD_OK) rc = qd_plan_last_kernel_ms(p->cmp_b, &b);
        *ms = a + b;
        return rc;
    }
    if (!p->ev_recorded) return fail(QD_ERR_INVALID, "no timed run recorded");
    HIPCHK(hipEventSynchronize(p->ev1));
    HIPCHK(hipEventElapsedTime(ms, p->ev0, p->ev1));
    return QD_OK;
}

namespace {
// Pageable -> pinned staging copy on several host threads: one thread moves ~10-15 GB/s, which would cap the
// host-resident path far below PCIe (qd_plan_options.copy_threads; default: up to 8).
void par_memcpy(void *dst, const void *src, size_t n, unsigned n_thr) {
    if (n_thr == 0) {
        unsigned hw = std::thread::hardware_concurrency();
        n_thr = hw / 2; if (n_thr < 1) n_thr = 1; if (n_thr > 8) n_thr = 8;
    }
    if (n_thr <= 1 || n < (8u << 20)) { memcpy(dst, src, n); return; }
    const size_t slice = ((n / n_thr) + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (unsigned i = 1; i < n_thr; ++i) {
        const size_t off = i * slice;
        if (off >= n) break;
        const size_t len = off + slice > n ? n - off : slice;
        th.emplace_back([=] { memcpy(static_cast<uint8_t *>(dst) + off, static_cast<const uint8_t *>(src) + off, len); });
    }
    memcpy(dst, src, slice < n ? slice : n);
    for (auto &t : th) t.join();
}

double now_ms() {
    timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

bool host_kind(int m) { return m == QD_MEM_HOST || m == QD_MEM_HOST_PINNED; }

// Windows per chunk of a run over windows [first_window, +n_windows): the plan's chunk_bytes at `bytes_per_window`, in whole tiles, and
// for row-aligned kernels in whole periods of the row grid, so that every chunk's launch is the one a whole-range launch would make.
uint64_t chunk_windows(const qd_plan *p, uint64_t first_window, uint64_t n_windows, uint64_t bytes_per_window) {
    const uint64_t step = (uint64_t)p->S * p->D;
    const uint64_t target_bytes = p->opt.chunk_bytes ? p->opt.chunk_bytes : (64ull << 20);
    uint64_t cw = target_bytes / (bytes_per_window ? bytes_per_window : 1);
    if (cw < p->geo.G) cw = p->geo.G;
    cw = (cw / p->geo.G) * p->geo.G;
    if (plan_on_rows(p)) {
        // row-aligned kernels: a launch whose first window is off the row grid goes to the per-sample kernel (launch_chain), so
        // chunks start on windows that are multiples of lcm(G, ROW / gcd(ROW, S D))
        const uint64_t ROW = (uint64_t)p->nt * spl_of(p->d.format);
        const uint64_t wa = ROW / ct_gcd(ROW, step % ROW);              // windows per row-grid period
        uint64_t unit = (uint64_t)p->geo.G / ct_gcd(p->geo.G, wa) * wa; // lcm
        uint64_t grid = wa;
        if (p->spark_R > 1) {                                           // interleaved launches: chunks start where every launch's first window sits on its grid
            unit = unit / ct_gcd(unit, p->phase_unit) * p->phase_unit;
            grid = p->phase_unit;
        }
        if (first_window % grid == 0 && cw >= unit) cw = (cw / unit) * unit;
    }
    // a cascade's write sink: chunks of whole read_at blocks (a sub-block reads past its own window's span, within its block's)
    if (p->casc && p->blk_subs > 1) cw = cw < p->blk_subs ? p->blk_subs : cw / p->blk_subs * p->blk_subs;
    if (cw > n_windows) cw = n_windows ? n_windows : 1;
    return cw;
}

// the host ring's two slots: device buffers of in_bytes / out_bytes each, pinned staging buffers where a side is pageable, a stream per slot
int ensure_ring(qd_plan *p, size_t in_bytes, size_t ob, bool stage_in, bool stage_out) {
    if (in_bytes > p->stage_in_bytes || ob > p->stage_out_bytes || (stage_in && in_bytes > p->pin_in_bytes) || (stage_out && ob > p->pin_out_bytes)) {
        free_streaming(p);
        for (int i = 0; i < 2; ++i) {
            if (stage_in) HIPCHK(hipHostMalloc(&p->pin_in[i], in_bytes, hipHostMallocDefault));
            if (stage_out) HIPCHK(hipHostMalloc(&p->pin_out[i], ob, hipHostMallocDefault));
            HIPCHK(hipMalloc(&p->dev_in[i], in_bytes));
            HIPCHK(hipMalloc(&p->dev_out[i], ob));
            HIPCHK(hipStreamCreateWithFlags(&p->streams[i], hipStreamNonBlocking));
        }
        p->stage_in_bytes = in_bytes; p->stage_out_bytes = ob;
        p->pin_in_bytes = stage_in ? in_bytes : 0; p->pin_out_bytes = stage_out ? ob : 0;
    }
    return QD_OK;
}

// Host-resident stream: windows [first_window, +n_windows) in chunks over the plan's two slots (slot = chunk parity, a stream each).  A chunk's
// slab goes up (a pageable buffer, QD_MEM_HOST, through the slot's pinned staging buffer with a multi-threaded memcpy; QD_MEM_HOST_PINNED
// memory is the DMA source itself) and through the plan's kernel into dev_out[slot]; `chunk` then enqueues, on the slot's stream, whatever
// takes the windows from there.  Each slot owns its device buffers AND its launch context (row tables, a two-stage plan's carrier), so nothing
// a kernel in flight on the other slot reads is ever touched.  Windows are kernel windows (sub-blocks for QD_EPI_CF32_BLOCKS).
struct RingMode {
    uint64_t bytes_per_window;      // what chunk_windows divides chunk_bytes by
    uint64_t obw;                   // bytes per window in dev_out[slot]
    bool stage_out;                 // pinned staging buffers for the way back too
    bool sync_always;               // a slot's chunk is through before the slot is used again; else only when staged, or to bound the queue
    qd_plan_stats *stats;           // bytes_h2d, chunks and the staging time are kept here (may be null)
};
using RingChunk = std::function<int(void *out_d, uint64_t w, uint64_t nw, int slot, hipStream_t st)>;
using RingFreed = std::function<int(int slot)>;        // the slot's stream has been synchronised: finish what its last chunk left
int walk_host(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
              const RingMode &m, const RingChunk &chunk, const RingFreed &freed) {
    const int bps = bps_of(p->d.format);
    const uint64_t step = (uint64_t)p->S * p->D, rpw = (uint64_t)p->W * p->D + p->T;
    const uint64_t cw = chunk_windows(p, first_window, n_windows, m.bytes_per_window);
    const size_t in_bytes = (size_t)(((cw - 1) * step + rpw + 8) * bps);
    const bool stage_in = src_mem == QD_MEM_HOST;
    if (const int rc = ensure_ring(p, in_bytes, (size_t)(cw * m.obw), stage_in, m.stage_out)) return rc;
    // Any error after the first enqueue leaves H2D copies, kernels and D2H copies of earlier chunks in flight — with pinned
    // buffers the D2H target is the CALLER's memory.  Quiesce both slot streams before handing the status back.
    auto quiesce = [&](int status) -> int {
        for (int i = 0; i < 2; ++i) if (p->streams[i]) (void)hipStreamSynchronize(p->streams[i]);
        return status;
    };
    auto release = [&](int slot) -> int {
        if (hipError_t e = hipStreamSynchronize(p->streams[slot]); e != hipSuccess) return fail(QD_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
        return freed ? freed(slot) : QD_OK;
    };
    int slot = 0;
    for (uint64_t w = first_window; w < first_window + n_windows; w += cw, slot ^= 1) {
        // a staged slot's pinned buffers are reused: wait for its previous chunk; a pinned-to-pinned run only needs
        // stream order (same slot = same stream), so the host runs ahead and just bounds the queue depth
        int rc = (m.sync_always || stage_in || m.stage_out || ((w - first_window) / cw) % 16 >= 14) ? release(slot) : QD_OK;
        if (rc) return quiesce(rc);
        const uint64_t nw = std::min<uint64_t>(first_window + n_windows - w, cw);
        const uint64_t s0 = w * step, cnt = (nw - 1) * step + rpw;
        // keep vector loads aligned: start the slab on a multiple of 8 samples
        uint64_t s0a = s0 & ~7ull;
        if (s0a < src_first) s0a = src_first;
        const uint64_t cnta = s0 + cnt - s0a;
        if (s0 < src_first || s0a + cnta > src_first + src_count)
            return quiesce(fail(QD_ERR_INVALID, "src slab does not cover the requested windows"));
        const uint8_t *hsrc = static_cast<const uint8_t *>(src) + (s0a - src_first) * bps;
        if (stage_in) {
            const double t0 = now_ms();
            par_memcpy(p->pin_in[slot], hsrc, cnta * bps, p->opt.copy_threads);
            if (m.stats) m.stats->stage_ms += now_ms() - t0;
            hsrc = static_cast<const uint8_t *>(p->pin_in[slot]);
        }
        if (hipError_t e = hipMemcpyAsync(p->dev_in[slot], hsrc, cnta * bps, hipMemcpyHostToDevice, p->streams[slot]); e != hipSuccess)
            return quiesce(fail(QD_ERR_HIP, "hipMemcpyAsync (H2D): %s", hipGetErrorString(e)));
        rc = launch_windows(p, &p->tabs_slot[slot], p->dev_in[slot], s0a, cnta, w, nw, w, p->dev_out[slot], p->streams[slot]);
        if (rc == QD_OK) rc = chunk(p->dev_out[slot], w, nw, slot, p->streams[slot]);
        if (rc) return quiesce(rc);
        if (m.stats) { m.stats->bytes_h2d += cnta * bps; m.stats->chunks += 1; }
    }
    for (int i = 0; i < 2; ++i)
        if (const int rc = release(i)) return quiesce(rc);
    return QD_OK;
}

// a run: each chunk's windows come back by a D2H copy on the slot's stream, into the caller's pinned memory or, for pageable memory, into
// the slot's pinned buffer, which is copied out once the slot's stream is through
int run_host(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window,
             uint64_t n_windows, void *out, int out_mem, uint64_t obw) {
    const double t_begin = now_ms();
    p->stats = qd_plan_stats{};
    const bool stage_out = out_mem == QD_MEM_HOST;
    struct Pending { bool live = false; uint64_t w0 = 0, nw = 0; } pend[2];
    const int rc = walk_host(p, src, src_mem, src_first, src_count, first_window, n_windows,
        RingMode{(uint64_t)p->S * p->D * bps_of(p->d.format), obw, stage_out, false, &p->stats},
        [&](void *out_d, uint64_t w, uint64_t nw, int slot, hipStream_t st) -> int {
            void *hdst = stage_out ? p->pin_out[slot] : static_cast<void *>(static_cast<uint8_t *>(out) + (w - first_window) * obw);
            if (hipError_t e = hipMemcpyAsync(hdst, out_d, nw * obw, hipMemcpyDeviceToHost, st); e != hipSuccess)
                return fail(QD_ERR_HIP, "hipMemcpyAsync (D2H): %s", hipGetErrorString(e));
            pend[slot].live = true; pend[slot].w0 = w; pend[slot].nw = nw;
            p->stats.bytes_d2h += nw * obw;
            return QD_OK;
        },
        [&](int slot) -> int {
            if (pend[slot].live && stage_out) {
                const double t0 = now_ms();
                par_memcpy(static_cast<uint8_t *>(out) + (pend[slot].w0 - first_window) * obw, p->pin_out[slot], pend[slot].nw * obw, p->opt.copy_threads);
                p->stats.stage_ms += now_ms() - t0;
            }
            pend[slot].live = false;
            return QD_OK;
        });
    if (rc == QD_OK) p->stats.wall_ms = now_ms() - t_begin;
    return rc;
}
}  // namespace

int qd_plan_run(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                uint64_t first_window, uint64_t n_windows, void *out, int out_mem, void *stream) {
    if (!p || !src || !out) return fail(QD_ERR_INVALID, "NULL argument");
    if (p->rows) return fail(QD_ERR_INVALID, "a QD_EPI_ROWS_F32 plan has no window loop: its calls are qd_rows_geometry and qd_plan_take_fft");
    const uint64_t subs = p->blk_subs;          // 1 except QD_EPI_CF32_BLOCKS (API windows are whole blocks)
    if (first_window + n_windows > p->n_windows)
        return fail(QD_ERR_SHORT, "windows [%llu,+%llu) exceed the sink's loop (%llu windows)", (unsigned long long)first_window,
                    (unsigned long long)n_windows, (unsigned long long)p->n_windows);
    if (src_first + src_count > p->d.n_samples) return fail(QD_ERR_INVALID, "src slab exceeds the stream length");
    if (p->casc && first_window + n_windows > p->c_complete) {
        // a cascade's last windows may fail read_exact_at (LowPass::len over-reports, src/filter.rs:45-48): every complete window
        // of the range is written, then the run reports the short read
        const uint64_t done = first_window < p->c_complete ? p->c_complete - first_window : 0;
        int rc = done ? qd_plan_run(p, src, src_mem, src_first, src_count, first_window, done, out, out_mem, stream) : QD_OK;
        if (rc) return rc;
        return fail(QD_ERR_SHORT, "window %llu: read_exact_at reads fewer samples than asked (%llu complete windows of %llu)",
                    (unsigned long long)p->c_complete, (unsigned long long)p->c_complete, (unsigned long long)p->n_windows);
    }
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard guard(p->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (src_mem == QD_MEM_DEVICE && out_mem == QD_MEM_DEVICE)
        return launch_windows(p, &p->tabs_dev, src, src_first, src_count, first_window * subs, n_windows * subs, first_window * subs, out, st);
    if (!host_kind(src_mem) || !host_kind(out_mem))
        return fail(QD_ERR_UNSUPPORTED, "mixed host/device buffers are not supported; use both host or both device");
    const uint64_t obw = out_bytes_per_window(p) / subs;      // per kernel window (a sub-block for QD_EPI_CF32_BLOCKS)
    return run_host(p, src, src_mem, src_first, src_count, first_window * subs, n_windows * subs, out, out_mem, obw);
}

int qd_plan_get_stats(const qd_plan *p, qd_plan_stats *stats) {
    if (!p || !stats) return fail(QD_ERR_INVALID, "NULL argument");
    *stats = p->stats;
    return QD_OK;
}

int qd_plan_shard_info(const qd_plan *p, uint32_t shard, qd_shard_info *info) {
    if (!p || !info) return fail(QD_ERR_INVALID, "NULL argument");
    if (shard >= p->shard_info.size()) return fail(QD_ERR_INVALID, "shard %u of %zu", shard, p->shard_info.size());
    *info = p->shard_info[shard];
    return QD_OK;
}

int qd_plan_run_sharded(qd_plan *p, const void *src, int src_mem, void *out, int out_mem) {
    if (!p || !src || !out) return fail(QD_ERR_INVALID, "NULL argument");
    if (!host_kind(src_mem) || !host_kind(out_mem)) return fail(QD_ERR_INVALID, "qd_plan_run_sharded takes host buffers (QD_MEM_HOST / QD_MEM_HOST_PINNED)");
    if (p->shards.empty()) return qd_plan_run(p, src, src_mem, 0, p->d.n_samples, 0, p->n_windows, out, out_mem, nullptr);
    // one host thread per shard: each drives its device's double-buffered ring; every shard reads its windows' source
    // range — halo included — straight from the host buffer, so there is no exchange step at all
    const uint64_t obw_api = out_bytes_per_window(p);
    const size_t n = p->shards.size();
    std::vector<int> rcs(n, QD_OK);
    std::vector<std::string> errs(n);
    std::vector<std::thread> th;
    for (size_t g = 0; g < n; ++g) {
        th.emplace_back([&, g] {
            const qd_shard_info &si = p->shard_info[g];
            if (si.w1 == si.w0) return;
            rcs[g] = qd_plan_run(p->shards[g], src, src_mem, 0, p->d.n_samples, si.w0, si.w1 - si.w0,
                                 static_cast<uint8_t *>(out) + si.w0 * obw_api, out_mem, nullptr);
            if (rcs[g]) errs[g] = g_err;         // thread-local message of the worker
        });
    }
    for (auto &t : th) t.join();
    p->stats = qd_plan_stats{};
    for (size_t g = 0; g < n; ++g) {
        if (rcs[g]) return fail(rcs[g], "shard %zu (device %d): %s", g, p->shard_info[g].device, errs[g].c_str());
        const qd_plan_stats &cs = p->shards[g]->stats;
        p->stats.wall_ms = std::max(p->stats.wall_ms, cs.wall_ms); p->stats.stage_ms += cs.stage_ms;
        p->stats.bytes_h2d += cs.bytes_h2d; p->stats.bytes_d2h += cs.bytes_d2h; p->stats.chunks += cs.chunks;
    }
    return QD_OK;
}

int qd_plan_run_sharded_device(qd_plan *p, void *const *slabs, void *const *outs, int sync) {
    if (!p || !slabs || !outs) return fail(QD_ERR_INVALID, "NULL argument");
    if (p->cmp_a) return fail(QD_ERR_UNSUPPORTED, "a two-stage plan (window larger than the LDS tile) has no pre-split device path");
    if (p->casc) return fail(QD_ERR_UNSUPPORTED, "a cascade plan (qd_plan_create_stages) has no pre-split device path");
    if (p->rows) return fail(QD_ERR_INVALID, "a QD_EPI_ROWS_F32 plan has no window loop: its calls are qd_rows_geometry and qd_plan_take_fft");
    const size_t n = p->shard_info.size();
    const int bps = bps_of(p->d.format);
    std::vector<qd_plan *> plans(n, p);
    for (size_t g = 0; g < n && !p->shards.empty(); ++g) plans[g] = p->shards[g];
    for (size_t g = 0; g < n; ++g) {
        const qd_shard_info &si = p->shard_info[g];
        if (si.w1 == si.w0) continue;
        if (!slabs[g] || !outs[g]) return fail(QD_ERR_INVALID, "shard %zu: NULL slab / out", g);
        if (si.halo && (g + 1 >= n || p->shard_info[g + 1].own_count < si.halo))
            return fail(QD_ERR_INVALID, "shard %zu needs a %llu-sample halo its neighbour does not own: use fewer shards", g, (unsigned long long)si.halo);
    }
    for (size_t g = 0; g < n; ++g) {
        const qd_shard_info &si = p->shard_info[g];
        if (si.w1 == si.w0) continue;
        qd_plan *c = plans[g];
        std::lock_guard<std::mutex> lock(c->mu);
        DeviceGuard guard(si.device);
        if (!c->streams[0]) HIPCHK(hipStreamCreateWithFlags(&c->streams[0], hipStreamNonBlocking));
        if (si.halo)     // the one exchange step of a pre-split device-resident stream: (W-S)*D+T samples from the next slab
            HIPCHK(hipMemcpyPeerAsync(static_cast<uint8_t *>(slabs[g]) + si.own_count * bps, si.device, slabs[g + 1],
                                      p->shard_info[g + 1].device, si.halo * bps, c->streams[0]));
        const uint64_t subs = c->blk_subs;
        int rc = launch_windows(c, &c->tabs_dev, slabs[g], si.own_first, si.own_count + si.halo, si.w0 * subs, (si.w1 - si.w0) * subs,
                              si.w0 * subs, outs[g], c->streams[0]);
        if (rc) return rc;
    }
    if (sync) {
        for (size_t g = 0; g < n; ++g) {
            if (p->shard_info[g].w1 == p->shard_info[g].w0 || !plans[g]->streams[0]) continue;
            DeviceGuard guard(p->shard_info[g].device);
            HIPCHK(hipStreamSynchronize(plans[g]->streams[0]));
        }
    }
    return QD_OK;
}

int qd_host_alloc(size_t bytes, void **ptr) {
    if (!ptr) return fail(QD_ERR_INVALID, "NULL argument");
    *ptr = nullptr;
    if (bytes == 0) return QD_OK;
    HIPCHK(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    return QD_OK;
}
int qd_host_free(void *ptr) { if (ptr) HIPCHK(hipHostFree(ptr)); return QD_OK; }
int qd_host_register(void *ptr, size_t bytes) {
    if (!ptr || !bytes) return fail(QD_ERR_INVALID, "NULL / empty range");
    HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return QD_OK;
}
int qd_host_unregister(void *ptr) { if (ptr) HIPCHK(hipHostUnregister(ptr)); return QD_OK; }

// ------------------------------------------------------------------ fine-grained ops
//
// These mirror one `read_at` each, so a host may call them once per window: no hipMalloc /
// hipFree / plan construction per call.  Device temporaries come from a process-wide pool of grow-only workspaces; a
// workspace is handed to one call at a time and remembers the stream that used it last, so reuse on the same stream
// needs no synchronisation (stream order) and reuse on another stream waits for the old one first.  The FFT-based
// calls keep their plans in a small cache.  All launches go to the calling thread's stream (qd_set_stream).

namespace {

thread_local hipStream_t g_stream = nullptr;

struct Workspace {
    static constexpr int kSlots = 6;
    void *buf[kSlots] = {};
    size_t cap[kSlots] = {};
    int device = 0;
    hipStream_t last = nullptr;          // compared, never dereferenced: the caller may have destroyed it since
    hipEvent_t done = nullptr;           // recorded behind the last call that used the buffers
    bool used = false;
    int get(int i, size_t bytes, void **out) {
        if (bytes > cap[i]) {
            if (buf[i]) {
                if (used && done) HIPCHK(hipEventSynchronize(done));      // earlier calls; this call has not touched slot i yet
                HIPCHK(hipFree(buf[i]));
                buf[i] = nullptr; cap[i] = 0;
            }
            const size_t want = (bytes + bytes / 4 + 4095) & ~(size_t)4095;
            HIPCHK(hipMalloc(&buf[i], want));
            cap[i] = want;
        }
        *out = buf[i];
        return QD_OK;
    }
    void release_buffers() {
        for (int i = 0; i < kSlots; ++i) { if (buf[i]) (void)hipFree(buf[i]); buf[i] = nullptr; cap[i] = 0; }
        if (done) (void)hipEventDestroy(done);
        done = nullptr;
    }
};

std::mutex g_ws_mu;
std::vector<Workspace *> g_ws_idle;

struct WsLease {                        // one workspace for the duration of a call
    Workspace *ws = nullptr;
    hipStream_t st_ = nullptr;
    int rc = QD_OK;
    explicit WsLease(hipStream_t st) : st_(st) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> lock(g_ws_mu);
            size_t pick = g_ws_idle.size();
            for (size_t i = 0; i < g_ws_idle.size(); ++i) {
                if (g_ws_idle[i]->device != dev) continue;
                if (pick == g_ws_idle.size() || g_ws_idle[i]->last == st) pick = i;
                if (g_ws_idle[i]->last == st) break;
            }
            if (pick < g_ws_idle.size()) { ws = g_ws_idle[pick]; g_ws_idle.erase(g_ws_idle.begin() + pick); }
        }
        if (!ws) { ws = new Workspace(); ws->device = dev; }
        // hand-over between streams: the new stream waits (on the device) for the event behind the workspace's last call
        // (always: `last` is kept to prefer a workspace this stream used, never to skip the wait — a handle may be a new stream at a recycled address)
        if (ws->used && ws->done && hipStreamWaitEvent(st, ws->done, 0) != hipSuccess) rc = fail(QD_ERR_HIP, "workspace hand-over: hipStreamWaitEvent failed");
        if (!ws->done && hipEventCreateWithFlags(&ws->done, hipEventDisableTiming) != hipSuccess) { ws->done = nullptr; rc = fail(QD_ERR_HIP, "workspace: hipEventCreate failed"); }
        ws->last = st; ws->used = true;
    }
    ~WsLease() {
        if (ws->done) (void)hipEventRecord(ws->done, st_);         // whatever this call enqueued (also on an error return)
        std::lock_guard<std::mutex> lock(g_ws_mu);
        g_ws_idle.push_back(ws);
    }
    int get(int i, size_t bytes, void **out) { return ws->get(i, bytes, out); }
};

// plans of the FFT-based fine-grained calls, keyed by (device, width, stride, kind)
// Entries are handed out as shared_ptr: an eviction (cache full) or qd_release_workspaces only drops the CACHE's reference,
// the plan is destroyed when the last caller still using it lets go — nobody locks a freed mutex or launches on a freed plan.
struct CachedPlan {
    int device; uint64_t W, S; int kind; qd_plan *plan; std::mutex mu;
    CachedPlan(int dev, uint64_t w, uint64_t s, int k, qd_plan *p) : device(dev), W(w), S(s), kind(k), plan(p) {}
    ~CachedPlan() { if (plan) { DeviceGuard guard(device); (void)qd_plan_destroy(plan); } }
};
std::mutex g_pc_mu;
std::vector<std::shared_ptr<CachedPlan>> g_plan_cache;
constexpr size_t kPlanCacheMax = 32;
constexpr uint64_t kOpenEnded = 1ull << 40;      // "any number of windows": the cached plans size no loop from it

int cached_fft_plan(uint64_t W, uint64_t S, int kind, std::shared_ptr<CachedPlan> *out) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_pc_mu);
    for (const std::shared_ptr<CachedPlan> &c : g_plan_cache)
        if (c->device == dev && c->W == W && c->S == S && c->kind == kind) { *out = c; return QD_OK; }
    qd_chain_desc d{};
    d.struct_size = sizeof d;
    d.format = QD_FMT_CF32; d.sample_rate = 1;
    d.n_samples = kOpenEnded;
    d.width = W; d.stride = S; d.epilogue = QD_EPI_NORMS_F32;
    qd_plan_options o{};
    o.struct_size = sizeof o;
    o.kernel_policy = QD_KERNEL_NO_PLAN_TIME;      // a per-window helper must not stall on a compile
    qd_plan *p = nullptr;
    int rc = qd_plan_create_ex(&d, &o, &p);
    if (rc) return rc;
    if (kind == 1) {                               // take_fft: one irregular row per tile, per-sample (unaligned) kernel
        p->geo.G = 1;
        uint32_t raw_elems = 0;
        p->geo.lds_bytes = lds_for(1, p->W, p->S, p->D, p->T, &raw_elems, 1, 1, false);
        p->geo.lds_main = p->geo.lds_bytes;
        p->geo.lds_raw_elems = raw_elems;
        p->fn = p->fn_unaligned;
        p->spark = false; p->kflags = 0;           // irregular rows: the per-sample generic kernel only
    }
    if (g_plan_cache.size() >= kPlanCacheMax) g_plan_cache.erase(g_plan_cache.begin());     // the oldest entry; destroyed once unused
    g_plan_cache.push_back(std::make_shared<CachedPlan>(dev, W, S, kind, p));
    *out = g_plan_cache.back();
    return QD_OK;
}

// ---- Bluestein tables per width (host f64 arithmetic, rounded once to f32), cached per device
struct BluesteinTab {
    int device = 0; uint32_t W = 0, M = 0, logM = 0; double2 *chirp = nullptr, *Bbr = nullptr, *tw = nullptr;
    BluesteinTab() = default;
    BluesteinTab(const BluesteinTab &) = delete;
    BluesteinTab &operator=(const BluesteinTab &) = delete;
    // hipFree waits for the device: a kernel still reading the tables (its caller has already let go) finishes first
    ~BluesteinTab() { DeviceGuard guard(device); if (chirp) (void)hipFree(chirp); if (Bbr) (void)hipFree(Bbr); if (tw) (void)hipFree(tw); }
};
std::mutex g_bt_mu;
std::vector<std::shared_ptr<BluesteinTab>> g_bt;       // by reference count, like the plan cache: eviction never frees under a caller

void fft64_inplace(std::vector<double> &re, std::vector<double> &im, uint32_t logM) {   // radix-2 DIT, natural order out
    const uint32_t M = 1u << logM;
    for (uint32_t i = 0; i < M; ++i) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < logM; ++b) if (i & (1u << b)) r |= 1u << (logM - 1 - b);
        if (r > i) { std::swap(re[i], re[r]); std::swap(im[i], im[r]); }
    }
    for (uint32_t h = 1; h < M; h <<= 1) {
        for (uint32_t j = 0; j < h; ++j) {
            const double ang = -kPi64 * (double)j / (double)h, wr = std::cos(ang), wi = std::sin(ang);
            for (uint32_t i = j; i < M; i += 2 * h) {
                const double vr = re[i + h] * wr - im[i + h] * wi, vi = re[i + h] * wi + im[i + h] * wr;
                re[i + h] = re[i] - vr; im[i + h] = im[i] - vi;
                re[i] += vr; im[i] += vi;
            }
        }
    }
}

int bluestein_tab(uint32_t W, std::shared_ptr<BluesteinTab> *out) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_bt_mu);
    for (const std::shared_ptr<BluesteinTab> &e : g_bt) if (e->device == dev && e->W == W) { *out = e; return QD_OK; }
    std::shared_ptr<BluesteinTab> tp = std::make_shared<BluesteinTab>();
    BluesteinTab &t = *tp;
    t.device = dev; t.W = W;
    t.logM = ilog2(2ull * W - 1); t.M = 1u << t.logM;
    const uint32_t M = t.M;
    std::vector<double2> chirp(W), Bbr(M), tw(M / 2 ? M / 2 : 1);
    std::vector<double> br(M, 0.0), bi(M, 0.0);
    for (uint32_t n = 0; n < W; ++n) {
        const uint64_t q = ((uint64_t)n * n) % (2ull * W);       // n^2 mod 2W: the angle is reduced exactly, in integers
        const double ang = kPi64 * (double)q / (double)W;
        const double cr = std::cos(ang), ci = std::sin(ang);     // b[n] = e^{+i pi n^2 / W}
        chirp[n] = make_double2(cr, -ci);                         // c[n] = conj(b[n])
        br[n] = cr; bi[n] = ci;
        if (n) { br[M - n] = cr; bi[M - n] = ci; }
    }
    fft64_inplace(br, bi, t.logM);
    for (uint32_t r = 0; r < M; ++r) {
        uint32_t k = 0;
        for (uint32_t b = 0; b < t.logM; ++b) if (r & (1u << b)) k |= 1u << (t.logM - 1 - b);
        Bbr[r] = make_double2(br[k] / (double)M, bi[k] / (double)M);
    }
    for (uint32_t k = 0; k < M / 2; ++k) {
        const double ang = -2.0 * kPi64 * (double)k / (double)M;
        tw[k] = make_double2(std::cos(ang), std::sin(ang));
    }
    if (M / 2 == 0) tw[0] = make_double2(1.0, 0.0);
    HIPCHK(hipMalloc(&t.chirp, chirp.size() * 16)); HIPCHK(hipMalloc(&t.Bbr, Bbr.size() * 16)); HIPCHK(hipMalloc(&t.tw, tw.size() * 16));
    HIPCHK(hipMemcpy(t.chirp, chirp.data(), chirp.size() * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.Bbr, Bbr.data(), Bbr.size() * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.tw, tw.data(), tw.size() * 16, hipMemcpyHostToDevice));
    if (g_bt.size() >= 64) g_bt.erase(g_bt.begin());               // the width slider walks through many lengths: bound the cache
    g_bt.push_back(tp);
    *out = tp;
    return QD_OK;
}

// rows at offs_d[] (source sample indices) of a slab; fmt / nco / src's NCO tables: the loader (cf32 without a shift: qd_take_fft's)
int bluestein_rows(int fmt, int nco, const BlueSrc &src, const uint64_t *offs_d, const float *win_d, size_t W, size_t n_rows,
                   float *dst, hipStream_t st) {
    if (W > 4096) return fail(QD_ERR_UNSUPPORTED, "take_fft width %zu: widths that are not a power of two are built up to 4096 (the reference front end's slider range, src/eui/mod.rs:157)", W);
    std::shared_ptr<BluesteinTab> tp;                  // held until the launch is enqueued
    int rc = bluestein_tab((uint32_t)W, &tp);
    if (rc) return rc;
    const BluesteinTab &t = *tp;
    const blue_fn fn = pick_blue(fmt, nco);
    if (!fn) return fail(QD_ERR_UNSUPPORTED, "no kernel built for this format (QD_DEV_FAST build?)");
    if ((size_t)t.M * 16 > 48 * 1024)     // per device, cheap: raise the dynamic-LDS limit to the hardware maximum
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    hipLaunchKernelGGL(fn, dim3((uint32_t)n_rows), dim3(256), (size_t)t.M * 16, st, src, offs_d, win_d, (uint32_t)W, t.M, t.logM,
                       t.chirp, t.Bbr, t.tw, dst);
    HIPCHK(hipGetLastError());
    return QD_OK;
}

int finish_call(int mem, hipStream_t st) {         // host buffers: results must be there on return
    if (mem != QD_MEM_DEVICE) HIPCHK(hipStreamSynchronize(st));
    return QD_OK;
}

}  // namespace

int qd_set_stream(void *stream) { g_stream = static_cast<hipStream_t>(stream); return QD_OK; }

int qd_release_workspaces(void) {
    {
        std::lock_guard<std::mutex> lock(g_ws_mu);
        for (Workspace *w : g_ws_idle) {
            DeviceGuard guard(w->device);
            if (w->used && w->done) (void)hipEventSynchronize(w->done);
            w->release_buffers();
            delete w;
        }
        g_ws_idle.clear();
    }
    std::vector<std::shared_ptr<CachedPlan>> dropped;
    {
        std::lock_guard<std::mutex> lock(g_pc_mu);
        dropped.swap(g_plan_cache);
    }
    dropped.clear();                               // plans nobody is running are destroyed here, the others when their call returns
    {
        std::lock_guard<std::mutex> lock(g_bt_mu);
        g_bt.clear();
    }
    return QD_OK;
}

int qd_unpack(int fmt, const void *bytes, size_t n_pairs, qd_c32 *out, int mem) {
    if (fmt < 0 || fmt > 3) return fail(QD_ERR_INVALID, "unknown format %d", fmt);
    if (n_pairs == 0) return QD_OK;
    if (!bytes || !out) return fail(QD_ERR_INVALID, "NULL buffer");
    const size_t ib = n_pairs * qd_pair_bytes(fmt), ob = n_pairs * 8;
    const hipStream_t st = g_stream;
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    const void *src = bytes; void *dst = out;
    if (mem != QD_MEM_DEVICE) {
        void *di = nullptr, *dout = nullptr;
        int rc = ws.get(0, ib, &di); if (rc) return rc;
        rc = ws.get(1, ob, &dout); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(di, bytes, ib, hipMemcpyHostToDevice, st));
        src = di; dst = dout;
    }
    size_t blocks = (n_pairs + 255) / 256; if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_unpack, dim3((uint32_t)blocks), dim3(256), 0, st, fmt, static_cast<const uint8_t *>(src), n_pairs,
                       static_cast<float2 *>(dst));
    HIPCHK(hipGetLastError());
    if (mem != QD_MEM_DEVICE) HIPCHK(hipMemcpyAsync(out, dst, ob, hipMemcpyDeviceToHost, st));
    return finish_call(mem, st);
}

int qd_shift(qd_c32 *buf, size_t n, uint64_t abs_off, double ratio, int mem) {
    if (n == 0) return QD_OK;
    if (!buf) return fail(QD_ERR_INVALID, "NULL buffer");
    constexpr uint32_t ROW = 512;
    const hipStream_t st = g_stream;
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    float2 *d = reinterpret_cast<float2 *>(buf);
    if (mem != QD_MEM_DEVICE) {
        void *db = nullptr;
        int rc = ws.get(0, n * 8, &db); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(db, buf, n * 8, hipMemcpyHostToDevice, st));
        d = static_cast<float2 *>(db);
    }
    const uint64_t r0 = abs_off / ROW, r1 = (abs_off + n + ROW - 1) / ROW, rows = r1 - r0;
    void *rt = nullptr, *jt = nullptr;
    int rc = ws.get(2, rows * sizeof(RowBase), &rt); if (rc) return rc;
    rc = ws.get(3, ROW * sizeof(LaneEntry), &jt); if (rc) return rc;
    hipLaunchKernelGGL(k_rowtab, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, st, ratio, ROW, r0, rows, (uint64_t)0, static_cast<RowBase *>(rt));
    hipLaunchKernelGGL(k_jtab, dim3(2), dim3(256), 0, st, ratio, ROW, static_cast<LaneEntry *>(jt));
    const int so = (std::fabs(ratio) * (double)(abs_off + n) > 268435456.0) ? 1 : 0;
    const uint32_t grid = (uint32_t)(rows < 4096 ? rows : 4096);
    hipLaunchKernelGGL(k_shift, dim3(grid), dim3(256), 0, st, d, abs_off, (uint64_t)n, ratio, static_cast<const RowBase *>(rt), r0, rows,
                       static_cast<const LaneEntry *>(jt), so);
    HIPCHK(hipGetLastError());
    if (mem != QD_MEM_DEVICE) HIPCHK(hipMemcpyAsync(buf, d, n * 8, hipMemcpyDeviceToHost, st));
    return finish_call(mem, st);
}

int qd_lowpass_block(const float *taps, size_t T, uint64_t D, const qd_c32 *raw, size_t valid, qd_c32 *out,
                     size_t out_cap, size_t *produced, int mem) {
    if (!taps || !raw || !out || !produced) return fail(QD_ERR_INVALID, "NULL argument");
    if (T < 2 || D == 0) return fail(QD_ERR_PANIC, "size < 2 or decimate 0 (src/filter.rs:47,74)");
    if (valid < T) return fail(QD_ERR_PANIC, "valid < filter.len(): usize underflow at src/filter.rs:76");
    size_t out_n = (size_t)((uint64_t)(valid - T) / D);
    if (out_n > out_cap) return fail(QD_ERR_PANIC, "buf too small for %zu outputs (src/filter.rs:78-80)", out_n);
    *produced = out_n;
    if (out_n == 0) return QD_OK;
    const hipStream_t st = g_stream;
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    void *dt = nullptr;
    int rc = ws.get(2, T * 4, &dt); if (rc) return rc;
    // taps are always host memory (O(T)); the caller may reuse its array at once, so this small copy is synchronous
    HIPCHK(hipMemcpyAsync(dt, taps, T * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    const float2 *r = reinterpret_cast<const float2 *>(raw);
    float2 *o = reinterpret_cast<float2 *>(out);
    if (mem != QD_MEM_DEVICE) {
        void *dr = nullptr, *dout = nullptr;
        rc = ws.get(0, valid * 8, &dr); if (rc) return rc;
        rc = ws.get(1, out_n * 8, &dout); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(dr, raw, valid * 8, hipMemcpyHostToDevice, st));
        r = static_cast<const float2 *>(dr); o = static_cast<float2 *>(dout);
    }
    size_t blocks = (out_n + 127) / 128; if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_lowpass_block, dim3((uint32_t)blocks), dim3(128), 0, st, static_cast<const float *>(dt), (uint32_t)T, D, r,
                       (uint64_t)valid, o, (uint64_t)out_n);
    HIPCHK(hipGetLastError());
    if (mem != QD_MEM_DEVICE) HIPCHK(hipMemcpyAsync(out, o, out_n * 8, hipMemcpyDeviceToHost, st));
    return finish_call(mem, st);
}

int qd_fft_norm_batch(const qd_c32 *in, size_t W, size_t n_fft, size_t in_stride, float *norms, int mem) {
    if (n_fft == 0) return QD_OK;
    if (!in || !norms) return fail(QD_ERR_INVALID, "NULL buffer");
    if (in_stride == 0) return fail(QD_ERR_INVALID, "in_stride 0");
    if (!is_pow2(W)) return fail(QD_ERR_PANIC, "Radix4 requires a power-of-two width (rustfft API contract), got %zu", W);
    std::shared_ptr<CachedPlan> c;
    int rc = cached_fft_plan(W, in_stride, 0, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(c->mu);
    qd_plan *p = c->plan;
    const hipStream_t st = g_stream;
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    const uint64_t have = (uint64_t)(n_fft - 1) * in_stride + W;
    const void *src = in; void *dst = norms;
    if (mem != QD_MEM_DEVICE) {
        void *di = nullptr, *dout = nullptr;
        rc = ws.get(0, have * 8, &di); if (rc) return rc;
        rc = ws.get(1, n_fft * W * 4, &dout); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(di, in, have * 8, hipMemcpyHostToDevice, st));
        src = di; dst = dout;
    }
    rc = launch_windows(p, &p->tabs_dev, src, 0, have, 0, n_fft, 0, dst, st);
    if (rc) return rc;
    if (mem != QD_MEM_DEVICE) HIPCHK(hipMemcpyAsync(norms, dst, n_fft * W * 4, hipMemcpyDeviceToHost, st));
    return finish_call(mem, st);
}

int qd_take_fft(const qd_c32 *in, uint64_t in_first, size_t n_in, uint64_t samples_len, int has_slice,
                uint64_t start, uint64_t end, size_t W, int windowing, size_t output_len, float *rows, int mem) {
    if (!in || !rows) return fail(QD_ERR_INVALID, "NULL buffer");
    if (W < 1 || W > (1u << 20)) return fail(QD_ERR_UNSUPPORTED, "take_fft width %zu", W);
    if (const int rcs = rows_slice(samples_len, W, has_slice, &start, &end, output_len)) return rcs;
    if (output_len == 0) return QD_OK;
    std::vector<uint64_t> offs(output_len);
    for (size_t i = 0; i < output_len; ++i) {
        offs[i] = rows_offset(start, end, output_len, i);
        if (offs[i] < in_first || offs[i] + W > in_first + n_in || offs[i] + W > samples_len)
            return fail(QD_ERR_SHORT, "row %zu at sample %llu is not inside the provided block / the stream (read_exact_at, src/ffts.rs:62)", i, (unsigned long long)offs[i]);
    }
    std::vector<float> win;
    if (windowing == 1) blackman_harris(W, &win);
    const hipStream_t st = g_stream;
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    void *doffs = nullptr, *dwin = nullptr;
    int rc = ws.get(2, output_len * 8, &doffs); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(doffs, offs.data(), output_len * 8, hipMemcpyHostToDevice, st));
    if (!win.empty()) {
        rc = ws.get(3, W * 4, &dwin); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(dwin, win.data(), W * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));               // offs / win are locals of this call
    const void *src = in; void *dst = rows;
    if (mem != QD_MEM_DEVICE) {
        void *di = nullptr, *dout = nullptr;
        rc = ws.get(0, n_in * 8, &di); if (rc) return rc;
        rc = ws.get(1, output_len * W * 4, &dout); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(di, in, n_in * 8, hipMemcpyHostToDevice, st));
        src = di; dst = dout;
    }
    if (is_pow2(W)) {
        // rustfft's planner gives a power-of-two length to its Radix4 as well: the chain kernel's FFT (bit-exact against
        // the oracle's own copy), rows gathered at irregular offsets by the per-sample kernel
        std::shared_ptr<CachedPlan> c;
        rc = cached_fft_plan(W, W, 1, &c);
        if (rc) return rc;
        std::lock_guard<std::mutex> lock(c->mu);
        qd_plan *p = c->plan;
        p->row_offsets_d = static_cast<const uint64_t *>(doffs);
        p->window_d = static_cast<const float *>(dwin);
        p->d.n_samples = in_first + n_in;
        rc = launch_windows(p, &p->tabs_dev, src, in_first, n_in, 0, output_len, 0, dst, st);
        p->row_offsets_d = nullptr; p->window_d = nullptr;
    } else {
        BlueSrc bs{};
        bs.in = static_cast<const uint8_t *>(src); bs.in_first = in_first;
        rc = bluestein_rows(QD_FMT_CF32, 0, bs, static_cast<const uint64_t *>(doffs), static_cast<const float *>(dwin),
                            W, output_len, static_cast<float *>(dst), st);
    }
    if (rc) return rc;
    if (mem != QD_MEM_DEVICE) HIPCHK(hipMemcpyAsync(rows, dst, output_len * W * 4, hipMemcpyDeviceToHost, st));
    return finish_call(mem, st);
}

namespace {
// the chain of a one-stage description as stages_geo sees it (validation with the plan's codes), sink = QD_EPI_ROWS_F32
int rows_chain_geo(const qd_chain_desc *desc, StageGeo *g) {
    if (!desc) return fail(QD_ERR_INVALID, "desc is NULL");
    if (desc->struct_size != sizeof(qd_chain_desc)) return fail(QD_ERR_INVALID, "qd_chain_desc size mismatch");
    qd_chain_desc d = *desc;
    qd_stage st[2] = {};
    size_t n = 0;
    if (d.has_shift) { st[n].kind = QD_STAGE_SHIFT; st[n++].shift_hz = d.shift_hz; }
    if (d.has_lowpass) { st[n].kind = QD_STAGE_LOWPASS; st[n].lowpass_hz = d.lowpass_hz; st[n].decimate = d.decimate; st[n++].taps = d.taps; }
    d.has_shift = d.has_lowpass = 0; d.epilogue = QD_EPI_ROWS_F32;
    return stages_geo(&d, st, n, g);
}

// slice rules, row offsets (the sink's samples) and the rows' source range [*lo, *hi); a row whose read_exact_at fails: QD_ERR_SHORT
int rows_layout(uint64_t n_samples, uint64_t len, uint64_t W, uint64_t D, uint64_t T, const qd_rows_desc *r, std::vector<uint64_t> *offs,
                uint64_t *lo, uint64_t *hi) {
    if (!r) return fail(QD_ERR_INVALID, "rows is NULL");
    if (r->struct_size != sizeof(qd_rows_desc)) return fail(QD_ERR_INVALID, "qd_rows_desc size mismatch");
    if (r->windowing != 0 && r->windowing != 1) return fail(QD_ERR_INVALID, "unknown windowing %d", r->windowing);
    uint64_t start = r->start, end = r->end;
    if (const int rc = rows_slice(len, W, r->has_slice, &start, &end, r->output_len)) return rc;
    if (r->output_len > (1ull << 32)) return fail(QD_ERR_UNSUPPORTED, "output_len too large");
    offs->resize(r->output_len);
    const uint64_t span = W * D + T;
    *lo = UINT64_MAX; *hi = 0;
    for (uint64_t i = 0; i < r->output_len; ++i) {
        const uint64_t o = rows_offset(start, end, r->output_len, i);
        (*offs)[i] = o;
        if (o > (UINT64_MAX - span) / D || o * D + span > n_samples)
            return fail(QD_ERR_SHORT, "row %llu at sample %llu reads source samples [%llu, +%llu) past the stream's %llu (read_exact_at, src/ffts.rs:62)",
                        (unsigned long long)i, (unsigned long long)o, (unsigned long long)(o * D), (unsigned long long)span, (unsigned long long)n_samples);
        *lo = std::min(*lo, o * D); *hi = std::max(*hi, o * D + span);
    }
    if (r->output_len == 0) *lo = *hi = 0;
    return QD_OK;
}

// G rows per workgroup of the row-mode kernel over a device slab: rows at source samples srcoffs_d[], epilogue `epi` (norms / cf32)
int launch_rows(qd_plan *p, const void *src_d, uint64_t src_first, uint64_t src_count, const uint64_t *srcoffs_d, const float *win_d,
                uint64_t n_rows, uint64_t lo, uint64_t hi, void *out_d, uint32_t epi, hipStream_t st) {
    NcoTabs *ctx = &p->tabs_dev;
    if (!ctx->done) HIPCHK(hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming));
    if (ctx->launched) HIPCHK(hipStreamWaitEvent(st, ctx->done, 0));          // the launch-context protocol of launch_windows
    int rc = QD_OK;
    if (p->has_shift) rc = ensure_rowtab_for(p, kThreads * spl_of(p->d.format), &ctx->main, lo, hi, st);
    if (rc == QD_OK) {
        ChainParams P{};
        plan_params(p, &P);
        P.src = static_cast<const uint8_t *>(src_d);
        P.src_first = src_first; P.src_count = src_count;
        P.first_window = 0; P.n_windows = n_rows; P.out_window0 = 0;
        P.rowtab = ctx->main.d; P.rowtab_row0 = ctx->main.row0;
        P.out = out_d;
        P.epi = epi;
        P.row_offsets = srcoffs_d; P.window = win_d;
        P.blk_len = p->blk_len; P.blk_sub_mask = 0; P.tile_extra = 0;
        P.work = nullptr;
        P.lds_dyn = (uint32_t)p->geo.lds_bytes;
        const uint64_t n_tiles = (n_rows + P.G - 1) / P.G, cap = (uint64_t)p->n_cu * p->wg_per_cu;
        hipLaunchKernelGGL(p->fn, dim3((uint32_t)(n_tiles < cap ? n_tiles : cap)), dim3(kThreads), p->geo.lds_bytes, st, P);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) rc = fail(QD_ERR_HIP, "row-mode launch -> %s", hipGetErrorString(e));
    }
    HIPCHK(hipEventRecord(ctx->done, st));
    ctx->launched = true;
    return rc;
}
}  // namespace

int qd_rows_geometry(const qd_chain_desc *desc, const qd_rows_desc *rows, uint64_t *offsets, size_t cap, uint64_t *src_first, uint64_t *src_count) {
    if (!src_first || !src_count) return fail(QD_ERR_INVALID, "src_first/src_count is NULL");
    StageGeo g;
    if (const int rc = rows_chain_geo(desc, &g)) return rc;
    std::vector<uint64_t> offs;
    uint64_t lo = 0, hi = 0;
    const bool fir = desc->has_lowpass != 0;
    if (const int rc = rows_layout(desc->n_samples, g.len, desc->width, fir ? desc->decimate : 1, fir ? desc->taps : 0, rows, &offs, &lo, &hi)) return rc;
    if (offs.size() > cap || (!offsets && !offs.empty())) return fail(QD_ERR_INVALID, "offsets holds %zu entries, the rows need %zu", offsets ? cap : (size_t)0, offs.size());
    if (!offs.empty()) memcpy(offsets, offs.data(), offs.size() * 8);
    *src_first = lo; *src_count = hi - lo;
    return QD_OK;
}

int qd_plan_take_fft(qd_plan *p, const qd_rows_desc *rows, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                     float *out, int out_mem, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "plan is NULL");
    if (!p->rows) return fail(QD_ERR_INVALID, "qd_plan_take_fft needs a QD_EPI_ROWS_F32 plan");
    if (src_first + src_count > p->d.n_samples) return fail(QD_ERR_INVALID, "src slab exceeds the stream length");
    const uint64_t W = p->blk_len, D = p->D, T = p->T, span = W * D + T;
    std::vector<uint64_t> offs;
    uint64_t lo = 0, hi = 0;
    if (const int rc = rows_layout(p->d.n_samples, p->dec_len, W, D, T, rows, &offs, &lo, &hi)) return rc;
    const uint64_t n_rows = offs.size();
    if (n_rows == 0) return QD_OK;
    if (!src || !out) return fail(QD_ERR_INVALID, "NULL buffer");
    for (uint64_t i = 0; i < n_rows; ++i)
        if (offs[i] * D < src_first || offs[i] * D + span > src_first + src_count)
            return fail(QD_ERR_SHORT, "row %llu reads source samples [%llu, +%llu), not inside the slab [%llu, +%llu)", (unsigned long long)i,
                        (unsigned long long)(offs[i] * D), (unsigned long long)span, (unsigned long long)src_first, (unsigned long long)src_count);
    const bool dev = src_mem == QD_MEM_DEVICE && out_mem == QD_MEM_DEVICE;
    if (!dev && (!host_kind(src_mem) || !host_kind(out_mem)))
        return fail(QD_ERR_UNSUPPORTED, "mixed host/device buffers are not supported; use both host or both device");
    std::vector<float> win;
    if (rows->windowing == 1) blackman_harris(W, &win);
    std::vector<uint64_t> soffs(n_rows);
    for (uint64_t i = 0; i < n_rows; ++i) soffs[i] = offs[i] * D;
    std::lock_guard<std::mutex> lock(p->mu);
    DeviceGuard guard(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    const int bps = bps_of(p->d.format);
    void *doffs = nullptr, *dwin = nullptr;
    int rc = ws.get(2, n_rows * 8, &doffs); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(doffs, soffs.data(), n_rows * 8, hipMemcpyHostToDevice, st));
    if (!win.empty()) {
        rc = ws.get(3, W * 4, &dwin); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(dwin, win.data(), W * 4, hipMemcpyHostToDevice, st));
    }
    const bool two_stage = p->rows_blue && p->has_fir;
    void *dcar = nullptr, *dboffs = nullptr;
    if (two_stage) {                                  // the carrier of the rows' read_at blocks and their places in it
        rc = ws.get(4, n_rows * W * 8, &dcar); if (rc) return rc;
        rc = ws.get(5, n_rows * 8, &dboffs); if (rc) return rc;
        for (uint64_t i = 0; i < n_rows; ++i) offs[i] = i * W;
        HIPCHK(hipMemcpyAsync(dboffs, offs.data(), n_rows * 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));                 // the tables are locals of this call
    // host slabs go up in one piece: the stretch the rows read, [lo, hi) — nothing of the slab outside it is touched
    const void *src_d = src; void *out_d = out;
    uint64_t d_first = src_first, d_count = src_count;
    if (!dev) {
        void *di = nullptr, *dout = nullptr;
        rc = ws.get(0, (hi - lo) * bps, &di); if (rc) return rc;
        rc = ws.get(1, n_rows * W * 4, &dout); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(di, static_cast<const uint8_t *>(src) + (lo - src_first) * bps, (hi - lo) * bps, hipMemcpyHostToDevice, st));
        src_d = di; out_d = dout; d_first = lo; d_count = hi - lo;
    }
    if (!p->rows_blue) {
        rc = launch_rows(p, src_d, d_first, d_count, static_cast<const uint64_t *>(doffs), static_cast<const float *>(dwin), n_rows, lo, hi, out_d,
                         QD_EPI_NORMS_F32, st);
    } else if (two_stage) {
        rc = launch_rows(p, src_d, d_first, d_count, static_cast<const uint64_t *>(doffs), nullptr, n_rows, lo, hi, dcar, QD_EPI_CF32_BLOCKS, st);
        BlueSrc bs{};
        bs.in = static_cast<const uint8_t *>(dcar); bs.in_first = 0;
        if (rc == QD_OK) rc = bluestein_rows(QD_FMT_CF32, 0, bs, static_cast<const uint64_t *>(dboffs), static_cast<const float *>(dwin), W, n_rows,
                                             static_cast<float *>(out_d), st);
    } else {
        BlueSrc bs{};
        bs.in = static_cast<const uint8_t *>(src_d); bs.in_first = d_first;
        NcoTabs *ctx = &p->tabs_dev;                  // the row table is the context's: launches that use it are ordered (see NcoTabs)
        if (!ctx->done) HIPCHK(hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming));
        if (ctx->launched) HIPCHK(hipStreamWaitEvent(st, ctx->done, 0));
        if (p->has_shift) {
            rc = ensure_rowtab(&p->rows_tab512, p->ratio, 512, lo, hi + 512, st);
            bs.ratio = p->ratio; bs.rowtab = p->rows_tab512.d; bs.rowtab_row0 = p->rows_tab512.row0; bs.jtab = p->jtab_d;
        }
        if (rc == QD_OK) rc = bluestein_rows(p->d.format, p->nco, bs, static_cast<const uint64_t *>(doffs), static_cast<const float *>(dwin), W, n_rows,
                                             static_cast<float *>(out_d), st);
        HIPCHK(hipEventRecord(ctx->done, st));
        ctx->launched = true;
    }
    if (rc) return rc;
    if (!dev) {
        HIPCHK(hipMemcpyAsync(out, out_d, n_rows * W * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return QD_OK;
}

// ------------------------------------------------------------------ level summary

namespace {
float f32_of_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
uint32_t bits_of_f32(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int check_summary(const qd_summary *sum) {
    if (!sum) return fail(QD_ERR_INVALID, "summary is NULL");
    if (sum->struct_size != sizeof(qd_summary)) return fail(QD_ERR_INVALID, "qd_summary size mismatch (qd_summary_init sets it)");
    return QD_OK;
}

#ifdef QD_DEVELOP
int summary_layout() { const char *e = dev_env("QD_SUMMARY_LAYOUT"); return e ? atoi(e) & 3 : 0; }
#else
int summary_layout() { return 0; }
#endif

// one batch of norms rows (device memory, 16-byte aligned) into the device accumulator, on `st`
int launch_summary(const qd_plan *p, const float *norms_d, uint64_t n_rows, SumAcc *acc, hipStream_t st) {
    if (n_rows == 0) return QD_OK;
    SumParams P{};
    uint32_t grid = 0;
    int V = 1;
    sum_geometry(n_rows, p->W, p->n_cu, &P, &grid, &V);
    P.norms = norms_d; P.acc = acc;
    void (*fn)(SumParams) = V == 4 ? k_summary<4, 0> : k_summary<1, 0>;
#ifdef QD_DEVELOP
    switch (summary_layout()) {
    case 1: fn = V == 4 ? k_summary<4, 1> : k_summary<1, 1>; break;
    case 2: fn = V == 4 ? k_summary<4, 2> : k_summary<1, 2>; break;
    case 3: fn = V == 4 ? k_summary<4, 3> : k_summary<1, 3>; break;
    default: break;
    }
#endif
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kSumThreads), 0, st, P);
    HIPCHK(hipGetLastError());
    return QD_OK;
}

// The driver of the folds of a norms plan's windows (qd_plan_summarize, qd_plan_pool, qd_plan_mean, qd_plan_density).  An entry point
// calls its steps in this order, with its own argument checks where they have always stood:
//   norms_plan, unsharded, admit    the refusals every fold shares, and the cascade short-read clamp (n_windows is the complete part after it)
//   open                            plan mutex, device, workspace lease: from here the sink lays out and initialises its accumulators ("begin")
//   walk (or device / host)         the norms of every window, batch by batch, to the sink's launch ("batch")
//   close (or sync, short_read)     after the sink has queued its results' way home ("end"): stream sync, status merge, the short read's report
struct Fold {
    qd_plan *p; const char *call;
    const void *src; int src_mem; uint64_t src_first, src_count, first_window, n_windows;
    hipStream_t st;
    bool is_short = false;
    std::unique_lock<std::mutex> lock;
    std::optional<DeviceGuard> guard;
    std::optional<WsLease> ws;
    float *car = nullptr; uint64_t cw = 0;          // device sources: the carrier (workspace slot 0) and its windows

    // one batch of norms rows (device memory, 16-byte aligned), windows [g0, g0 + nw) of the range, to be folded on `st`
    using Batch = std::function<int(const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t st)>;

    int norms_plan() const {
        if (p->rows || p->d.epilogue != QD_EPI_NORMS_F32) return fail(QD_ERR_INVALID, "%s folds the norms sink's rows: it needs a QD_EPI_NORMS_F32 plan", call);
        return QD_OK;
    }
    int unsharded(const char *advice) const { return p->opt.n_shards > 1 ? fail(QD_ERR_UNSUPPORTED, "%s", advice) : QD_OK; }
    int admit() {
        if (first_window + n_windows > p->n_windows)
            return fail(QD_ERR_SHORT, "windows [%llu,+%llu) exceed the sink's loop (%llu windows)", (unsigned long long)first_window,
                        (unsigned long long)n_windows, (unsigned long long)p->n_windows);
        if (src_first + src_count > p->d.n_samples) return fail(QD_ERR_INVALID, "src slab exceeds the stream length");
        if (p->casc && first_window + n_windows > p->c_complete) {       // as qd_plan_run: every complete window of the range, then the short read
            n_windows = first_window < p->c_complete ? p->c_complete - first_window : 0;
            is_short = true;
        }
        return known_mem(src_mem, "src_mem");
    }
    static int known_mem(int mem, const char *what) { return mem == QD_MEM_DEVICE || host_kind(mem) ? QD_OK : fail(QD_ERR_INVALID, "unknown %s %d", what, mem); }
    int open() {
        if (n_windows && !src) return fail(QD_ERR_INVALID, "src is NULL");
        lock = std::unique_lock<std::mutex>(p->mu);
        guard.emplace(p->device);
        ws.emplace(st);
        return ws->rc;
    }
    // device sources: the carrier holds at most max(chunk_bytes, a tile of windows) of norms; windows [g0, g0 + nw), nw <= cw, go through the
    // plan's own norms kernel into it, then the sink's launch behind it
    int carrier() {
        cw = chunk_windows(p, first_window, n_windows, (uint64_t)p->W * 4);
        void *c = nullptr;
        const int rc = ws->get(0, (size_t)(cw * p->W * 4), &c);
        car = static_cast<float *>(c);
        return rc;
    }
    int device(uint64_t g0, uint64_t nw, const Batch &batch) {
        const int rc = launch_windows(p, &p->tabs_dev, src, src_first, src_count, first_window + g0, nw, first_window + g0, car, st);
        return rc ? rc : batch(car, g0, nw, st);
    }
    // host sources: windows [g0, g0 + n) up the plan's ring, which cuts its own batches on its two streams; their launches fold into the
    // sink's accumulators side by side (atomics), so whatever `st` holds for those is through first.  The run statistics stay the last run's.
    int host(uint64_t g0, uint64_t n, const Batch &batch) {
        HIPCHK(hipStreamSynchronize(st));
        const uint64_t obw = (uint64_t)p->W * 4;
        return walk_host(p, src, src_mem, src_first, src_count, first_window + g0, n,
                         RingMode{std::max<uint64_t>((uint64_t)p->S * p->D * bps_of(p->d.format), obw), obw, false, true, nullptr},
                         [&](void *norms_d, uint64_t w, uint64_t nw, int, hipStream_t s) { return batch(static_cast<const float *>(norms_d), w - first_window, nw, s); },
                         nullptr);
    }
    int walk(const Batch &batch) {
        if (n_windows == 0) return QD_OK;
        if (src_mem != QD_MEM_DEVICE) return host(0, n_windows, batch);
        int rc = carrier();
        for (uint64_t g0 = 0; g0 < n_windows && rc == QD_OK; g0 += cw) rc = device(g0, std::min<uint64_t>(n_windows - g0, cw), batch);
        return rc;
    }
    int sync(int rc) const {
        if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess && rc == QD_OK) rc = fail(QD_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
        return rc;
    }
    int short_read() const {
        if (!is_short) return QD_OK;
        return fail(QD_ERR_SHORT, "window %llu: read_exact_at reads fewer samples than asked (%llu complete windows of %llu)",
                    (unsigned long long)p->c_complete, (unsigned long long)p->c_complete, (unsigned long long)p->n_windows);
    }
    int close(int rc) const { rc = sync(rc); return rc ? rc : short_read(); }
};

// What the pooled sinks (qd_plan_pool, qd_plan_mean, qd_plan_density) and their CPU twins share besides the driver.
int pool_given(uint64_t pool) { return pool ? QD_OK : fail(QD_ERR_INVALID, "pool is 0: a row folds at least one window"); }
// the rows R and cells R x W of a range of n_windows >= 1 windows as asked: pool is clamped to one row, and where a cell counts its values
// (max_count != 0) a row holds at most that many windows
int pool_rows(uint64_t *pool, uint64_t n_windows, uint32_t W, uint64_t max_count, uint64_t *R, uint64_t *cells) {
    if (*pool > n_windows) *pool = n_windows;                        // one row either way
    if (max_count && *pool > max_count) return fail(QD_ERR_INVALID, "a row of %llu windows: a group holds at most 2^31", (unsigned long long)*pool);
    *R = (n_windows - 1) / *pool + 1; *cells = *R * W;
    return QD_OK;
}
// Output planes of a sink: the caller's pointers when out_dev, else back to back in workspace slot `slot` (a plane of 0 bytes is absent
// and has no address); home queues the copies of the planes the caller asked for.
struct Planes {
    struct Plane { void *user; size_t bytes; void *dev; };
    std::vector<Plane> v;
    bool out_dev = false;
    int place(Fold &f, int slot, bool dev, std::initializer_list<Plane> planes) {
        v = planes; out_dev = dev;
        size_t total = 0;
        for (Plane &pl : v) { pl.dev = pl.bytes ? pl.user : nullptr; total += pl.bytes; }
        if (out_dev || total == 0) return QD_OK;
        void *base = nullptr;
        if (const int rc = f.ws->get(slot, total, &base)) return rc;
        for (Plane &pl : v) { pl.dev = pl.bytes ? base : nullptr; base = static_cast<uint8_t *>(base) + pl.bytes; }
        return QD_OK;
    }
    int home(hipStream_t st) const {
        for (const Plane &pl : v)
            if (!out_dev && pl.user && pl.bytes) HIPCHK(hipMemcpyAsync(pl.user, pl.dev, pl.bytes, hipMemcpyDeviceToHost, st));
        return QD_OK;
    }
};
int launch_grid(uint64_t grid, uint64_t nw) {
    return grid > 0x7fffffffull ? fail(QD_ERR_INVALID, "a batch of %llu windows is too large for one launch: lower chunk_bytes", (unsigned long long)nw) : QD_OK;
}
// the CPU twins' pre-pass over the rows that windows [at, at + n) touch (n >= 1), once per row and before anything is added: a row's
// cells take at most its windows of this call on top of the held(cell) values they hold
static_assert(kMeanMaxCount == kDensityMaxCount, "one limit for every counting cell");
int rows_have_room(uint64_t pool, uint64_t at, uint64_t n, uint32_t width, const std::function<uint64_t(uint64_t cell)> &held) {
    for (uint64_t r = at / pool; r <= (at + n - 1) / pool; ++r) {
        const uint64_t a = std::max(at, r * pool), b = std::min(at + n, (r + 1) * pool);
        for (uint32_t c = 0; c < width; ++c)
            if (held(r * width + c) + (b - a) > kMeanMaxCount) return fail(QD_ERR_INVALID, "row %llu would hold more than 2^31 windows", (unsigned long long)r);
    }
    return QD_OK;
}
}  // namespace

int qd_summary_init(qd_summary *sum, float *peak, float *floor, uint32_t width) {
    if (!sum) return fail(QD_ERR_INVALID, "summary is NULL");
    memset(sum, 0, sizeof *sum);
    sum->struct_size = sizeof *sum;
    sum->width = width;
    sum->min = INFINITY;
    sum->max = 0.0f;
    for (uint32_t b = 0; b < width; ++b) {
        if (peak) peak[b] = 0.0f;
        if (floor) floor[b] = INFINITY;
    }
    return QD_OK;
}

int qd_summary_fold(qd_summary *sum, float *peak, float *floor, const float *norms, uint64_t n_rows) {
    if (const int rc = check_summary(sum)) return rc;
    if (n_rows == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    const uint32_t W = sum->width;
    if (W == 0) return fail(QD_ERR_INVALID, "a summary of width 0 holds no rows");
    float mx = sum->max, mn = sum->min;
    uint64_t nan = 0;
    for (uint64_t r = 0; r < n_rows; ++r) {
        const float *row = norms + r * W;
        for (uint32_t b = 0; b < W; ++b) {
            const float x = row[b];
            if (x != x) { ++nan; continue; }               // f32::max / f32::min ignore a NaN operand (src/ffts.rs:101-107)
            sum->hist[(bits_of_f32(x) & 0x7fffffffu) >> 20] += 1;
            if (x > mx) mx = x;
            if (x < mn) mn = x;
            if (peak && x > peak[b]) peak[b] = x;
            if (floor && x < floor[b]) floor[b] = x;
        }
    }
    sum->max = mx; sum->min = mn;
    sum->n_nan += nan;
    sum->n_windows += n_rows;
    return QD_OK;
}

int qd_summary_merge(qd_summary *dst, float *dst_peak, float *dst_floor, const qd_summary *src, const float *src_peak, const float *src_floor) {
    if (const int rc = check_summary(dst)) return rc;
    if (const int rc = check_summary(src)) return rc;
    if (dst->width != src->width) return fail(QD_ERR_INVALID, "summaries of different widths (%u, %u) do not merge", dst->width, src->width);
    if ((dst_peak && !src_peak) || (dst_floor && !src_floor)) return fail(QD_ERR_INVALID, "a peak / floor array to merge into needs one to merge from");
    for (int i = 0; i < 2048; ++i) dst->hist[i] += src->hist[i];
    dst->n_nan += src->n_nan;
    dst->n_windows += src->n_windows;
    if (src->max > dst->max) dst->max = src->max;
    if (src->min < dst->min) dst->min = src->min;
    for (uint32_t b = 0; b < dst->width; ++b) {
        if (dst_peak && src_peak[b] > dst_peak[b]) dst_peak[b] = src_peak[b];
        if (dst_floor && src_floor[b] < dst_floor[b]) dst_floor[b] = src_floor[b];
    }
    return QD_OK;
}

int qd_summary_quantile(const qd_summary *sum, double q, float *lo, float *hi) {
    if (const int rc = check_summary(sum)) return rc;
    if (!(q >= 0.0 && q <= 1.0)) return fail(QD_ERR_INVALID, "quantile %g outside [0, 1]", q);
    uint64_t N = 0;
    for (int i = 0; i < 2048; ++i) N += sum->hist[i];
    if (N == 0) return fail(QD_ERR_INVALID, "the summary holds no values");
    const double want = std::ceil(q * (double)N);
    uint64_t r = want < 1.0 ? 1 : (want >= (double)N ? N : (uint64_t)want);
    uint64_t cum = 0;
    uint32_t j = 0;
    for (; j < 2048; ++j) { cum += sum->hist[j]; if (cum >= r) break; }
    if (lo) *lo = f32_of_bits(j << 20);
    if (hi) *hi = j >= 2040 ? INFINITY : f32_of_bits((j + 1) << 20);
    return QD_OK;
}

int qd_plan_summarize(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                      qd_summary *sum, float *peak, float *floor, void *stream) {
    if (!p || !sum) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_summarize", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    if (const int rc = f.norms_plan()) return rc;
    if (const int rc = f.unsharded("a sharded plan is not summarised in one call: summarise each shard's windows on a plan of its own and qd_summary_merge them")) return rc;
    const uint32_t W = p->W;
    (void)qd_summary_init(sum, peak, floor, W);
    if (const int rc = f.admit()) return rc;
    if (f.n_windows) {
        if (const int rc = f.open()) return rc;
        // the accumulator starts from the fold identities: +0.0 is bit pattern 0, +inf the largest non-NaN
        const size_t acc_bytes = sum_acc_bytes(W);
        std::vector<uint32_t> image(acc_bytes / 4, 0u);
        uint32_t *ipeak = image.data() + sizeof(SumAcc) / 4, *ifloor = ipeak + W;
        for (uint32_t b = 0; b < W; ++b) ifloor[b] = kSumInfBits;
        void *acc_v = nullptr;
        if (const int rc = f.ws->get(1, acc_bytes, &acc_v)) return rc;
        SumAcc *acc = static_cast<SumAcc *>(acc_v);
        HIPCHK(hipMemcpyAsync(acc, image.data(), acc_bytes, hipMemcpyHostToDevice, f.st));
        const int rc = f.sync(f.walk([&](const float *norms_d, uint64_t, uint64_t nw, hipStream_t s) { return launch_summary(p, norms_d, nw, acc, s); }));
        if (rc) return rc;
        HIPCHK(hipMemcpy(image.data(), acc, acc_bytes, hipMemcpyDeviceToHost));
        const SumAcc *h = reinterpret_cast<const SumAcc *>(image.data());
        memcpy(sum->hist, h->hist, sizeof sum->hist);
        sum->n_nan = h->n_nan;
        sum->n_windows = f.n_windows;
        uint32_t mx = 0, mn = kSumInfBits;
        for (uint32_t b = 0; b < W; ++b) {
            mx = std::max(mx, ipeak[b]); mn = std::min(mn, ifloor[b]);
            if (peak) peak[b] = f32_of_bits(ipeak[b]);
            if (floor) floor[b] = f32_of_bits(ifloor[b]);
        }
        sum->max = f32_of_bits(mx); sum->min = f32_of_bits(mn);
    }
    return f.short_read();
}

// ------------------------------------------------------------------ peak-hold rows

namespace {
// one batch of norms rows (device memory, 16-byte aligned) — windows [g0, g0 + nw) of a range of n_total — into the R x W accumulators, on `st`
int launch_pool(const qd_plan *p, const float *norms_d, uint64_t g0, uint64_t nw, uint64_t n_total, uint64_t pool, uint32_t *peak_d,
                uint32_t *floor_d, hipStream_t st) {
    if (nw == 0) return QD_OK;
    PoolParams P{};
    uint64_t grid = 0;
    int V = 1;
    pool_geometry(g0, nw, n_total, pool, p->W, p->n_cu, &P.G, &grid, &V);
    if (const int rc = launch_grid(grid, nw)) return rc;
    P.norms = norms_d; P.peak = peak_d; P.floor = floor_d;
    P.vec_store = (((uintptr_t)peak_d | (uintptr_t)floor_d) & 15) == 0;
    hipLaunchKernelGGL(V == 4 ? k_pool<4> : k_pool<1>, dim3((uint32_t)grid), dim3(kPoolThreads), 0, st, P);
    HIPCHK(hipGetLastError());
    return QD_OK;
}
}  // namespace

int qd_pool_init(float *peak_rows, float *floor_rows, uint32_t width, uint64_t rows) {
    const uint64_t n = (uint64_t)width * rows;
    for (uint64_t i = 0; i < n; ++i) {
        if (peak_rows) peak_rows[i] = 0.0f;
        if (floor_rows) floor_rows[i] = INFINITY;
    }
    return QD_OK;
}

int qd_pool_fold(float *peak_rows, float *floor_rows, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n) {
    if (const int rc = pool_given(pool)) return rc;
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (!peak_rows && !floor_rows) return fail(QD_ERR_INVALID, "both peak_rows and floor_rows are NULL");
    if (n == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    for (uint64_t i = 0; i < n; ++i) {
        const float *row = norms + i * width;
        const uint64_t o = (at + i) / pool * width;
        for (uint32_t b = 0; b < width; ++b) {
            const float x = row[b];
            if (x != x) continue;                                  // f32::max / f32::min ignore a NaN operand (src/ffts.rs:101-107)
            if (peak_rows && x > peak_rows[o + b]) peak_rows[o + b] = x;
            if (floor_rows && x < floor_rows[o + b]) floor_rows[o + b] = x;
        }
    }
    return QD_OK;
}

int qd_plan_pool(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                 uint64_t pool, float *peak_rows, float *floor_rows, int out_mem, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_pool", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    if (const int rc = f.norms_plan()) return rc;
    if (const int rc = pool_given(pool)) return rc;
    if (!peak_rows && !floor_rows) return fail(QD_ERR_INVALID, "both peak_rows and floor_rows are NULL");
    if (const int rc = Fold::known_mem(src_mem, "src_mem")) return rc;
    if (const int rc = Fold::known_mem(out_mem, "out_mem")) return rc;
    if (const int rc = f.unsharded("a sharded plan is not pooled in one call: give each device a contiguous range of rows on a plan of its own")) return rc;
    if (const int rc = f.admit()) return rc;
    if (n_windows == 0) return QD_OK;
    uint64_t R, words;                                               // rows of the range as asked; f.n_windows is its complete part
    if (const int rc = pool_rows(&pool, n_windows, p->W, 0, &R, &words)) return rc;
    if (const int rc = f.open()) return rc;
    const hipStream_t st = f.st;
    Planes out;                                                      // the accumulators: [peak][floor]
    if (const int rc = out.place(f, 1, out_mem == QD_MEM_DEVICE, {{peak_rows, peak_rows ? (size_t)(words * 4) : 0}, {floor_rows, floor_rows ? (size_t)(words * 4) : 0}})) return rc;
    uint32_t *peak_d = static_cast<uint32_t *>(out.v[0].dev), *floor_d = static_cast<uint32_t *>(out.v[1].dev);
    // the fold identities: +0.0 is bit pattern 0, +inf the largest non-NaN
    if (peak_d) HIPCHK(hipMemsetAsync(peak_d, 0, (size_t)(words * 4), st));
    if (floor_d) HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(floor_d), (int)kPoolInfBits, (size_t)words, st));
    int rc = f.walk([&](const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t s) {
        return launch_pool(p, norms_d, g0, nw, f.n_windows, pool, peak_d, floor_d, s);
    });
    if (rc == QD_OK) rc = out.home(st);
    return f.close(rc);
}

// ------------------------------------------------------------------ exact-sum rows: average, RMS and deviation traces (DESIGN.md sections 3.13, 3.17, 3.18; the one path is 3.24)

extern "C++" {                                                       // templates
namespace {
struct LimbAcc { unsigned long long *limbs; uint32_t *flags; uint64_t rows; };      // device: words x rows x W limbs (planar), rows flags

// k_power's form (qd_power.h): one bin a lane; a development build also holds four bins a lane, for measuring them side by side
#ifdef QD_DEVELOP
int power_form() { const char *e = dev_env("QD_POWER_V"); return e && atoi(e) == 4 ? 4 : 1; }
#else
int power_form() { return 1; }
#endif

// a cell's kernels on `grid` workgroups of `st` (qd_mean.h, qd_power.h; k_spread takes the same parameters in its own struct, qd_spread.h)
void enqueue_fold(const LimbParams<MeanCell> &M, int V, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(V == 4 ? k_mean<4> : k_mean<1>, dim3(grid), dim3(kPoolThreads), 0, st, M);
}
void enqueue_fold(const LimbParams<PowerCell> &M, int V, uint32_t grid, hipStream_t st) {
    void (*fn)(LimbParams<PowerCell>) = k_power<1>;
#ifdef QD_DEVELOP
    if (V == 4) fn = k_power<4>;
#endif
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kPoolThreads), 0, st, M);
}
void enqueue_fold(const LimbParams<SpreadCell> &M, int, uint32_t grid, hipStream_t st) {
    const SpreadCell::Out &o = M.out;
    const SpreadParams S{M.norms, M.G, o.std, o.ssd, o.count, o.mean, o.rms, M.acc, M.flags, M.r_base, M.acc_rows, M.cells, o.want};
    hipLaunchKernelGGL(k_spread, dim3(grid), dim3(kPoolThreads), 0, st, S);
}
// the finish kernel over the accumulator's flagged rows [r_base, r_base + n_rows)
void enqueue_finish(const MeanCell::Out &o, const LimbAcc &acc, uint64_t cells, uint64_t r_base, uint64_t n_rows, uint32_t W, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(k_mean_finish, dim3(grid), dim3(kPoolThreads), 0, st, acc.limbs, acc.flags, cells, r_base, n_rows, W, o);
}
void enqueue_finish(const PowerCell::Out &o, const LimbAcc &acc, uint64_t cells, uint64_t r_base, uint64_t n_rows, uint32_t W, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(k_power_finish, dim3(grid), dim3(kPoolThreads), 0, st, acc.limbs, acc.flags, cells, r_base, n_rows, W, o);
}
void enqueue_finish(const SpreadCell::Out &o, const LimbAcc &acc, uint64_t cells, uint64_t r_base, uint64_t n_rows, uint32_t W, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(k_spread_finish, dim3(grid), dim3(kPoolThreads), 0, st, acc.limbs, acc.flags, cells, r_base, n_rows, W, o.want, o.std, o.ssd, o.count, o.mean, o.rms);
}

// one batch of norms rows (device memory, 16-byte aligned) — the windows of G — into the outputs (whole rows) and the accumulator (cut
// rows), which holds rows [r_base, r_base + acc.rows) of the range, on `st`
template <class Cell>
int launch_limbs(const qd_plan *p, const PieceGeometry &G, uint64_t grid, int V, const float *norms_d, const typename Cell::Out &out, const LimbAcc &acc,
                 bool cuts, uint64_t r_base, hipStream_t st) {
    if (const int rc = launch_grid(grid, G.nw)) return rc;
    const uint64_t ra = G.g0 / G.pool, rb = (G.g0 + G.nw - 1) / G.pool;
    if (cuts && (ra < r_base || rb >= r_base + acc.rows)) return fail(QD_ERR_INVALID, "internal: rows [%llu,%llu] outside the accumulator", (unsigned long long)ra, (unsigned long long)rb);
    enqueue_fold(LimbParams<Cell>{norms_d, G, out, acc.limbs, acc.flags, r_base, cuts ? acc.rows : 0, acc.rows * p->W}, V, (uint32_t)grid, st);
    HIPCHK(hipGetLastError());
    return QD_OK;
}
// the flagged rows [r_base, r_base + n_rows) of the accumulator into the outputs
template <class Cell>
int launch_limbs_finish(const qd_plan *p, const LimbAcc &acc, uint64_t r_base, uint64_t n_rows, const typename Cell::Out &out, hipStream_t st) {
    const uint64_t cells = n_rows * p->W, grid = (cells + kPoolThreads - 1) / kPoolThreads;
    if (!cells) return QD_OK;
    enqueue_finish(out, acc, acc.rows * p->W, r_base, n_rows, p->W, (uint32_t)grid, st);
    HIPCHK(hipGetLastError());
    return QD_OK;
}

// The walk of the sinks that fold through a limb accumulator (qd_plan_mean, qd_plan_power, qd_plan_spread): the fold kernel rounds whole
// rows itself and adds cut rows into Cell::kWords planar u64 a cell, the finish kernel rounds the flagged rows.  The walk owns the
// accumulator (workspace slot 1: at most max(2 chunk_bytes, one row), its flags behind it) and the batches.  form: 0 lays a batch out with
// pool_geometry (k_mean), 1 or 4 with power_geometry in that form.
template <class Cell>
int walk_limbs(Fold &f, uint64_t pool, uint64_t R, int form, const typename Cell::Out &out) {
    const qd_plan *p = f.p;
    const uint64_t n_windows = f.n_windows;                          // the complete part of the range; R counts the rows as asked
    const hipStream_t st = f.st;
    if (!n_windows) return QD_OK;
    // the launch geometry of the batch [g0, g0 + nw) of the range's complete windows
    auto geometry = [&](uint64_t g0, uint64_t nw, PieceGeometry *G, uint64_t *grid, int *V) {
        if (form) power_geometry(g0, nw, n_windows, pool, p->W, p->n_cu, form, G, grid, V);
        else pool_geometry(g0, nw, n_windows, pool, p->W, p->n_cu, G, grid, V);
    };
    const uint64_t row_bytes = (uint64_t)p->W * Cell::kWords * 8;
    const uint64_t target = 2 * (p->opt.chunk_bytes ? p->opt.chunk_bytes : (64ull << 20));
    LimbAcc acc{nullptr, nullptr, std::max<uint64_t>(1, std::min<uint64_t>(target / row_bytes, R))};
    void *a = nullptr;
    int rc = f.ws->get(1, (size_t)(acc.rows * row_bytes + acc.rows * 4), &a); if (rc) return rc;
    acc.limbs = static_cast<unsigned long long *>(a);
    acc.flags = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(a) + acc.rows * row_bytes);
    auto clear = [&]() { HIPCHK(hipMemsetAsync(acc.limbs, 0, (size_t)(acc.rows * row_bytes + acc.rows * 4), st)); return (int)QD_OK; };
    if (f.src_mem == QD_MEM_DEVICE) {
        // this walk cuts its own batches of the carrier's windows
        rc = f.carrier();
        const uint64_t cw = f.cw, bw = pool <= cw ? cw / pool * pool : cw;       // seams on row boundaries where a chunk holds a row
        bool open = false;
        uint64_t r_base = 0;
        auto close = [&]() { const int c = open ? launch_limbs_finish<Cell>(p, acc, r_base, std::min(acc.rows, R - r_base), out, st) : QD_OK; open = false; return c; };
        for (uint64_t g0 = 0; g0 < n_windows && rc == QD_OK;) {
            uint64_t nw = std::min<uint64_t>(n_windows - g0, bw), grid = 0;
            PieceGeometry G{};
            int V = 1;
            geometry(g0, nw, &G, &grid, &V);
            const uint64_t ra = g0 / pool, rb = (g0 + nw - 1) / pool;
            const bool mid = g0 % pool != 0;                                     // row ra has windows in the open span already
            const bool cuts = G.spr > 1 || mid || ((g0 + nw) % pool && g0 + nw != n_windows);
            if (cuts) {
                if (!open || (!mid && rb >= r_base + acc.rows)) {                // move the accumulator: only between rows
                    rc = close();
                    if (rc == QD_OK) rc = clear();
                    r_base = ra; open = true;
                }
                if (rb >= r_base + acc.rows) {                                   // clip the batch to the rows the accumulator holds
                    nw = (r_base + acc.rows) * pool - g0;
                    geometry(g0, nw, &G, &grid, &V);
                }
            }
            if (rc == QD_OK)
                rc = f.device(g0, nw, [&](const float *norms_d, uint64_t, uint64_t, hipStream_t s) {
                    return launch_limbs<Cell>(p, G, grid, V, norms_d, out, acc, cuts, cuts ? r_base : ra, s);
                });
            g0 += nw;
        }
        if (rc == QD_OK) rc = close();
    } else {
        // host sources: the upload ring cuts its own batches, on two streams; the range goes span by span of the accumulator's rows
        const uint64_t Rn = (n_windows - 1) / pool + 1;
        for (uint64_t r_base = 0; r_base < Rn && rc == QD_OK; r_base += acc.rows) {
            const uint64_t g_a = r_base * pool, g_b = std::min<uint64_t>(n_windows, (r_base + acc.rows) * pool);
            rc = clear();
            if (rc) break;
            rc = f.host(g_a, g_b - g_a, [&](const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t s) {
                PieceGeometry G{};
                uint64_t grid = 0;
                int V = 1;
                geometry(g0, nw, &G, &grid, &V);
                return launch_limbs<Cell>(p, G, grid, V, norms_d, out, acc, true, r_base, s);
            });
            if (rc == QD_OK) rc = launch_limbs_finish<Cell>(p, acc, r_base, std::min(acc.rows, Rn - r_base), out, st);
        }
    }
    return rc;
}
// the empty rows of a sink whose outputs are an f32, an f64 and a u32 plane of `words` cells: the quiet NaN, 0.0, 0
int fill_no_values(float *f32_d, double *f64_d, uint32_t *u32_d, uint64_t words, hipStream_t st) {
    if (f32_d) HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(f32_d), (int)kMeanNanBits, (size_t)words, st));
    if (f64_d) HIPCHK(hipMemsetAsync(f64_d, 0, (size_t)(words * 8), st));
    if (u32_d) HIPCHK(hipMemsetAsync(u32_d, 0, (size_t)(words * 4), st));
    return QD_OK;
}

SpreadCell::Out spread_out(float *std, double *ssd, uint32_t *count, float *mean, float *rms) {
    return {std, ssd, count, mean, rms, (std ? kSpreadStd : 0u) | (ssd ? kSpreadSsd : 0u) | (mean ? kSpreadMean : 0u) | (rms ? kSpreadRms : 0u)};
}
// why a qd_spread_rows is refused, or nullptr
const char *spread_rows_refusal(const qd_spread_rows *out) {
    if (!out) return "out is NULL";
    if (!out->std_rows && !out->ssd_rows && !out->count_rows && !out->mean_rows && !out->rms_rows) return "std_rows, ssd_rows, count_rows, mean_rows and rms_rows are all NULL";
    return nullptr;
}

// What a plan call's outputs give plan_limbs, in one place per shape of outputs:
//   refusal()                     why they are refused (all NULL), or nullptr
//   place(planes, f, dev, words)  the caller's planes of `words` cells into workspace slot 2 or as they are, the f64 plane first
//   out(planes)                   the placed planes as the cell's Out;  fill_empty(out, words, st)  every row as a row without values
// the mean's and the power's: an f32, an f64 and a u32 plane
template <class C>
struct TraceRows {
    using Cell = C;
    float *f32; double *f64; uint32_t *u32;
    const char *all_null;
    const char *refusal() const { return !f32 && !f64 && !u32 ? all_null : nullptr; }
    int place(Planes &o, Fold &f, bool dev, uint64_t words) const {
        return o.place(f, 2, dev, {{f64, f64 ? (size_t)(words * 8) : 0}, {f32, f32 ? (size_t)(words * 4) : 0}, {u32, u32 ? (size_t)(words * 4) : 0}});
    }
    static typename C::Out out(const Planes &o) { return {static_cast<float *>(o.v[1].dev), static_cast<double *>(o.v[0].dev), static_cast<uint32_t *>(o.v[2].dev)}; }
    static int fill_empty(const typename C::Out &d, uint64_t words, hipStream_t st) {
        const auto &[f, g, u] = d;
        return fill_no_values(f, g, u, words, st);
    }
};
// the spread's: a qd_spread_rows, which may itself be NULL until refusal() has been asked
struct SpreadRows {
    using Cell = SpreadCell;
    const qd_spread_rows *rows;
    const char *refusal() const { return spread_rows_refusal(rows); }
    int place(Planes &o, Fold &f, bool dev, uint64_t words) const {                       // [ssd][std][count][mean][rms]
        auto plane = [&](void *u, size_t each) { return Planes::Plane{u, u ? (size_t)(words * each) : 0, nullptr}; };
        return o.place(f, 2, dev, {plane(rows->ssd_rows, 8), plane(rows->std_rows, 4), plane(rows->count_rows, 4), plane(rows->mean_rows, 4), plane(rows->rms_rows, 4)});
    }
    static SpreadCell::Out out(const Planes &o) {
        return spread_out(static_cast<float *>(o.v[1].dev), static_cast<double *>(o.v[0].dev), static_cast<uint32_t *>(o.v[2].dev),
                          static_cast<float *>(o.v[3].dev), static_cast<float *>(o.v[4].dev));
    }
    static int fill_empty(const SpreadCell::Out &d, uint64_t words, hipStream_t st) {
        if (const int e = fill_no_values(d.std, d.ssd, d.count, words, st)) return e;
        if (const int e = fill_no_values(d.mean, nullptr, nullptr, words, st)) return e;
        return fill_no_values(d.rms, nullptr, nullptr, words, st);
    }
};

// The body of qd_plan_mean, qd_plan_power and qd_plan_spread behind their own NULL check and Fold: the shared refusals in their order,
// the outputs' own (`rows`, above) in its place among them, `advice` to a sharded plan, `form` for walk_limbs.
template <class Rows>
int plan_limbs(Fold &f, uint64_t pool, int out_mem, const Rows &rows, const char *advice, int form) {
    using Cell = typename Rows::Cell;
    const uint64_t n_windows = f.n_windows;                          // as asked: admit clamps f.n_windows to the complete part
    if (const int rc = f.norms_plan()) return rc;
    if (const int rc = pool_given(pool)) return rc;
    if (const char *why = rows.refusal()) return fail(QD_ERR_INVALID, "%s", why);
    if (const int rc = Fold::known_mem(f.src_mem, "src_mem")) return rc;
    if (const int rc = Fold::known_mem(out_mem, "out_mem")) return rc;
    if (const int rc = f.unsharded(advice)) return rc;
    if (const int rc = f.admit()) return rc;
    if (n_windows == 0) return QD_OK;
    uint64_t R, words;                                               // rows of the range as asked; f.n_windows is its complete part
    if (const int rc = pool_rows(&pool, n_windows, f.p->W, kMeanMaxCount, &R, &words)) return rc;
    if (int rc = f.open()) return rc;
    Planes planes;
    int rc = rows.place(planes, f, out_mem == QD_MEM_DEVICE, words);
    if (rc) return rc;
    const typename Cell::Out out = Rows::out(planes);
    if (f.is_short) rc = Rows::fill_empty(out, words, f.st);         // a short cascade: rows without a complete window keep this
    if (rc == QD_OK) rc = walk_limbs<Cell>(f, pool, R, form, out);
    if (rc == QD_OK) rc = planes.home(f.st);
    return f.close(rc);
}

// The CPU twins of the three sinks: cells of Cell::kWords words, interleaved (word k of cell c at c kWords + k); the count word is the last
template <class Cell>
uint64_t cell_count(const uint64_t *cell) { return (cell[Cell::kWords - 1] & 0xffffffffull) + (cell[Cell::kWords - 1] >> 32); }

template <class Cell>
int limb_init(uint64_t *acc, uint32_t width, uint64_t rows) {
    if (!acc) return fail(QD_ERR_INVALID, "acc is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    memset(acc, 0, (size_t)(rows * width * Cell::kWords * 8));
    return QD_OK;
}
template <class Cell>
int limb_fold(uint64_t *acc, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n) {
    if (const int rc = pool_given(pool)) return rc;
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (!acc) return fail(QD_ERR_INVALID, "acc is NULL");
    if (n == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    if (const int rc = rows_have_room(pool, at, n, width, [&](uint64_t cell) { return cell_count<Cell>(acc + cell * Cell::kWords); })) return rc;
    for (uint64_t i = 0; i < n; ++i) {
        const float *row = norms + i * width;
        uint64_t *cells = acc + (at + i) / pool * width * Cell::kWords;
        for (uint32_t b = 0; b < width; ++b) {
            uint32_t bits;
            memcpy(&bits, row + b, 4);
            Cell::add(cells + (uint64_t)b * Cell::kWords, bits);
        }
    }
    return QD_OK;
}
template <class Cell>
int limb_merge(uint64_t *dst, const uint64_t *src, uint32_t width, uint64_t rows) {
    if (!dst || !src) return fail(QD_ERR_INVALID, "acc is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    const uint64_t cells = rows * width;
    for (uint64_t c = 0; c < cells; ++c)
        if (cell_count<Cell>(dst + c * Cell::kWords) + cell_count<Cell>(src + c * Cell::kWords) > kMeanMaxCount)
            return fail(QD_ERR_INVALID, "row %llu would hold more than 2^31 windows", (unsigned long long)(c / width));
    for (uint64_t i = 0; i < cells * Cell::kWords; ++i) dst[i] += src[i];
    return QD_OK;
}

static_assert(MeanCell::kWords == QD_MEAN_WORDS && PowerCell::kWords == QD_POWER_WORDS && SpreadCell::kWords == QD_SPREAD_WORDS, "the header's cell sizes");
}  // namespace
}  // extern "C++"

// ---- average-trace rows

int qd_mean_init(uint64_t *acc, uint32_t width, uint64_t rows) { return limb_init<MeanCell>(acc, width, rows); }
int qd_mean_fold(uint64_t *acc, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n) { return limb_fold<MeanCell>(acc, width, pool, at, norms, n); }
int qd_mean_merge(uint64_t *dst, const uint64_t *src, uint32_t width, uint64_t rows) { return limb_merge<MeanCell>(dst, src, width, rows); }

int qd_mean_finish(const uint64_t *acc, uint32_t width, uint64_t rows, float *mean_rows, double *sum_rows, uint32_t *count_rows) {
    if (!acc) return fail(QD_ERR_INVALID, "acc is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (!mean_rows && !sum_rows && !count_rows) return fail(QD_ERR_INVALID, "mean_rows, sum_rows and count_rows are all NULL");
    const uint64_t cells = rows * width;
    for (uint64_t c = 0; c < cells; ++c) {
        uint32_t mb, cnt; double s;
        mean_finish_cell(acc + c * QD_MEAN_WORDS, &mb, &s, &cnt);
        if (mean_rows) memcpy(mean_rows + c, &mb, 4);
        if (sum_rows) sum_rows[c] = s;
        if (count_rows) count_rows[c] = cnt;
    }
    return QD_OK;
}

int qd_plan_mean(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                 uint64_t pool, float *mean_rows, double *sum_rows, uint32_t *count_rows, int out_mem, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_mean", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    return plan_limbs(f, pool, out_mem, TraceRows<MeanCell>{mean_rows, sum_rows, count_rows, "mean_rows, sum_rows and count_rows are all NULL"},
        "a sharded plan is not averaged in one call: give each device a contiguous range of rows on a plan of its own, or merge per-shard accumulators (qd_mean_merge)", 0);
}

// ---- RMS-trace rows

int qd_power_init(uint64_t *acc, uint32_t width, uint64_t rows) { return limb_init<PowerCell>(acc, width, rows); }
int qd_power_fold(uint64_t *acc, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n) { return limb_fold<PowerCell>(acc, width, pool, at, norms, n); }
int qd_power_merge(uint64_t *dst, const uint64_t *src, uint32_t width, uint64_t rows) { return limb_merge<PowerCell>(dst, src, width, rows); }

int qd_power_finish(const uint64_t *acc, uint32_t width, uint64_t rows, float *rms_rows, double *sumsq_rows, uint32_t *count_rows) {
    if (!acc) return fail(QD_ERR_INVALID, "acc is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (!rms_rows && !sumsq_rows && !count_rows) return fail(QD_ERR_INVALID, "rms_rows, sumsq_rows and count_rows are all NULL");
    const uint64_t cells = rows * width;
    for (uint64_t c = 0; c < cells; ++c) {
        uint32_t rb, cnt; double s;
        power_finish_cell(acc + c * QD_POWER_WORDS, &rb, &s, &cnt);
        if (rms_rows) memcpy(rms_rows + c, &rb, 4);
        if (sumsq_rows) sumsq_rows[c] = s;
        if (count_rows) count_rows[c] = cnt;
    }
    return QD_OK;
}

int qd_plan_power(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                  uint64_t pool, float *rms_rows, double *sumsq_rows, uint32_t *count_rows, int out_mem, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_power", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    return plan_limbs(f, pool, out_mem, TraceRows<PowerCell>{rms_rows, sumsq_rows, count_rows, "rms_rows, sumsq_rows and count_rows are all NULL"},
        "a sharded plan is not power-averaged in one call: give each device a contiguous range of rows on a plan of its own, or merge per-shard accumulators (qd_power_merge)",
        power_form());
}

// ---- deviation-trace rows

int qd_spread_init(uint64_t *acc, uint32_t width, uint64_t rows) { return limb_init<SpreadCell>(acc, width, rows); }
int qd_spread_fold(uint64_t *acc, uint32_t width, uint64_t pool, uint64_t at, const float *norms, uint64_t n) { return limb_fold<SpreadCell>(acc, width, pool, at, norms, n); }
int qd_spread_merge(uint64_t *dst, const uint64_t *src, uint32_t width, uint64_t rows) { return limb_merge<SpreadCell>(dst, src, width, rows); }

int qd_spread_finish(const uint64_t *acc, uint32_t width, uint64_t rows, const qd_spread_rows *out) {
    if (!acc) return fail(QD_ERR_INVALID, "acc is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (const char *why = spread_rows_refusal(out)) return fail(QD_ERR_INVALID, "%s", why);
    const SpreadCell::Out o = spread_out(out->std_rows, out->ssd_rows, out->count_rows, out->mean_rows, out->rms_rows);
    const uint64_t cells = rows * width;
    for (uint64_t c = 0; c < cells; ++c) {
        SpreadRounded r;
        spread_finish_cell(acc + c * QD_SPREAD_WORDS, o.want, &r);
        if (o.std) memcpy(o.std + c, &r.std_bits, 4);
        if (o.ssd) o.ssd[c] = r.ssd;
        if (o.count) o.count[c] = r.count;
        if (o.mean) memcpy(o.mean + c, &r.mean_bits, 4);
        if (o.rms) memcpy(o.rms + c, &r.rms_bits, 4);
    }
    return QD_OK;
}

int qd_plan_spread(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                   uint64_t pool, const qd_spread_rows *rows, int out_mem, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_spread", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    return plan_limbs(f, pool, out_mem, SpreadRows{rows},
        "a sharded plan's deviation is not taken in one call: give each device a contiguous range of rows on a plan of its own, or merge per-shard accumulators (qd_spread_merge)", 1);
}

// ------------------------------------------------------------------ percentile traces and persistence counts

namespace {
int density_grid(uint32_t level0, uint32_t levels) {
    if (levels == 0 || levels > kDensityMaxLevels || level0 > kDensityBuckets || level0 + levels > kDensityBuckets)
        return fail(QD_ERR_INVALID, "a level grid of %u levels from bucket %u: 1 <= levels <= 256 and level0 + levels <= 2041", levels, level0);
    return QD_OK;
}
int density_q(double q) { return q >= 0.0 && q <= 1.0 ? QD_OK : fail(QD_ERR_INVALID, "quantile %g outside [0, 1]", q); }

// one batch of norms rows (device memory) — windows [g0, g0 + nw) of a range of n_total — into the R x W x L counts, on `st`
int launch_density(const qd_plan *p, const float *norms_d, uint64_t g0, uint64_t nw, uint64_t n_total, uint64_t pool, uint32_t level0, uint32_t levels,
                   uint32_t *counts_d, hipStream_t st) {
    if (nw == 0) return QD_OK;
    DensityParams D{};
    uint64_t grid = 0;
    density_geometry(g0, nw, n_total, pool, p->W, levels, p->n_cu, &D, &grid);
    if (const int rc = launch_grid(grid, nw)) return rc;
    D.norms = norms_d; D.counts = counts_d; D.level0 = level0;
    hipLaunchKernelGGL(k_density, dim3((uint32_t)grid), dim3(kDensityThreads), 0, st, D);
    HIPCHK(hipGetLastError());
    return QD_OK;
}
}  // namespace

int qd_density_init(uint32_t *counts, uint32_t width, uint32_t levels, uint64_t rows) {
    if (!counts) return fail(QD_ERR_INVALID, "counts is NULL");
    if (width == 0 || levels == 0) return fail(QD_ERR_INVALID, "rows of width 0 or of 0 levels hold nothing");
    memset(counts, 0, (size_t)(rows * width * levels * 4));
    return QD_OK;
}

int qd_density_fold(uint32_t *counts, uint32_t width, uint32_t level0, uint32_t levels, uint64_t pool, uint64_t at, const float *norms, uint64_t n) {
    if (const int rc = pool_given(pool)) return rc;
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (const int rc = density_grid(level0, levels)) return rc;
    if (!counts) return fail(QD_ERR_INVALID, "counts is NULL");
    if (n == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    auto held = [&](uint64_t cell) { return std::accumulate(counts + cell * levels, counts + (cell + 1) * levels, uint64_t{0}); };
    if (const int rc = rows_have_room(pool, at, n, width, held)) return rc;
    for (uint64_t i = 0; i < n; ++i) {
        const float *row = norms + i * width;
        uint32_t *cells = counts + (at + i) / pool * width * levels;
        for (uint32_t b = 0; b < width; ++b) {
            uint32_t bits;
            memcpy(&bits, row + b, 4);
            const uint32_t lv = density_level(bits, level0, levels);
            if (lv < levels) cells[(uint64_t)b * levels + lv] += 1;
        }
    }
    return QD_OK;
}

int qd_density_merge(uint32_t *dst, const uint32_t *src, uint32_t width, uint32_t levels, uint64_t rows) {
    if (!dst || !src) return fail(QD_ERR_INVALID, "counts is NULL");
    if (width == 0 || levels == 0) return fail(QD_ERR_INVALID, "rows of width 0 or of 0 levels hold nothing");
    const uint64_t cells = rows * width;
    for (uint64_t c = 0; c < cells; ++c) {
        uint64_t N = 0;
        for (uint32_t l = 0; l < levels; ++l) N += (uint64_t)dst[c * levels + l] + src[c * levels + l];
        if (N > kDensityMaxCount) return fail(QD_ERR_INVALID, "row %llu would hold more than 2^31 windows", (unsigned long long)(c / width));
    }
    for (uint64_t i = 0; i < cells * levels; ++i) dst[i] += src[i];
    return QD_OK;
}

int qd_density_quantile(const uint32_t *counts, uint32_t width, uint32_t level0, uint32_t levels, uint64_t rows, double q, float *lo_rows,
                        float *hi_rows, uint32_t *n_rows) {
    if (!counts) return fail(QD_ERR_INVALID, "counts is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (const int rc = density_grid(level0, levels)) return rc;
    if (const int rc = density_q(q)) return rc;
    if (!lo_rows && !hi_rows && !n_rows) return fail(QD_ERR_INVALID, "lo_rows, hi_rows and n_rows are all NULL");
    const uint64_t cells = rows * width;
    for (uint64_t c = 0; c < cells; ++c) {
        const uint32_t *cell = counts + c * levels;
        uint64_t N = 0;
        for (uint32_t l = 0; l < levels; ++l) N += cell[l];
        uint32_t lo = kDensityNanBits, hi = kDensityNanBits;
        if (N) {
            const uint32_t j = density_quantile_level(cell, 1, levels, N, q);
            lo = density_lo_bits(level0, j); hi = density_hi_bits(level0, levels, j);
        }
        if (lo_rows) memcpy(lo_rows + c, &lo, 4);
        if (hi_rows) memcpy(hi_rows + c, &hi, 4);
        if (n_rows) n_rows[c] = (uint32_t)N;
    }
    return QD_OK;
}

int qd_plan_density(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                    uint64_t pool, uint32_t level0, uint32_t levels, uint32_t *count_rows, const double *q, uint32_t n_q, float *trace_rows,
                    int out_mem, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_density", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    if (const int rc = f.norms_plan()) return rc;
    if (const int rc = pool_given(pool)) return rc;
    if (const int rc = density_grid(level0, levels)) return rc;
    if (n_q > (uint32_t)kDensityMaxQ) return fail(QD_ERR_INVALID, "%u quantiles: a call takes at most %d", n_q, kDensityMaxQ);
    if (n_q && !q) return fail(QD_ERR_INVALID, "q is NULL");
    DensityQ Q{};
    for (uint32_t i = 0; i < n_q; ++i) {
        if (const int rc = density_q(q[i])) return rc;
        Q.q[i] = q[i];
    }
    if (n_q && !trace_rows) return fail(QD_ERR_INVALID, "trace_rows is NULL with %u quantiles asked", n_q);
    if (!count_rows && !n_q) return fail(QD_ERR_INVALID, "both count_rows and trace_rows are NULL");
    if (const int rc = Fold::known_mem(src_mem, "src_mem")) return rc;
    if (const int rc = Fold::known_mem(out_mem, "out_mem")) return rc;
    if (const int rc = f.unsharded("a sharded plan is not counted in one call: give each device a contiguous range of rows on a plan of its own, or merge per-shard counts (qd_density_merge)")) return rc;
    if (const int rc = f.admit()) return rc;
    if (n_windows == 0) return QD_OK;
    const uint32_t W = p->W;
    uint64_t R, cells;                                               // rows of the range as asked; f.n_windows is its complete part
    if (const int rc = pool_rows(&pool, n_windows, W, kDensityMaxCount, &R, &cells)) return rc;
    const bool out_dev = out_mem == QD_MEM_DEVICE;
    const bool own_acc = !(out_dev && count_rows);
    if (own_acc && (cells > kDensityMaxWorkspace / 4 / levels))
        return fail(QD_ERR_UNSUPPORTED, "%llu rows x %u bins x %u levels of counts need a workspace of %llu bytes, above the %llu allowed: walk the range in spans of rows",
                    (unsigned long long)R, W, levels, (unsigned long long)(cells * levels * 4), (unsigned long long)kDensityMaxWorkspace);
    const uint64_t words = cells * levels;
    if (const int rc = f.open()) return rc;
    const hipStream_t st = f.st;
    // the accumulator: the caller's counts when they are device memory, else a workspace, asked for or not; the traces likewise
    Planes counts, traces;
    if (const int rc = counts.place(f, 1, !own_acc, {{count_rows, (size_t)(words * 4)}})) return rc;
    if (const int rc = traces.place(f, 2, out_dev, {{trace_rows, (size_t)(cells * n_q * 4)}})) return rc;
    uint32_t *acc = static_cast<uint32_t *>(counts.v[0].dev), *trace_d = static_cast<uint32_t *>(traces.v[0].dev);
    HIPCHK(hipMemsetAsync(acc, 0, (size_t)(words * 4), st));
    int rc = f.walk([&](const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t s) {
        return launch_density(p, norms_d, g0, nw, f.n_windows, pool, level0, levels, acc, s);
    });
    if (rc == QD_OK && n_q) {
        const uint64_t grid = (cells + kDensityThreads - 1) / kDensityThreads;
        if (grid > 0x7fffffffull) rc = fail(QD_ERR_INVALID, "%llu cells are too many for one launch: walk the range in spans of rows", (unsigned long long)cells);
        else {
            hipLaunchKernelGGL(k_density_quantile, dim3((uint32_t)grid), dim3(kDensityThreads), 0, st, acc, cells, level0, levels, Q, n_q, trace_d);
            HIPCHK(hipGetLastError());
        }
    }
    if (rc == QD_OK) rc = counts.home(st);
    if (rc == QD_OK) rc = traces.home(st);
    return f.close(rc);
}

// ------------------------------------------------------------------ band traces

namespace {
static_assert(sizeof(Band) == sizeof(qd_band) && kBandsMax == QD_BANDS_MAX && kBandNone == QD_BAND_NONE, "qd_bands.h and the public header agree on a band");

// the checks qd_bands_fold and qd_plan_bands share; *longest is the longest band's bins
int bands_given(const qd_band *bands, uint32_t n_bands, uint32_t W, const qd_band_rows *out, uint32_t *longest) {
    if (n_bands == 0 || n_bands > QD_BANDS_MAX) return fail(QD_ERR_INVALID, "%u bands: a call takes 1 ... %d", n_bands, QD_BANDS_MAX);
    if (!bands) return fail(QD_ERR_INVALID, "bands is NULL");
    *longest = 0;
    for (uint32_t k = 0; k < n_bands; ++k) {
        if (bands[k].lo >= bands[k].hi || bands[k].hi > W) return fail(QD_ERR_INVALID, "band %u is [%u, %u): 0 <= lo < hi <= %u", k, bands[k].lo, bands[k].hi, W);
        *longest = std::max(*longest, bands[k].hi - bands[k].lo);
    }
    if (!out) return fail(QD_ERR_INVALID, "out is NULL");
    if (!out->level_rows && !out->sum_rows && !out->count_rows && !out->peak_rows && !out->peak_bin_rows && !out->pick_rows)
        return fail(QD_ERR_INVALID, "every row of out is NULL");
    return QD_OK;
}
}  // namespace

int qd_bands_fold(const float *norms, uint32_t width, uint64_t n, const qd_band *bands, uint32_t n_bands, const qd_band_rows *out) {
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    uint32_t longest = 0;
    if (const int rc = bands_given(bands, n_bands, width, out, &longest)) return rc;
    if (n == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    uint32_t level[QD_BANDS_MAX], count[QD_BANDS_MAX];
    for (uint64_t i = 0; i < n; ++i) {
        const float *row = norms + i * width;
        for (uint32_t k = 0; k < n_bands; ++k) {
            uint64_t acc[kMeanWords] = {}, key = 0;
            for (uint32_t b = bands[k].lo; b < bands[k].hi; ++b) {
                uint32_t bits;
                memcpy(&bits, row + b, 4);
                mean_add(acc, bits);
                key = std::max(key, bands_key(bits, b));
            }
            double s;
            mean_finish_cell(acc, &level[k], &s, &count[k]);
            const uint64_t o = i * n_bands + k;
            const uint32_t pk = bands_key_peak(key);
            if (out->level_rows) memcpy(out->level_rows + o, &level[k], 4);
            if (out->sum_rows) out->sum_rows[o] = s;
            if (out->count_rows) out->count_rows[o] = count[k];
            if (out->peak_rows) memcpy(out->peak_rows + o, &pk, 4);
            if (out->peak_bin_rows) out->peak_bin_rows[o] = bands_key_bin(key);
        }
        if (out->pick_rows) out->pick_rows[i] = bands_pick(level, count, n_bands);
    }
    return QD_OK;
}

int qd_plan_bands(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                  const qd_band *bands, uint32_t n_bands, const qd_band_rows *out, int out_mem, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_bands", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    if (const int rc = f.norms_plan()) return rc;
    const uint32_t W = p->W, K = n_bands;
    uint32_t longest = 0;
    if (const int rc = bands_given(bands, n_bands, W, out, &longest)) return rc;
    if (const int rc = Fold::known_mem(src_mem, "src_mem")) return rc;
    if (const int rc = Fold::known_mem(out_mem, "out_mem")) return rc;
    if (const int rc = f.unsharded("a sharded plan's bands are not traced in one call: give each device a contiguous range of windows on a plan of its own; the rows simply concatenate")) return rc;
    if (const int rc = f.admit()) return rc;
    if (n_windows == 0) return QD_OK;
    const bool out_dev = out_mem == QD_MEM_DEVICE;
    const uint64_t items = n_windows * K;                            // of the range as asked; f.n_windows is its complete part
    // the workspace: the rows that are not device memory, and the level / count rows the pick reads when they are not asked for
    const bool own_level = out->pick_rows && !out->level_rows, own_count = out->pick_rows && !out->count_rows;
    uint64_t ws_bytes = (own_level ? items * 4 : 0) + (own_count ? items * 4 : 0);
    if (!out_dev)
        ws_bytes += (out->sum_rows ? items * 8 : 0) + (out->level_rows ? items * 4 : 0) + (out->count_rows ? items * 4 : 0) + (out->peak_rows ? items * 4 : 0) +
                    (out->peak_bin_rows ? items * 4 : 0) + (out->pick_rows ? n_windows : 0);
    if (ws_bytes > kBandsMaxWorkspace)
        return fail(QD_ERR_UNSUPPORTED, "%llu windows x %u bands need a workspace of %llu bytes, above the %llu allowed: walk the range in spans of windows",
                    (unsigned long long)n_windows, K, (unsigned long long)ws_bytes, (unsigned long long)kBandsMaxWorkspace);
    if (const int rc = f.open()) return rc;
    const hipStream_t st = f.st;
    Planes planes;                                                   // the outputs: [sum][level][count][peak][peak_bin][pick]
    int rc = planes.place(f, 2, out_dev, {{out->sum_rows, out->sum_rows ? (size_t)(items * 8) : 0}, {out->level_rows, out->level_rows ? (size_t)(items * 4) : 0},
                                          {out->count_rows, out->count_rows ? (size_t)(items * 4) : 0}, {out->peak_rows, out->peak_rows ? (size_t)(items * 4) : 0},
                                          {out->peak_bin_rows, out->peak_bin_rows ? (size_t)(items * 4) : 0}, {out->pick_rows, out->pick_rows ? (size_t)n_windows : 0}});
    if (rc) return rc;
    BandsParams B{};
    B.sum = static_cast<double *>(planes.v[0].dev); B.level = static_cast<float *>(planes.v[1].dev); B.count = static_cast<uint32_t *>(planes.v[2].dev);
    B.peak = static_cast<float *>(planes.v[3].dev); B.peak_bin = static_cast<uint32_t *>(planes.v[4].dev);
    uint8_t *pick_d = static_cast<uint8_t *>(planes.v[5].dev);
    void *v = nullptr;
    if (own_level) { rc = f.ws->get(3, (size_t)(items * 4), &v); if (rc) return rc; B.level = static_cast<float *>(v); }
    if (own_count) { rc = f.ws->get(4, (size_t)(items * 4), &v); if (rc) return rc; B.count = static_cast<uint32_t *>(v); }
    // the band table: device memory, uploaded once a call
    rc = f.ws->get(1, (size_t)K * sizeof(Band), &v); if (rc) return rc;
    B.bands = static_cast<const Band *>(v);
    HIPCHK(hipMemcpyAsync(v, bands, (size_t)K * sizeof(Band), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                                // the table is the caller's array
    if (f.is_short) {                                                // windows without a complete read keep the rows of a band without values
        rc = fill_no_values(B.level, B.sum, B.count, items, st); if (rc) return rc;
        if (B.peak) HIPCHK(hipMemsetAsync(B.peak, 0, (size_t)(items * 4), st));
        if (B.peak_bin) HIPCHK(hipMemsetAsync(B.peak_bin, 0xff, (size_t)(items * 4), st));
    }
    rc = f.walk([&](const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t s) {
        if (nw == 0) return (int)QD_OK;
        BandsParams Q = B;
        uint64_t grid = 0;
        bands_split(g0, nw, W, K, longest, &Q.G, &grid);
        if (const int c = launch_grid(grid, nw)) return c;
        Q.norms = norms_d;
        hipLaunchKernelGGL(k_bands, dim3((uint32_t)grid), dim3(kBandsThreads), 0, s, Q);
        HIPCHK(hipGetLastError());
        return (int)QD_OK;
    });
    if (rc == QD_OK && pick_d) {                                     // every batch is through or queued on st (Fold::host returns with its streams drained)
        const uint32_t lg = bands_pick_log2_lanes(K), per = kBandsThreads >> lg;
        const uint64_t grid = (n_windows + per - 1) / per;
        rc = launch_grid(grid, n_windows);
        if (rc == QD_OK) {
            hipLaunchKernelGGL(k_bands_pick, dim3((uint32_t)grid), dim3(kBandsThreads), 0, st, B.level, B.count, n_windows, K, lg, pick_d);
            HIPCHK(hipGetLastError());
        }
    }
    if (rc == QD_OK) rc = planes.home(st);
    return f.close(rc);
}

// ------------------------------------------------------------------ waterfall pictures

namespace {
static_assert(kPaintMaxWorkspace == QD_PICTURE_MAX_WORKSPACE, "qd_paint.h and the public header agree on the workspace cap");

int picture_scale(float scale) {
    return std::isfinite(scale) && scale > 0.0f ? QD_OK : fail(QD_ERR_INVALID, "scale %g: the colour map divides by a finite positive f32", (double)scale);
}
// the checks every picture call shares
int picture_page(const qd_picture_desc *d, uint32_t W, PaintPage *G) {
    if (!d) return fail(QD_ERR_INVALID, "desc is NULL");
    if (d->struct_size != sizeof(qd_picture_desc)) return fail(QD_ERR_INVALID, "qd_picture_desc size mismatch");
    if (W == 0) return fail(QD_ERR_INVALID, "windows of width 0 paint nothing");
    if (d->px_width == 0 || d->px_height == 0) return fail(QD_ERR_INVALID, "a picture of %u x %u pixels", d->px_width, d->px_height);
    if (d->stretch == 0) return fail(QD_ERR_INVALID, "stretch is 0: a bin paints at least one pixel row");
    if (const int rc = picture_scale(d->scale)) return rc;
    paint_page(W, d->px_width, d->px_height, d->stretch, d->scan, d->scale, G);
    return QD_OK;
}
}  // namespace

int qd_picture_geometry(const qd_picture_desc *desc, uint32_t width, uint64_t *strips, uint64_t *max_windows, uint64_t *bytes) {
    PaintPage G;
    if (const int rc = picture_page(desc, width, &G)) return rc;
    if (strips) *strips = G.strips;
    if (max_windows) *max_windows = G.max_windows;
    if (bytes) *bytes = G.bytes;
    return QD_OK;
}

int qd_picture_color(const float *norms, size_t n, float scale, uint8_t *rgb) {
    if (const int rc = picture_scale(scale)) return rc;
    if (n == 0) return QD_OK;
    if (!norms || !rgb) return fail(QD_ERR_INVALID, "NULL argument");
    for (size_t i = 0; i < n; ++i) {
        const uint32_t px = paint_color(norms[i], scale);
        rgb[3 * i] = (uint8_t)px; rgb[3 * i + 1] = (uint8_t)(px >> 8); rgb[3 * i + 2] = (uint8_t)(px >> 16);
    }
    return QD_OK;
}

int qd_picture_init(uint8_t *pixels, const qd_picture_desc *desc) {
    PaintPage G;
    if (const int rc = picture_page(desc, 1, &G)) return rc;
    if (!pixels) return fail(QD_ERR_INVALID, "pixels is NULL");
    memset(pixels, 0, (size_t)G.bytes);
    return QD_OK;
}

int qd_picture_fold(uint8_t *pixels, const qd_picture_desc *desc, uint32_t width, uint64_t at, const float *norms, uint64_t n) {
    PaintPage G;
    if (const int rc = picture_page(desc, width, &G)) return rc;
    if (!pixels) return fail(QD_ERR_INVALID, "pixels is NULL");
    if (n == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    for (uint64_t i = 0; i < n && at + i < G.max_windows; ++i) {         // the reference breaks out of its loop at the first strip past the page (:330)
        const uint64_t p = at + i, x = p % G.w, oy = p / G.w * G.row_height;
        const bool marker = paint_marker(p, G.scan);
        const float *row = norms + i * width;
        for (uint32_t o = 0; o < width; ++o) {
            const uint64_t ya = oy + (uint64_t)o * G.stretch;
            if (ya >= G.h) break;
            const uint32_t px = marker ? 0u : paint_color(row[o], G.scale);
            for (uint64_t y = ya; y < ya + G.stretch && y < G.h; ++y) {
                uint8_t *d = pixels + ((G.h - 1 - y) * G.w + x) * 3;
                d[0] = (uint8_t)px; d[1] = (uint8_t)(px >> 8); d[2] = (uint8_t)(px >> 16);
            }
        }
    }
    return QD_OK;
}

int qd_plan_picture(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                    const qd_picture_desc *desc, uint8_t *pixels, int out_mem, uint64_t *painted, void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    Fold f{p, "qd_plan_picture", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)};
    if (const int rc = f.norms_plan()) return rc;
    PaintPage G;
    if (const int rc = picture_page(desc, p->W, &G)) return rc;
    if (!pixels) return fail(QD_ERR_INVALID, "pixels is NULL");
    if (const int rc = Fold::known_mem(src_mem, "src_mem")) return rc;
    if (const int rc = Fold::known_mem(out_mem, "out_mem")) return rc;
    if (const int rc = f.unsharded("a sharded plan is not painted in one call: give each device a contiguous range of columns on a plan of its own and compose the "
                                   "parts on the host, the way qd_picture_fold composes the parts of a range")) return rc;
    if (const int rc = f.admit()) return rc;
    const bool out_dev = out_mem == QD_MEM_DEVICE;
    if (!out_dev && G.bytes > kPaintMaxWorkspace)
        return fail(QD_ERR_UNSUPPORTED, "a picture of %u x %u pixels needs a workspace of %llu bytes, above the %llu allowed: paint into device memory, or page by page",
                    G.w, G.h, (unsigned long long)G.bytes, (unsigned long long)kPaintMaxWorkspace);
    // the windows that are looked at: the surplus past the page is not run through the chain, and cannot make the read short
    const uint64_t look = std::min(n_windows, G.max_windows);
    if (f.is_short && first_window + look <= p->c_complete) f.is_short = false;
    f.n_windows = std::min(f.n_windows, look);
    if (const int rc = f.open()) return rc;
    const hipStream_t st = f.st;
    Planes out;                                                      // the accumulator is the picture
    if (const int rc = out.place(f, 1, out_dev, {{pixels, (size_t)G.bytes}})) return rc;
    uint8_t *pix_d = static_cast<uint8_t *>(out.v[0].dev);
    HIPCHK(hipMemsetAsync(pix_d, 0, (size_t)G.bytes, st));           // black first
    const uint32_t tps = paint_tiles_per_strip(G.w), bin_tiles = (G.W + kPaintBins - 1) / kPaintBins;
    int rc = f.walk([&](const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t s) {
        if (nw == 0) return (int)QD_OK;
        PaintParams Q{};
        Q.norms = norms_d; Q.pixels = pix_d; Q.g0 = g0; Q.nw = nw;
        Q.tile0 = paint_tile_of(g0, G.w);
        Q.row_height = G.row_height;
        Q.W = G.W; Q.w = G.w; Q.h = G.h; Q.stretch = G.stretch; Q.scan = G.scan; Q.tiles_per_strip = tps; Q.bin_tiles = bin_tiles;
        Q.scale = G.scale;
        const uint64_t grid = (paint_tile_of(g0 + nw - 1, G.w) - Q.tile0 + 1) * bin_tiles;
        if (const int c = launch_grid(grid, nw)) return c;
        hipLaunchKernelGGL(k_paint, dim3((uint32_t)grid), dim3(kPaintThreads), 0, s, Q);
        HIPCHK(hipGetLastError());
        return (int)QD_OK;
    });
    if (rc == QD_OK) rc = out.home(st);
    rc = f.sync(rc);
    if (rc) return rc;
    if (painted) *painted = f.n_windows;
    return f.short_read();
}

// ------------------------------------------------------------------ event lists

namespace {
// the refusals of a list's arguments, in the order every caller has had them: found, the sink's minima in the sink's noun, the list
struct ListMin { uint64_t value; const char *name, *unit; };
int list_given(const void *list, uint64_t cap, const uint64_t *found, const char *noun, std::initializer_list<ListMin> mins) {
    if (!found) return fail(QD_ERR_INVALID, "found is NULL");
    for (const ListMin &m : mins)
        if (m.value == 0) return fail(QD_ERR_INVALID, "%s is 0: %s holds at least one %s", m.name, noun, m.unit);
    if (!list && cap) return fail(QD_ERR_INVALID, "list is NULL with cap %llu", (unsigned long long)cap);
    return QD_OK;
}

// the longest batch either walk of a fold cuts (the device carrier's, the host ring's): what a per-batch workspace is sized by
uint64_t longest_batch(const Fold &f) {
    const qd_plan *p = f.p;
    const uint64_t obw = (uint64_t)p->W * 4;
    return std::max(chunk_windows(p, f.first_window, f.n_windows, obw),
                    chunk_windows(p, f.first_window, f.n_windows, std::max<uint64_t>((uint64_t)p->S * p->D * bps_of(p->d.format), obw)));
}

// A record crosses batches, so a batch's walk starts behind the previous batch's: the host ring's two streams meet through an event.
// wait(s) stands in front of a batch's launches on its stream and record(s) behind them; a device source has one stream and needs neither.
struct Seam {
    hipEvent_t e[2] = {nullptr, nullptr}; bool ring = false; uint64_t k = 0;
    ~Seam() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }       // destroyed on every way out of the call
    int open(int src_mem) {
        ring = src_mem != QD_MEM_DEVICE;
        if (ring) for (hipEvent_t &x : e) HIPCHK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
        return QD_OK;
    }
    int wait(hipStream_t s) const { if (ring && k) HIPCHK(hipStreamWaitEvent(s, e[(k - 1) & 1], 0)); return QD_OK; }
    int record(hipStream_t s) { if (ring) HIPCHK(hipEventRecord(e[k & 1], s)); ++k; return QD_OK; }
};

// The driver of the sinks that list records (qd_plan_bursts, qd_plan_emissions), on top of Fold.  An entry point calls its steps in this
// order, with its own checks, workspace (slots 2 ... 4), batch launches and close launch between them:
//   whole, admit      the refusals the list sinks share around the sink's too-wide refusal; admit ends with Fold::open
//   lay               workspace slot 1 from one host image, and the list (slot 5 unless it is device memory): the cursor L but for its pieces
//   pieces            totals and bases of at most n pieces (slot 4)
//   home              found and the list come home: stream sync, status merge, *found, the short read's report
extern "C++" template <typename Record>
struct ListCall {
    Fold f;
    Record *list; uint64_t cap; uint64_t *found; int out_mem;
    uint64_t max_workspace;                                          // of the list when it is not device memory
    ListCursor<Record> L{}; unsigned long long *head = nullptr; bool out_dev = false;       // head: slot 1
    template <typename T> int slot(int i, size_t bytes, T **at) { void *v = nullptr; const int rc = f.ws->get(i, bytes, &v); *at = static_cast<T *>(v); return rc; }
    int whole(const char *sharded_advice) const {
        if (const int rc = Fold::known_mem(f.src_mem, "src_mem")) return rc;
        if (const int rc = Fold::known_mem(out_mem, "out_mem")) return rc;
        return f.unsharded(sharded_advice);
    }
    int admit() {
        if (const int rc = f.admit()) return rc;
        out_dev = out_mem == QD_MEM_DEVICE;
        if (!out_dev && cap > max_workspace / sizeof(Record))
            return fail(QD_ERR_UNSUPPORTED, "a list of %llu records needs a workspace of %llu bytes, above the %llu allowed: list into device memory, or lower cap",
                        (unsigned long long)cap, (unsigned long long)cap * sizeof(Record), (unsigned long long)max_workspace);
        return f.open();
    }
    // slot 1: [front: the sink's own u64 words][found = 0][behind: u64 words, zero][threshold words: W u32]; *thr_d receives the last
    int lay(const std::vector<uint64_t> &front, size_t behind, const std::vector<uint32_t> &thr, const uint32_t **thr_d) {
        const size_t head_words = front.size() + 1 + behind;
        std::vector<uint64_t> image(head_words + (thr.size() + 1) / 2, 0);
        std::copy(front.begin(), front.end(), image.begin());
        memcpy(image.data() + head_words, thr.data(), thr.size() * 4);
        if (const int rc = slot(1, image.size() * 8, &head)) return rc;
        HIPCHK(hipMemcpyAsync(head, image.data(), image.size() * 8, hipMemcpyHostToDevice, f.st));
        HIPCHK(hipStreamSynchronize(f.st));                          // the image is this call's array
        L.found = head + front.size(); L.cap = cap; L.list = list;
        *thr_d = reinterpret_cast<const uint32_t *>(head + head_words);
        return cap && !out_dev ? slot(5, (size_t)(cap * sizeof(Record)), &L.list) : QD_OK;
    }
    int pieces(uint64_t n) { const int rc = slot(4, (size_t)(n * 16), &L.totals); L.bases = L.totals + n; return rc; }
    // `also` comes home behind found: a plane of the sink's in the workspace (bytes 0: none)
    int home(int rc, void *also_user = nullptr, const void *also_dev = nullptr, size_t also_bytes = 0) {
        uint64_t total = 0;
        if (rc == QD_OK) {
            HIPCHK(hipMemcpyAsync(&total, L.found, 8, hipMemcpyDeviceToHost, f.st));
            if (also_bytes) HIPCHK(hipMemcpyAsync(also_user, also_dev, also_bytes, hipMemcpyDeviceToHost, f.st));
        }
        rc = f.sync(rc);
        if (rc) return rc;
        const uint64_t written = std::min(total, cap);
        if (written && !out_dev) HIPCHK(hipMemcpy(list, L.list, (size_t)(written * sizeof(Record)), hipMemcpyDeviceToHost));
        *found = total;
        return f.short_read();
    }
};
}  // namespace

// ------------------------------------------------------------------ burst list

namespace {
static_assert(sizeof(Burst) == sizeof(qd_burst) && sizeof(qd_burst) == 32 && kBurstsWords == QD_BURSTS_WORDS && kBurstsMaxWorkspace == QD_BURSTS_MAX_WORKSPACE,
              "qd_bursts.h and the public header agree on a record");

// the checks the twin and qd_plan_bursts share; words (may be NULL) receives the W threshold words
int bursts_given(uint32_t W, const float *thresholds, uint64_t min_len, const qd_burst *list, uint64_t cap, const uint64_t *found, uint32_t *words) {
    if (W == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (!thresholds) return fail(QD_ERR_INVALID, "thresholds is NULL");
    if (const int rc = list_given(list, cap, found, "a burst", {{min_len, "min_len", "window"}})) return rc;
    for (uint32_t b = 0; b < W; ++b) {
        uint32_t w;
        if (!bursts_threshold(bits_of_f32(thresholds[b]), &w))
            return fail(QD_ERR_INVALID, "threshold %u is %g: a threshold is +0 ... +inf, or a NaN that masks the bin", b, (double)thresholds[b]);
        if (words) words[b] = w;
    }
    return QD_OK;
}
void bursts_emit(const BurstsRun &r, uint64_t end, uint32_t bin, uint64_t min_len, qd_burst *list, uint64_t cap, uint64_t *found) {
    if (end - r.first < min_len) return;
    if (*found < cap) {
        qd_burst &d = list[*found];
        d.first = r.first; d.length = end - r.first; d.peak_at = r.peak_at; d.bin = bin; d.peak = f32_of_bits(r.peak);
    }
    *found += 1;
}
}  // namespace

int qd_bursts_init(uint64_t *state, uint64_t *on_counts, uint32_t width) {
    if (!state) return fail(QD_ERR_INVALID, "state is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    for (uint32_t b = 0; b < width; ++b) {
        state[(size_t)b * kBurstsWords] = kBurstsNone; state[(size_t)b * kBurstsWords + 1] = 0; state[(size_t)b * kBurstsWords + 2] = 0;
        if (on_counts) on_counts[b] = 0;
    }
    state[(size_t)width * kBurstsWords] = 0;
    return QD_OK;
}

int qd_bursts_fold(uint64_t *state, uint32_t width, const float *thresholds, uint64_t min_len, uint64_t at, const float *norms, uint64_t n,
                   qd_burst *list, uint64_t cap, uint64_t *found, uint64_t *on_counts) {
    if (!state) return fail(QD_ERR_INVALID, "state is NULL");
    std::vector<uint32_t> thr(width);
    if (const int rc = bursts_given(width, thresholds, min_len, list, cap, found, thr.data())) return rc;
    uint64_t &next = state[(size_t)width * kBurstsWords];
    if (at != next) return fail(QD_ERR_INVALID, "the fold starts at window %llu, the state expects %llu", (unsigned long long)at, (unsigned long long)next);
    if (n == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    for (uint64_t i = 0; i < n; ++i) {
        const float *row = norms + i * width;
        const uint64_t w = at + i;
        for (uint32_t b = 0; b < width; ++b) {
            uint64_t *s = state + (size_t)b * kBurstsWords;
            BurstsRun r{s[0], s[1], (uint32_t)s[2]}, e;
            const uint32_t a = bursts_mag(bits_of_f32(row[b]));
            const bool on = bursts_on(a, thr[b]);
            if (bursts_step(r, w, a, on, &e)) bursts_emit(e, w, b, min_len, list, cap, found);
            if (on && on_counts) on_counts[b] += 1;
            s[0] = r.first; s[1] = r.peak_at; s[2] = r.peak;
        }
    }
    next = at + n;
    return QD_OK;
}

int qd_bursts_finish(uint64_t *state, uint32_t width, uint64_t min_len, qd_burst *list, uint64_t cap, uint64_t *found) {
    if (!state) return fail(QD_ERR_INVALID, "state is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (const int rc = list_given(list, cap, found, "a burst", {{min_len, "min_len", "window"}})) return rc;
    const uint64_t next = state[(size_t)width * kBurstsWords];
    for (uint32_t b = 0; b < width; ++b) {
        const uint64_t *s = state + (size_t)b * kBurstsWords;
        if (s[0] != kBurstsNone) bursts_emit(BurstsRun{s[0], s[1], (uint32_t)s[2]}, next, b, min_len, list, cap, found);
    }
    return qd_bursts_init(state, nullptr, width);
}

int qd_plan_bursts(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                   const float *thresholds, uint64_t min_len, qd_burst *list, uint64_t cap, uint64_t *found, uint64_t *on_counts, int out_mem,
                   void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    ListCall<Burst> c{{p, "qd_plan_bursts", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)},
                      reinterpret_cast<Burst *>(list), cap, found, out_mem, kBurstsMaxWorkspace};
    Fold &f = c.f;
    if (const int rc = f.norms_plan()) return rc;
    const uint32_t W = p->W;
    std::vector<uint32_t> thr(W);
    if (const int rc = bursts_given(W, thresholds, min_len, list, cap, found, thr.data())) return rc;
    if (const int rc = c.whole("a sharded plan's bursts are not listed in one call: run one range on one device on a plan of its own; joining the lists across a "
                               "seam, where a run may cross, is the caller's job")) return rc;
    if (bursts_seg_max(W) == 0) return fail(QD_ERR_UNSUPPORTED, "windows of %u bins are too wide for the burst walker (at most 131072)", W);
    if (const int rc = c.admit()) return rc;
    const hipStream_t st = f.st;
    // slot 1: [state: 3 W][found][on_counts: W][threshold words: W u32]
    std::vector<uint64_t> state((size_t)kBurstsWords * W, 0);
    std::fill(state.begin(), state.begin() + W, kBurstsNone);
    BurstsParams B{};
    if (const int rc = c.lay(state, W, thr, &B.thr)) return rc;
    B.state = c.head;
    unsigned long long *counts_ws = c.L.found + 1;
    B.on_counts = !on_counts ? nullptr : c.out_dev ? reinterpret_cast<unsigned long long *>(on_counts) : counts_ws;
    if (on_counts && c.out_dev) HIPCHK(hipMemsetAsync(on_counts, 0, (size_t)W * 8, st));
    B.min_len = min_len;
    B.vec_store = ((uintptr_t)c.L.list & 15) == 0;
    int rc = QD_OK;
    if (f.n_windows) {
        // the per-piece words: sized by the longest batch either walk cuts
        const uint64_t bound = bursts_pieces_bound(longest_batch(f), W, p->n_cu);
        const size_t piece_bytes = (size_t)(bound * kBurstsWords * W * 8);
        if ((rc = c.slot(2, piece_bytes, &B.edge)) || (rc = c.slot(3, piece_bytes, &B.inc)) || (rc = c.pieces(bound))) return rc;
        B.L = c.L;
        Seam seam;
        if ((rc = seam.open(src_mem))) return rc;
        rc = f.walk([&](const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t s) {
            if (nw == 0) return (int)QD_OK;
            BurstsParams Q = B;
            uint64_t grid = 0;
            bursts_split(g0, nw, W, p->n_cu, &Q.G, &grid);
            if (Q.G.n_pieces > bound) return fail(QD_ERR_INVALID, "a batch of %llu windows is cut into more pieces than the workspace holds", (unsigned long long)nw);
            if (const int r = launch_grid(grid, nw)) return r;
            Q.norms = norms_d;
            if (const int r = seam.wait(s)) return r;
            hipLaunchKernelGGL(k_bursts_edge, dim3((uint32_t)grid), dim3(kBurstsThreads), 0, s, Q);
            hipLaunchKernelGGL(k_bursts_stitch, dim3((W + kBurstsStitchBins - 1) / kBurstsStitchBins), dim3(kBurstsThreads), 0, s, Q);
            hipLaunchKernelGGL(k_bursts_emit<kBurstsCount>, dim3((uint32_t)grid), dim3(kBurstsThreads), 0, s, Q);
            hipLaunchKernelGGL(k_bursts_scan, dim3(1), dim3(kBurstsThreads), 0, s, Q);
            if (cap) hipLaunchKernelGGL(k_bursts_emit<kBurstsEmit>, dim3((uint32_t)grid), dim3(kBurstsThreads), 0, s, Q);
            HIPCHK(hipGetLastError());
            return seam.record(s);
        });
        if (rc == QD_OK) {
            BurstsParams Q = B;
            Q.G.W = W;
            hipLaunchKernelGGL(k_bursts_close, dim3(1), dim3(kBurstsThreads), 0, st, Q, f.n_windows);
            HIPCHK(hipGetLastError());
        }
    }
    return c.home(rc, on_counts, counts_ws, on_counts && !c.out_dev ? (size_t)W * 8 : 0);
}

// ------------------------------------------------------------------ emission list

namespace {
static_assert(sizeof(Emission) == sizeof(qd_emission) && sizeof(qd_emission) == 56 && kEmissionsWords == QD_EMISSIONS_WORDS &&
              kEmissionsMaxWorkspace == QD_EMISSIONS_MAX_WORKSPACE && kEmissionsMaxWidth == QD_EMISSIONS_MAX_WIDTH &&
              kEmissionsCutFirst == QD_EMISSION_CUT_FIRST && kEmissionsCutLast == QD_EMISSION_CUT_LAST,
              "qd_emissions.h and the public header agree on a record");
static_assert(kEmissionsLdsWords * 4 <= 64 * 1024, "k_emissions_tile's LDS");

// the checks the twin and qd_plan_emissions share: the burst list's of the width, the thresholds and found, then the list's own
int emissions_given(uint32_t W, const float *thresholds, uint64_t min_len, uint64_t min_cells, const qd_emission *list, uint64_t cap, const uint64_t *found,
                    uint32_t *words) {
    if (const int rc = bursts_given(W, thresholds, 1, nullptr, 0, found, words)) return rc;
    return list_given(list, cap, found, "an emission", {{min_len, "min_len", "window"}, {min_cells, "min_cells", "cell"}});
}
}  // namespace

int qd_emissions_init(uint64_t *state, uint32_t width) {
    if (!state) return fail(QD_ERR_INVALID, "state is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    emissions_twin_init(state, width);
    return QD_OK;
}

int qd_emissions_fold(uint64_t *state, uint32_t width, const float *thresholds, uint64_t min_len, uint64_t min_cells, uint64_t at, const float *norms,
                      uint64_t n, qd_emission *list, uint64_t cap, uint64_t *found) {
    if (!state) return fail(QD_ERR_INVALID, "state is NULL");
    std::vector<uint32_t> thr(width);
    if (const int rc = emissions_given(width, thresholds, min_len, min_cells, list, cap, found, thr.data())) return rc;
    uint64_t &next = state[(size_t)width * kEmissionsWords];
    if (at != next) return fail(QD_ERR_INVALID, "the fold starts at window %llu, the state expects %llu", (unsigned long long)at, (unsigned long long)next);
    if (n == 0) return QD_OK;
    if (!norms) return fail(QD_ERR_INVALID, "norms is NULL");
    const EmissionsSink sink{reinterpret_cast<Emission *>(list), cap, found, min_len, min_cells};
    for (uint64_t i = 0; i < n; ++i) emissions_twin_row(state, width, thr.data(), at + i, reinterpret_cast<const uint32_t *>(norms + i * width), sink);
    next = at + n;
    return QD_OK;
}

int qd_emissions_finish(uint64_t *state, uint32_t width, uint64_t min_len, uint64_t min_cells, qd_emission *list, uint64_t cap, uint64_t *found) {
    if (!state) return fail(QD_ERR_INVALID, "state is NULL");
    if (width == 0) return fail(QD_ERR_INVALID, "rows of width 0 hold nothing");
    if (const int rc = list_given(list, cap, found, "an emission", {{min_len, "min_len", "window"}, {min_cells, "min_cells", "cell"}})) return rc;
    emissions_twin_finish(state, width, EmissionsSink{reinterpret_cast<Emission *>(list), cap, found, min_len, min_cells});
    return QD_OK;
}

int qd_plan_emissions(qd_plan *p, const void *src, int src_mem, uint64_t src_first, uint64_t src_count, uint64_t first_window, uint64_t n_windows,
                      const float *thresholds, uint64_t min_len, uint64_t min_cells, qd_emission *list, uint64_t cap, uint64_t *found, int out_mem,
                      void *stream) {
    if (!p) return fail(QD_ERR_INVALID, "NULL argument");
    ListCall<Emission> c{{p, "qd_plan_emissions", src, src_mem, src_first, src_count, first_window, n_windows, static_cast<hipStream_t>(stream)},
                         reinterpret_cast<Emission *>(list), cap, found, out_mem, kEmissionsMaxWorkspace};
    Fold &f = c.f;
    if (const int rc = f.norms_plan()) return rc;
    const uint32_t W = p->W;
    std::vector<uint32_t> thr(W);
    if (const int rc = emissions_given(W, thresholds, min_len, min_cells, list, cap, found, thr.data())) return rc;
    if (const int rc = c.whole("a sharded plan's emissions are not listed in one call: run one range on one device on a plan of its own; an emission crosses "
                               "the seam, and joining the lists there is the caller's job")) return rc;
    if (W > kEmissionsMaxWidth) return fail(QD_ERR_UNSUPPORTED, "windows of %u bins are too wide for the emission tiles (at most %u)", W, kEmissionsMaxWidth);
    if (const int rc = c.admit()) return rc;
    const hipStream_t st = f.st;
    // slot 1: [found][threshold words: W u32]
    EmissionsParams E{};
    if (const int rc = c.lay({}, 0, thr, &E.thr)) return rc;
    E.min_len = min_len; E.min_cells = min_cells;
    int rc = QD_OK;
    if (f.n_windows) {
        // the span's workspace: sized by the longest batch either walk cuts, and by the span rule whatever chunk_bytes is
        const uint64_t span_max = emissions_span_max(W, longest_batch(f)), ns = emissions_slots(W, span_max);
        if ((rc = c.slot(2, (size_t)emissions_plane_bytes(W, span_max), &E.plane)) || (rc = c.slot(3, (size_t)(ns * kEmissionsRecWords * 8), &E.rec)) ||
            (rc = c.pieces(emissions_pieces_bound(W, span_max)))) return rc;
        E.L = c.L;
        // nothing is open before the first window: an off virtual row without records
        HIPCHK(hipMemsetAsync(E.plane, 0xff, (size_t)W * 4, st));
        HIPCHK(hipMemsetAsync(E.rec + (uint64_t)kEmOwn * ns, 0xff, (size_t)emissions_half(W) * 8, st));
        Seam seam;
        if ((rc = seam.open(src_mem))) return rc;
        if (seam.ring) HIPCHK(hipStreamSynchronize(st));             // the virtual row is laid before a ring stream reads it
        EmissionsGeometry last{};
        rc = f.walk([&](const float *norms_d, uint64_t g0, uint64_t nw, hipStream_t s) {
            if (nw == 0) return (int)QD_OK;
            if (const int r = seam.wait(s)) return r;
            for (uint64_t a = 0; a < nw; a += span_max) {
                EmissionsParams Q = E;
                const uint64_t S = std::min<uint64_t>(nw - a, span_max);
                emissions_split(g0 + a, S, W, span_max, &Q.G);
                Q.norms = norms_d + a * W;
                const uint64_t slots = (S + 1) * Q.G.H;
                const dim3 t(kEmissionsThreads), g_slots((uint32_t)((slots + kEmissionsThreads - 1) / kEmissionsThreads));
                hipLaunchKernelGGL(k_emissions_tile, dim3(Q.G.n_trows * Q.G.n_tcols), t, 0, s, Q);
                hipLaunchKernelGGL(k_emissions_link, dim3((uint32_t)((emissions_link_lanes(Q.G) + kEmissionsThreads - 1) / kEmissionsThreads)), t, 0, s, Q);
                hipLaunchKernelGGL(k_emissions_fold, g_slots, t, 0, s, Q);
                hipLaunchKernelGGL(k_emissions_peak, g_slots, t, 0, s, Q);
                hipLaunchKernelGGL(k_emissions_emit<kEmissionsCount>, dim3(Q.G.n_pieces), t, 0, s, Q);
                hipLaunchKernelGGL(k_emissions_scan, dim3(1), t, 0, s, Q);
                if (cap) hipLaunchKernelGGL(k_emissions_emit<kEmissionsEmit>, dim3(Q.G.n_pieces), t, 0, s, Q);
                hipLaunchKernelGGL(k_emissions_carry, dim3((W + kEmissionsThreads - 1) / kEmissionsThreads), t, 0, s, Q);
                last = Q.G;
            }
            HIPCHK(hipGetLastError());
            return seam.record(s);
        });
        if (rc == QD_OK) {
            EmissionsParams Q = E;
            Q.G = last;
            hipLaunchKernelGGL(k_emissions_close, dim3(1), dim3(kEmissionsThreads), 0, st, Q);
            HIPCHK(hipGetLastError());
        }
    }
    return c.home(rc);
}

// ------------------------------------------------------------------ cut list (include/quadrs_hip.h, "cut list"; qd_cuts.h, qd_cuts_plan.h)

int qd_cuts_geometry(uint64_t sample_rate, uint64_t n_samples, const qd_cut *cuts, size_t n_cuts, uint64_t *offsets, uint64_t *src_first, uint64_t *src_count) {
    std::string err;
    if (const int rc = cuts_check(sample_rate, n_samples, cuts, n_cuts, false, 0, 0, offsets, src_first, src_count, &err)) return fail(rc, "%s", err.c_str());
    return QD_OK;
}

int qd_cut_of_emission(const qd_chain_desc *desc, uint64_t first_window, const qd_emission *e, const qd_cut_rule *rule, qd_cut *cut) {
    std::string err;
    if (const int rc = cut_of_emission(desc, first_window, e, rule, cut, &err)) return fail(rc, "%s", err.c_str());
    return QD_OK;
}

// qd_cuts_run's body, shared with qd_cuts_symbols.  check_only: the validation alone, up to where the first buffer would be looked at.
static int cuts_run_impl(int fmt, uint64_t sample_rate, uint64_t n_samples, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                         const qd_cut *cuts, size_t n_cuts, qd_c32 *out, int out_mem, const qd_plan_options *options, void *stream, bool check_only) {
    if (fmt < 0 || fmt > 3) return fail(QD_ERR_INVALID, "unknown format %d", fmt);
    if (src_mem < QD_MEM_HOST || src_mem > QD_MEM_HOST_PINNED || out_mem < QD_MEM_HOST || out_mem > QD_MEM_HOST_PINNED) return fail(QD_ERR_INVALID, "unknown memory kind");
    qd_plan_options opt;
    if (const int rc = check_options(options, &opt)) return rc;
    const uint64_t bps = (uint64_t)bps_of(fmt);
    if (src_count > (~0ull - src_first) || src_count > (1ull << 60)) return fail(QD_ERR_INVALID, "the slab [%llu, +%llu) is no range of samples", (unsigned long long)src_first, (unsigned long long)src_count);
    std::vector<uint64_t> offs(n_cuts + 1);
    std::string err;
    if (const int rc = cuts_check(sample_rate, n_samples, cuts, n_cuts, true, src_first, src_count, offs.data(), nullptr, nullptr, &err)) return fail(rc, "%s", err.c_str());
    if (offs[n_cuts] == 0 || check_only) return QD_OK;
    if (!src || !out) return fail(QD_ERR_INVALID, "NULL buffer");

    // the job table: one entry per cut; taps designed once per (lowpass_hz, taps), a lane table per distinct shift
    std::vector<CutJob> jobs(n_cuts);
    std::vector<float> taps_h;
    std::vector<double> lane_ratio;
    std::map<std::pair<uint64_t, uint64_t>, uint64_t> taps_of;
    std::map<int64_t, uint64_t> lane_of;
    for (size_t k = 0; k < n_cuts; ++k) {
        const qd_cut &c = cuts[k];
        CutJob &j = jobs[k];
        j = CutJob{};
        j.D = (uint32_t)c.decimate; j.T = (uint32_t)c.taps;
        j.span0 = c.first * c.decimate; j.valid = c.count * c.decimate + c.taps;
        if (c.count == 0) continue;
        auto t = taps_of.find({c.lowpass_hz, c.taps});
        if (t == taps_of.end()) {
            t = taps_of.insert({{c.lowpass_hz, c.taps}, (uint64_t)taps_h.size()}).first;
            taps_h.resize(taps_h.size() + c.taps);
            design_taps(c.lowpass_hz, sample_rate, c.taps, taps_h.data() + t->second);
        }
        j.taps_at = t->second;
        if (c.shift_hz != 0) {
            j.ratio = qd_shift_ratio(c.shift_hz, sample_rate);
            auto l = lane_of.find(c.shift_hz);
            if (l == lane_of.end()) { l = lane_of.insert({c.shift_hz, (uint64_t)lane_ratio.size()}).first; lane_ratio.push_back(j.ratio); }
            j.lane_at = l->second * kCutsNcoRow;
            j.flags = kCutShift | ((std::fabs(j.ratio) * (double)(j.span0 + j.valid) > 268435456.0) ? kCutSecondOrder : 0u);      // qd_shift's rule over the span
        }
    }
    std::vector<CutBatch> batches;
    cuts_batches(cuts, n_cuts, std::max<uint64_t>(1, (opt.chunk_bytes ? opt.chunk_bytes : kCutsDefaultChunk) / bps), &batches);

    int dev = 0;
    (void)hipGetDevice(&dev);
    const void *anchor = src_mem == QD_MEM_DEVICE ? src : (out_mem == QD_MEM_DEVICE ? (const void *)out : nullptr);
    if (anchor) {                                        // run where the caller's device buffer lives
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, anchor) == hipSuccess) dev = at.device;
        else (void)hipGetLastError();
    }
    DeviceGuard guard(dev);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    const bool src_dev = src_mem == QD_MEM_DEVICE, out_dev = out_mem == QD_MEM_DEVICE;
    const size_t n_lane = lane_ratio.size();
    const size_t jobs_b = (jobs.size() * sizeof(CutJob) + 15) & ~(size_t)15, taps_b = (taps_h.size() * 4 + 15) & ~(size_t)15, ratio_b = (n_lane * 8 + 15) & ~(size_t)15;
    void *tab_d = nullptr, *lane_d = nullptr;
    int rc = ws.get(2, jobs_b + taps_b + ratio_b, &tab_d); if (rc) return rc;
    rc = ws.get(3, std::max<size_t>(n_lane, 1) * kCutsNcoRow * sizeof(LaneEntry), &lane_d); if (rc) return rc;
    char *const tab = static_cast<char *>(tab_d);
    HIPCHK(hipMemcpyAsync(tab, jobs.data(), jobs.size() * sizeof(CutJob), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(tab + jobs_b, taps_h.data(), taps_h.size() * 4, hipMemcpyHostToDevice, st));
    if (n_lane) HIPCHK(hipMemcpyAsync(tab + jobs_b + taps_b, lane_ratio.data(), n_lane * 8, hipMemcpyHostToDevice, st));
    const CutJob *jobs_d = reinterpret_cast<const CutJob *>(tab);
    const float *taps_d = reinterpret_cast<const float *>(tab + jobs_b);
    const double *ratio_d = reinterpret_cast<const double *>(tab + jobs_b + taps_b);

    const void *fn = fmt == 0 ? reinterpret_cast<const void *>(k_cuts<0>) : fmt == 1 ? reinterpret_cast<const void *>(k_cuts<1>)
                   : fmt == 2 ? reinterpret_cast<const void *>(k_cuts<2>) : reinterpret_cast<const void *>(k_cuts<3>);
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCutsLdsBytes));

    std::vector<std::vector<CutTile>> kept;              // the tile tables stay alive until their copies are done
    kept.reserve(batches.size());
    std::vector<qd_c32> down;
    bool first_batch = true;
    for (const CutBatch &b : batches) {
        kept.emplace_back();
        std::vector<CutTile> &tiles = kept.back();
        cuts_tiles(cuts, b, out_dev, offs.data(), src_dev, src_first, &tiles);
        const uint32_t n_tiles = (uint32_t)tiles.size();
        const size_t tiles_b = ((size_t)n_tiles * sizeof(CutTile) + 31) & ~(size_t)31;
        void *batch_d = nullptr, *in_d = nullptr, *out_d = nullptr;
        rc = ws.get(4, tiles_b + (size_t)n_tiles * kCutsTileRows * sizeof(RowBase), &batch_d); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(batch_d, tiles.data(), (size_t)n_tiles * sizeof(CutTile), hipMemcpyHostToDevice, st));
        const CutTile *tiles_d = static_cast<const CutTile *>(batch_d);
        RowBase *rows_d = reinterpret_cast<RowBase *>(static_cast<char *>(batch_d) + tiles_b);
        const uint8_t *in = static_cast<const uint8_t *>(src);
        if (!src_dev) {                                  // only the union of the batch's reads goes up
            rc = ws.get(0, b.src_samples * bps + 16, &in_d); if (rc) return rc;
            for (const CutSpan &sp : b.spans)
                HIPCHK(hipMemcpyAsync(static_cast<char *>(in_d) + sp.at * bps, static_cast<const char *>(src) + (sp.first - src_first) * bps, sp.count * bps,
                                      hipMemcpyHostToDevice, st));
            in = static_cast<const uint8_t *>(in_d);
        }
        float2 *o = reinterpret_cast<float2 *>(out);
        if (!out_dev) {
            rc = ws.get(1, b.out_samples * 8, &out_d); if (rc) return rc;
            o = static_cast<float2 *>(out_d);
        }
        const uint32_t lanes = first_batch ? (uint32_t)n_lane : 0u;
        const uint64_t table_threads = (uint64_t)n_tiles * kCutsTileRows + (uint64_t)lanes * kCutsNcoRow;
        hipLaunchKernelGGL(k_cuts_tables, dim3((uint32_t)((table_threads + 255) / 256)), dim3(256), 0, st, jobs_d, tiles_d, n_tiles, rows_d, ratio_d, lanes,
                           static_cast<LaneEntry *>(lane_d));
        const RowBase *rows_c = rows_d;
        const LaneEntry *lane_c = static_cast<const LaneEntry *>(lane_d);
        switch (fmt) {
        case 0: hipLaunchKernelGGL(k_cuts<0>, dim3(n_tiles), dim3(kCutsThreads), kCutsLdsBytes, st, in, jobs_d, tiles_d, taps_d, rows_c, lane_c, o); break;
        case 1: hipLaunchKernelGGL(k_cuts<1>, dim3(n_tiles), dim3(kCutsThreads), kCutsLdsBytes, st, in, jobs_d, tiles_d, taps_d, rows_c, lane_c, o); break;
        case 2: hipLaunchKernelGGL(k_cuts<2>, dim3(n_tiles), dim3(kCutsThreads), kCutsLdsBytes, st, in, jobs_d, tiles_d, taps_d, rows_c, lane_c, o); break;
        default: hipLaunchKernelGGL(k_cuts<3>, dim3(n_tiles), dim3(kCutsThreads), kCutsLdsBytes, st, in, jobs_d, tiles_d, taps_d, rows_c, lane_c, o); break;
        }
        HIPCHK(hipGetLastError());
        first_batch = false;
        if (!out_dev) {                                  // the batch's outputs come down in one piece and are put in place here
            down.resize(b.out_samples);
            HIPCHK(hipMemcpyAsync(down.data(), out_d, b.out_samples * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (const CutPiece &p : b.pieces) memcpy(out + offs[p.cut] + p.first, down.data() + p.out_at, (size_t)p.count * 8);
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return QD_OK;
}

int qd_cuts_run(int fmt, uint64_t sample_rate, uint64_t n_samples, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                const qd_cut *cuts, size_t n_cuts, qd_c32 *out, int out_mem, const qd_plan_options *options, void *stream) {
    return cuts_run_impl(fmt, sample_rate, n_samples, src, src_mem, src_first, src_count, cuts, n_cuts, out, out_mem, options, stream, false);
}

// ------------------------------------------------------------------ symbol list (include/quadrs_hip.h, "symbol list"; qd_symbols.h, qd_symbols_plan.h)

int qd_symbols_geometry(const qd_symbols_desc *desc, const qd_segment *segments, size_t n, uint64_t *offsets) {
    std::string err;
    if (const int rc = symbols_check(desc, segments, n, false, 0, offsets, nullptr, nullptr, &err)) return fail(rc, "%s", err.c_str());
    return QD_OK;
}

// the device a call runs on: where the caller's device buffer lives
static int symbols_device_of(const void *a, bool a_dev, const void *b, bool b_dev) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const void *anchor = a_dev ? a : (b_dev ? b : nullptr);
    if (anchor) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, anchor) == hipSuccess) dev = at.device;
        else (void)hipGetLastError();
    }
    return dev;
}

// Validated segments of a device buffer (its element 0 is element `base` of the segments' indices) -> bytes at out_d + offs[k], all of it
// complete on return.  Workspace slots 2 (twiddles, window) and 4 (tile table).
static int symbols_on_device(const qd_symbols_desc &d, const float2 *in_d, uint64_t base, const qd_segment *segs, size_t n, const uint64_t *offs,
                             uint8_t *out_d, WsLease &ws, hipStream_t st) {
    const FftLayout L = fft_layout(d.width);
    std::vector<float> win;
    if (d.windowing) blackman_harris(d.width, &win);
    const size_t tw_b = (L.tw.size() * sizeof(float2) + 15) & ~(size_t)15;
    void *tab_d = nullptr;
    int rc = ws.get(2, tw_b + win.size() * 4 + 16, &tab_d); if (rc) return rc;
    if (!L.tw.empty()) HIPCHK(hipMemcpyAsync(tab_d, L.tw.data(), L.tw.size() * sizeof(float2), hipMemcpyHostToDevice, st));
    if (!win.empty()) HIPCHK(hipMemcpyAsync(static_cast<char *>(tab_d) + tw_b, win.data(), win.size() * 4, hipMemcpyHostToDevice, st));
    ChainParams P{};
    P.W = (uint32_t)d.width; P.logW = ilog2(d.width);
    P.S = (uint32_t)std::min<uint64_t>(d.stride, kSymMaxCount);
    P.base_len = L.base_len; P.log_base = L.log_base; P.layers = L.layers;
    P.epi = (uint32_t)d.epilogue;
    P.rmin = d.has_range ? d.range_min : 0.08f;          // src/fft.rs:22-23
    P.root2 = (float)std::sqrt(0.5);
    P.tw16_1 = compute_twiddle(1, 16); P.tw16_2 = compute_twiddle(2, 16); P.tw16_3 = compute_twiddle(3, 16);
    P.tw = static_cast<const float2 *>(tab_d);
    P.window = win.empty() ? nullptr : reinterpret_cast<const float *>(static_cast<char *>(tab_d) + tw_b);
    P.out = out_d; P.out_window0 = 0;
    const bool bucket = d.epilogue == QD_EPI_BUCKET2_U8;
    const void *fn = bucket ? reinterpret_cast<const void *>(k_symbols<QD_EPI_BUCKET2_U8>) : reinterpret_cast<const void *>(k_symbols<QD_EPI_MARK_U8>);
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSymLdsBytes));
    const uint32_t waves = symbols_waves(d.width);
    std::vector<std::vector<SymTile>> kept;              // the tile tables stay alive until their copies are done
    SymCursor cur;
    for (bool more = true; more;) {
        kept.emplace_back();
        std::vector<SymTile> &tiles = kept.back();
        more = symbols_tiles(&d, segs, n, offs, base, &cur, kSymBatchTiles, &tiles);
        if (tiles.empty()) break;
        const uint32_t n_tiles = (uint32_t)tiles.size();
        void *tiles_d = nullptr;
        rc = ws.get(4, (size_t)kSymBatchTiles * sizeof(SymTile), &tiles_d); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(tiles_d, tiles.data(), (size_t)n_tiles * sizeof(SymTile), hipMemcpyHostToDevice, st));
        const dim3 grid((n_tiles + waves - 1) / waves), block(kSymThreads);
        if (bucket) hipLaunchKernelGGL(k_symbols<QD_EPI_BUCKET2_U8>, grid, block, kSymLdsBytes, st, P, in_d, static_cast<const SymTile *>(tiles_d), n_tiles);
        else hipLaunchKernelGGL(k_symbols<QD_EPI_MARK_U8>, grid, block, kSymLdsBytes, st, P, in_d, static_cast<const SymTile *>(tiles_d), n_tiles);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));
    return QD_OK;
}

int qd_symbols_run(const qd_symbols_desc *desc, const qd_c32 *in, int in_mem, uint64_t n_in, const qd_segment *segments, size_t n,
                   uint8_t *out, int out_mem, void *stream) {
    if (in_mem < QD_MEM_HOST || in_mem > QD_MEM_HOST_PINNED || out_mem < QD_MEM_HOST || out_mem > QD_MEM_HOST_PINNED) return fail(QD_ERR_INVALID, "unknown memory kind");
    std::vector<uint64_t> offs(n + 1);
    uint64_t hull_first = 0, hull_count = 0;
    std::string err;
    if (const int rc = symbols_check(desc, segments, n, true, n_in, offs.data(), &hull_first, &hull_count, &err)) return fail(rc, "%s", err.c_str());
    const uint64_t total = offs[n];
    if (total == 0) return QD_OK;
    if (!in || !out) return fail(QD_ERR_INVALID, "NULL buffer");
    const bool in_dev = in_mem == QD_MEM_DEVICE, out_dev = out_mem == QD_MEM_DEVICE;
    DeviceGuard guard(symbols_device_of(in, in_dev, out, out_dev));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    const float2 *in_d = reinterpret_cast<const float2 *>(in);
    uint64_t base = 0;
    if (!in_dev) {                                       // the hull of the segments that have a window goes up
        void *up = nullptr;
        if (const int rc = ws.get(0, hull_count * 8 + 16, &up)) return rc;
        HIPCHK(hipMemcpyAsync(up, in + hull_first, hull_count * 8, hipMemcpyHostToDevice, st));
        in_d = static_cast<const float2 *>(up);
        base = hull_first;
    }
    uint8_t *out_d = out;
    if (!out_dev) {
        void *o = nullptr;
        if (const int rc = ws.get(1, total, &o)) return rc;
        out_d = static_cast<uint8_t *>(o);
    }
    if (const int rc = symbols_on_device(*desc, in_d, base, segments, n, offs.data(), out_d, ws, st)) return rc;
    if (!out_dev) {
        HIPCHK(hipMemcpyAsync(out, out_d, total, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return QD_OK;
}

int qd_cuts_symbols(int fmt, uint64_t sample_rate, uint64_t n_samples, const void *src, int src_mem, uint64_t src_first, uint64_t src_count,
                    const qd_cut *cuts, size_t n_cuts, const qd_symbols_desc *desc, uint8_t *out, int out_mem, const qd_plan_options *options, void *stream) {
    if (const int rc = cuts_run_impl(fmt, sample_rate, n_samples, src, src_mem, src_first, src_count, cuts, n_cuts, nullptr, out_mem, options, stream, true)) return rc;
    std::vector<qd_segment> segs(n_cuts);
    for (size_t k = 0; k < n_cuts; ++k) segs[k] = qd_segment{0, cuts[k].count};
    std::vector<uint64_t> offs(n_cuts + 1);
    std::string err;
    if (const int rc = symbols_check(desc, segs.data(), n_cuts, false, 0, offs.data(), nullptr, nullptr, &err)) return fail(rc, "%s", err.c_str());
    std::vector<std::pair<size_t, size_t>> groups;
    if (const int rc = symbols_groups(cuts, n_cuts, desc->iq_bytes, &groups, &err)) return fail(rc, "%s", err.c_str());
    if (offs[n_cuts] == 0) return QD_OK;
    if (!src || !out) return fail(QD_ERR_INVALID, "NULL buffer");
    const bool out_dev = out_mem == QD_MEM_DEVICE;
    DeviceGuard guard(symbols_device_of(src, src_mem == QD_MEM_DEVICE, out, out_dev));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    std::vector<uint64_t> goffs;
    for (const auto &g : groups) {
        const size_t k0 = g.first, ng = g.second - g.first;
        const uint64_t bytes = offs[g.second] - offs[k0];
        if (bytes == 0) continue;                        // (no cut of the group has a window: its IQ is not needed)
        uint64_t iq = 0;
        for (size_t k = 0; k < ng; ++k) { segs[k0 + k].first = iq; iq += cuts[k0 + k].count; }
        void *iq_d = nullptr;
        if (const int rc = ws.get(0, iq * 8, &iq_d)) return rc;
        if (const int rc = cuts_run_impl(fmt, sample_rate, n_samples, src, src_mem, src_first, src_count, cuts + k0, ng, static_cast<qd_c32 *>(iq_d), QD_MEM_DEVICE,
                                         options, stream, false))
            return rc;
        goffs.assign(offs.begin() + k0, offs.begin() + g.second + 1);
        uint8_t *out_d = out;                            // a device out is written in place, at the list's own offsets
        if (!out_dev) {
            void *o = nullptr;
            if (const int rc = ws.get(1, bytes, &o)) return rc;
            out_d = static_cast<uint8_t *>(o);
            for (uint64_t &v : goffs) v -= offs[k0];
        }
        if (const int rc = symbols_on_device(*desc, static_cast<const float2 *>(iq_d), 0, segs.data() + k0, ng, goffs.data(), out_d, ws, st)) return rc;
        if (!out_dev) {
            HIPCHK(hipMemcpyAsync(out + offs[k0], out_d, bytes, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    return QD_OK;
}

int qd_device_alloc(size_t bytes, void **ptr) {
    if (!ptr) return fail(QD_ERR_INVALID, "NULL argument");
    *ptr = nullptr;
    if (bytes == 0) return QD_OK;
    HIPCHK(hipMalloc(ptr, bytes));
    return QD_OK;
}

int qd_device_free(void *ptr) {
    if (ptr) HIPCHK(hipFree(ptr));
    return QD_OK;
}

int qd_device_copy(void *dst, int dst_mem, const void *src, int src_mem, size_t bytes) {
    if (bytes == 0) return QD_OK;
    if (!dst || !src) return fail(QD_ERR_INVALID, "NULL buffer");
    if ((dst_mem != QD_MEM_HOST && dst_mem != QD_MEM_DEVICE) || (src_mem != QD_MEM_HOST && src_mem != QD_MEM_DEVICE))
        return fail(QD_ERR_INVALID, "unknown memory kind");
    const hipMemcpyKind kind = dst_mem == QD_MEM_DEVICE ? (src_mem == QD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                                                        : (src_mem == QD_MEM_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost);
    HIPCHK(hipMemcpy(dst, src, bytes, kind));
    return QD_OK;
}

int qd_gen(const int64_t *cos_hz, size_t n_cos, uint64_t sample_rate, uint64_t first, size_t n, qd_c32 *out, int mem) {
    if (!cos_hz || n_cos == 0) return fail(QD_ERR_INVALID, "cos cannot be empty (src/gen.rs:18)");
    if (sample_rate == 0) return fail(QD_ERR_INVALID, "sample rate may not be zero (src/gen.rs:19)");
    if (n == 0) return QD_OK;
    if (!out) return fail(QD_ERR_INVALID, "NULL buffer");
    const hipStream_t st = g_stream;
    WsLease ws(st);
    if (ws.rc) return ws.rc;
    void *dc = nullptr;
    int rc = ws.get(2, n_cos * 8, &dc); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dc, cos_hz, n_cos * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));              // the tone list is the caller's array
    float2 *o = reinterpret_cast<float2 *>(out);
    if (mem != QD_MEM_DEVICE) { void *dout = nullptr; rc = ws.get(1, n * 8, &dout); if (rc) return rc; o = static_cast<float2 *>(dout); }
    size_t blocks = (n + 255) / 256; if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_gen, dim3((uint32_t)blocks), dim3(256), 0, st, static_cast<const int64_t *>(dc), (uint32_t)n_cos, sample_rate, first, n, o);
    HIPCHK(hipGetLastError());
    if (mem != QD_MEM_DEVICE) HIPCHK(hipMemcpyAsync(out, o, n * 8, hipMemcpyDeviceToHost, st));
    return finish_call(mem, st);
}

}  // extern "C"
