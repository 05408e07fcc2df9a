// qd_power.h — RMS-trace rows of norms rows (qd_plan_power): k_power folds a batch of the norms sink's windows,
// each group of `pool` consecutive windows per bin, into EXACT fixed-point sums of squares; power_finish_cell rounds a cell once into its
// f64 sum of squares and its f32 root mean square.  qd_power_fold / qd_power_finish (quadrs_hip.hip) are the CPU twins and use the same
// functions.
//
// The technique is qd_mean.h's with a wider cell.  The square of a non-negative f32 is a 48-bit integer times an even power of two, 554
// bits over the whole finite range: eighteen limbs L[0..17] in units of 2^-298, 32 payload bits each in a u64 so that carries are
// deferred (2^31 values a cell at most: no limb passes 2^63; the carried sum stays below 2^585, nineteen limbs of 32 bits), and a count
// word: finite values + (+inf values << 32).  Every word is an integer sum, so no split and no arrival order changes a bit.
#ifndef QD_POWER_H
#define QD_POWER_H

#include <string.h>

#include "qd_mean.h"

namespace qd {

constexpr int kPowerWords = 19;                  // QD_POWER_WORDS: limbs 0..17, count word 18
constexpr int kPowerLimbs = 18;
constexpr int kPowerSumLimbs = 19;               // 32-bit limbs of a carried sum, and of four times it

// One value as the three limb addends and the count addend: L[j] += w0, L[j + 1] += w1, L[j + 2] += w2, word 18 += cnt.  The sign bit is
// dropped, a NaN adds nothing anywhere, +inf only counts (in the upper half of the count word).
struct PowerTerm { uint32_t j, w0, w1, w2; uint64_t cnt; };
QD_MEAN_HD inline PowerTerm power_term(uint32_t bits) {
    bits &= 0x7fffffffu;
    const uint32_t e = bits >> 23;
    uint32_t m = bits & 0x7fffffu;
    if (e) m |= 1u << 23;
    if (e == 255) m = 0;
    const uint32_t s = (e ? e : 1u) - 1u, sh = 2 * s, t = sh & 31;
    const uint64_t q = (uint64_t)m * m;                                  // below 2^48; the 79-bit q << t in three pieces
    const uint64_t up = q >> (32 - t);                                   // (q << t) >> 32: t <= 30
    PowerTerm p;
    p.j = sh >> 5; p.w0 = (uint32_t)(q << t); p.w1 = (uint32_t)up; p.w2 = (uint32_t)(up >> 32);
    p.cnt = e < 255 ? 1ull : (bits == 0x7f800000u ? 1ull << 32 : 0ull);
    return p;
}

// acc[0..18] += one value.  The limb index is data dependent: an unrolled select over the eighteen limbs keeps them in registers.
QD_MEAN_HD inline void power_add(uint64_t *acc, uint32_t bits) {
    const PowerTerm p = power_term(bits);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)kPowerLimbs; ++k) acc[k] += k == p.j ? p.w0 : (k == p.j + 1 ? p.w1 : (k == p.j + 2 ? p.w2 : 0u));
    acc[18] += p.cnt;
}

// a c as 96 bits: a below 2^52, c below 2^32
struct Power96 { uint32_t x0, x1, x2; };
QD_MEAN_HD inline Power96 power_mul96(uint64_t a, uint32_t c) {
    const uint64_t p0 = (a & 0xffffffffull) * c, p1 = (a >> 32) * c, t = (p0 >> 32) + p1;
    Power96 x;
    x.x0 = (uint32_t)p0; x.x1 = (uint32_t)t; x.x2 = (uint32_t)(t >> 32);
    return x;
}

// The sign of J - (X << sh) for the integer J[18..0] and sh <= 508.  The 128 bits of J from bit sh on are picked with an unrolled select,
// what lies above them must be zero and what lies below them decides equality: fixed trip count, no indexed store.
QD_MEAN_HD inline int power_cmp(const uint32_t *J, Power96 X, uint32_t sh) {
    const uint32_t j = sh >> 5, t = sh & 31;
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, above = 0, below = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)kPowerSumLimbs; ++k) {
        w0 = k == j ? J[k] : w0; w1 = k == j + 1 ? J[k] : w1; w2 = k == j + 2 ? J[k] : w2; w3 = k == j + 3 ? J[k] : w3;
        above |= k > j + 3 ? J[k] : 0u;
        below |= k < j ? J[k] : 0u;
    }
    below |= w0 & ((1u << t) - 1u);
    const uint32_t h0 = (uint32_t)((((uint64_t)w1 << 32) | w0) >> t), h1 = (uint32_t)((((uint64_t)w2 << 32) | w1) >> t),
                   h2 = (uint32_t)((((uint64_t)w3 << 32) | w2) >> t), h3 = w3 >> t;
    if (above | h3) return 1;
    if (h2 != X.x2) return h2 > X.x2 ? 1 : -1;
    if (h1 != X.x1) return h1 > X.x1 ? 1 : -1;
    if (h0 != X.x0) return h0 > X.x0 ? 1 : -1;
    return below ? 1 : 0;
}

// the f32 of bit pattern p (0 ... 0x7f800000) as the integer M << s in units of 2^-149
QD_MEAN_HD inline void power_units(uint32_t p, uint64_t *M, uint32_t *s) {
    const uint32_t e = p >> 23;
    *M = (p & 0x7fffffu) | (e ? 1u << 23 : 0u);
    *s = (e ? e : 1u) - 1u;
}
// the sign of 4 S - c (M << s)^2: where the f32 M << s stands against the root
QD_MEAN_HD inline int power_side(const uint32_t *J, uint32_t p, uint32_t c) {
    uint64_t M; uint32_t s;
    power_units(p, &M, &s);
    return power_cmp(J, power_mul96(4 * M * M, c), 2 * s);
}

// A cell's words into its three results, each rounded once, to nearest, ties to even:
//   count  finite + inf values;  none: sumsq 0.0, rms the quiet NaN 0x7fc00000;  any +inf: sumsq and rms +inf
//   sumsq  the exact sum of squares S as f64: the leading 53 bits of the carried limbs plus a sticky bit over everything below
//   rms    sqrt(S / count) as f32.  In units of 2^-149 every f32 is an integer and S, in units of 2^-298, is one too.  A candidate
//          pattern comes from an f64 estimate and is walked (two steps; the estimate is one off at the most) until its f32 `lo` and
//          the next one `up` hold lo^2 count <= S < up^2 count; then 4 S against count (lo + up)^2 says which of the two is nearer, and
//          the even pattern wins a tie.  The estimate only starts the walk: every decision is an integer comparison.
QD_MEAN_HD inline void power_finish_cell(const uint64_t *acc, uint32_t *rms_bits, double *sumsq, uint32_t *count) {
    const uint64_t n_inf = acc[18] >> 32, c64 = (acc[18] & 0xffffffffull) + n_inf;
    const uint32_t c = (uint32_t)c64;
    *count = c;
    if (c == 0) { *rms_bits = kMeanNanBits; *sumsq = 0.0; return; }
    if (n_inf) { *rms_bits = 0x7f800000u; *sumsq = INFINITY; return; }
    uint32_t I[kPowerSumLimbs];
    uint64_t carry = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kPowerLimbs; ++k) { carry += acc[k]; I[k] = (uint32_t)carry; carry >>= 32; }
    I[18] = (uint32_t)carry;                                             // below 2^9: the sum is below 2^31 2^554
    uint64_t top; bool sticky; int bits;
    limbs_leading<kPowerSumLimbs>(I, &top, &sticky, &bits);
    double S;
    {
        uint64_t q = top >> 11;
        const uint64_t r = top & 0x7ffull;
        if (r > 0x400ull || (r == 0x400ull && (sticky || (q & 1)))) ++q;
        S = ldexp((double)q, bits - 53 - 298);                           // exact: q <= 2^53, the result is 0 or a normal f64
    }
    *sumsq = S;
    // the candidate: sqrt(S / c), 2^-149 ... < 2^128, cut to an f32 pattern with integers (no f32 rounding mode or denormal mode enters)
    uint32_t p = 0;
    if (S > 0.0) {
        const double x = sqrt(S / (double)c);
        uint64_t xb;
        memcpy(&xb, &x, 8);
        const int E = (int)(xb >> 52) - 1023;
        const uint64_t f = (xb & 0xfffffffffffffull) | (1ull << 52);
        if (E >= -126) p = ((uint32_t)(E + 127) << 23) | ((uint32_t)(f >> 29) & 0x7fffffu);
        else if (E >= -149) p = (uint32_t)(f >> (52 - (E + 149)));
        if (p > 0x7f7fffffu) p = 0x7f7fffffu;
    }
    uint32_t J[kPowerSumLimbs];                                          // 4 S: below 2^587
    J[0] = I[0] << 2;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 1; k < kPowerSumLimbs; ++k) J[k] = (I[k] << 2) | (I[k - 1] >> 30);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int step = 0; step < 2; ++step) {
        if (power_side(J, p, c) < 0) --p;                                // lo^2 c > S (never at p == 0)
        else if (p < 0x7f7fffffu && power_side(J, p + 1, c) >= 0) ++p;   // up^2 c <= S
    }
    uint64_t M; uint32_t s;
    power_units(p, &M, &s);
    const int half = power_cmp(J, power_mul96((2 * M + 1) * (2 * M + 1), c), 2 * s);   // lo + up is (2 M + 1) << s
    *rms_bits = p + ((half > 0 || (half == 0 && (p & 1))) ? 1u : 0u);
}

// the power's cell for the limb fold (qd_limbs.h)
struct PowerCell {
    static constexpr int kWords = kPowerWords;
    struct Out { float *rms; double *sumsq; uint32_t *count; };                         // R x W each; any may be nullptr
    QD_MEAN_HD static void add(uint64_t *acc, uint32_t bits) { power_add(acc, bits); }
#if defined(__HIPCC__)
    __device__ static void round_to(const uint64_t *acc, const Out &out, uint64_t at) {
        uint32_t rb, cnt; double s;
        power_finish_cell(acc, &rb, &s, &cnt);
        if (out.rms) out.rms[at] = __uint_as_float(rb);
        if (out.sumsq) out.sumsq[at] = s;
        if (out.count) out.count[at] = cnt;
    }
#endif
};

}  // namespace qd

#if defined(__HIPCC__)
namespace qd {

// k_power is the limb fold (qd_limbs.h) with nineteen words a cell.  Nineteen u64 a bin are 38 VGPRs a bin, so two forms are built:
// V = 4 bins a lane (one 16-byte load a window, pool_geometry as it stands) and V = 1 (4-byte loads, 256 bins a workgroup);
// power_geometry lays out either.
template <int V>
__global__ __launch_bounds__(kPoolThreads) void k_power(const LimbParams<PowerCell> M) { limb_fold<PowerCell, V, kPoolThreads * V>(M); }

__global__ __launch_bounds__(kPoolThreads) void k_power_finish(const unsigned long long *accg, const uint32_t *flags, uint64_t cells, uint64_t r_base,
                                                               uint64_t n_rows, uint32_t W, const PowerCell::Out out) {
    limb_finish<PowerCell>(accg, flags, cells, r_base, n_rows, W, out);
}

// The launch geometry for the batch [g0, g0 + nw) in the form `form`: pool_geometry for V = 4 (W < 4 is always V = 1); V = 1 has its own
// column layout, 256 bins a workgroup.  Which form: V = 1 won at every width measured, W = 4, 64, 128 and 2048,
// at every pool but one row of everything, so the shipped library launches V = 1 alone; V = 4 lives in development builds.
inline void power_geometry(uint64_t g0, uint64_t nw, uint64_t n_total, uint64_t pool, uint32_t W, int n_cu, int form, PieceGeometry *P, uint64_t *grid, int *V) {
    if (form == 4 && W >= 4) { pool_geometry(g0, nw, n_total, pool, W, n_cu, P, grid, V); return; }
    *V = 1;
    const uint32_t cols = W < (uint32_t)kPoolThreads ? W : (uint32_t)kPoolThreads;
    piece_split(g0, nw, n_total, pool, W, cols, cols, kPoolThreads / cols, kPoolMinSeg, kPoolGroupsPerCu, n_cu, P, grid);
}

}  // namespace qd
#endif  // __HIPCC__
#endif
