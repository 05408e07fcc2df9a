// qd_mean.h — average-trace rows of norms rows (qd_plan_mean): k_mean folds a batch of the norms sink's windows,
// each group of `pool` consecutive windows per bin, into EXACT fixed-point sums; mean_finish_cell rounds a cell once into its f64 sum and
// its f32 mean.  qd_mean_fold / qd_mean_finish (quadrs_hip.hip) are the CPU twins and use the same two functions.
//
// A floating-point sum depends on its order; an integer sum does not.  A norm is a non-negative f32: a 24-bit integer times a power of
// two, 277 bits over the whole finite range.  A cell is nine limbs L[0..8] in units of 2^-149, 32 payload bits each in a u64 so that
// carries are deferred (2^31 values a cell at most: no limb passes 2^63), and a count word: finite values + (+inf values << 32).  Every
// word is an integer sum, so neither the split of the windows over lanes, workgroups, batches and launches nor the order the atomics
// arrive in changes a bit; the cell is rounded once, at the end.
#ifndef QD_MEAN_H
#define QD_MEAN_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QD_MEAN_HD __host__ __device__
#else
#define QD_MEAN_HD
#endif

namespace qd {

constexpr int kMeanWords = 10;                   // QD_MEAN_WORDS: limbs 0..8, count word 9
constexpr int kMeanLimbs = 9;
constexpr uint64_t kMeanMaxCount = 1ull << 31;   // values a cell may hold
constexpr uint32_t kMeanNanBits = 0x7fc00000u;   // the mean of no values

// One value as the two limb addends and the count addend: L[j] += lo, L[j + 1] += hi, word 9 += cnt.  The sign bit is dropped, a NaN
// adds nothing anywhere, +inf only counts (in the upper half of the count word).
struct MeanTerm { uint32_t j, lo, hi; uint64_t cnt; };
QD_MEAN_HD inline MeanTerm mean_term(uint32_t bits) {
    bits &= 0x7fffffffu;
    const uint32_t e = bits >> 23;
    uint32_t m = bits & 0x7fffffu;
    if (e) m |= 1u << 23;
    if (e == 255) m = 0;
    const uint32_t s = (e ? e : 1u) - 1u;
    const uint64_t v = (uint64_t)m << (s & 31);                         // 55 bits at most
    MeanTerm t;
    t.j = s >> 5; t.lo = (uint32_t)v; t.hi = (uint32_t)(v >> 32);
    t.cnt = e < 255 ? 1ull : (bits == 0x7f800000u ? 1ull << 32 : 0ull);
    return t;
}

// acc[0..9] += one value.  The limb index is data dependent: an unrolled select over the nine limbs keeps them in registers.
QD_MEAN_HD inline void mean_add(uint64_t *acc, uint32_t bits) {
    const MeanTerm t = mean_term(bits);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)kMeanLimbs; ++k) acc[k] += k == t.j ? t.lo : (k == t.j + 1 ? t.hi : 0u);
    acc[9] += t.cnt;
}

QD_MEAN_HD inline int mean_clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// The leading 64 bits of the integer I[N-1..0] of N 32-bit limbs (I[N-1] the most significant): top has bit 63 set unless I is 0, `bits`
// is I's bit length and sticky says whether any bit below the 64 is set.  Fixed trip count, no indexed store: it unrolls into registers.
template <int N>
QD_MEAN_HD inline void limbs_leading(const uint32_t *I, uint64_t *top, bool *sticky, int *bits) {
    uint64_t t = 0;
    uint32_t nxt = 0;
    int low = 0;
    bool have = false, st = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = N - 1; k >= 0; --k) {
        if ((t >> 32) == 0) { t = (t << 32) | I[k]; low = k; }
        else if (!have) { nxt = I[k]; have = true; }
        else st = st || I[k] != 0;
    }
    if (t == 0) { *top = 0; *sticky = false; *bits = 0; return; }
    const int lz = mean_clz64(t);                                        // >= 32 only when every limb was taken in: nxt is 0 then
    const uint64_t n64 = (uint64_t)nxt << lz;
    *top = (t << lz) | (n64 >> 32);
    *sticky = st || (uint32_t)n64 != 0;
    *bits = 64 - lz + 32 * low;
}
// the mean's 320-bit integers I[9..0]
QD_MEAN_HD inline void mean_leading(const uint32_t *I, uint64_t *top, bool *sticky, int *bits) { limbs_leading<kMeanWords>(I, top, sticky, bits); }

// A cell's words into its three results, each rounded once, to nearest, ties to even:
//   count  finite + inf values;  none: sum 0.0, mean the quiet NaN 0x7fc00000;  any +inf: sum and mean +inf
//   sum    the exact sum S as f64: the leading 53 bits of I plus a sticky bit over everything below
//   mean   S / count as f32: long division of I by count limb by limb, the quotient's leading 24 bits rounded with a sticky bit of the
//          lower quotient bits and the remainder; a quotient of 24 bits or fewer IS the f32's bit pattern (subnormal quantum 2^-149,
//          exponent field 1 from 2^23 on) and is rounded by comparing the remainder with count / 2.
QD_MEAN_HD inline void mean_finish_cell(const uint64_t *acc, uint32_t *mean_bits, double *sum, uint32_t *count) {
    const uint64_t n_inf = acc[9] >> 32, c = (acc[9] & 0xffffffffull) + n_inf;
    *count = (uint32_t)c;
    if (c == 0) { *mean_bits = kMeanNanBits; *sum = 0.0; return; }
    if (n_inf) { *mean_bits = 0x7f800000u; *sum = INFINITY; return; }
    uint32_t I[kMeanWords];
    uint64_t carry = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kMeanLimbs; ++k) { carry += acc[k]; I[k] = (uint32_t)carry; carry >>= 32; }
    I[9] = (uint32_t)carry;                                              // below 2^22: the sum is below 2^31 2^128
    uint64_t top; bool sticky; int bits;
    mean_leading(I, &top, &sticky, &bits);
    {
        uint64_t q = top >> 11;
        const uint64_t r = top & 0x7ffull;
        if (r > 0x400ull || (r == 0x400ull && (sticky || (q & 1)))) ++q;
        *sum = ldexp((double)q, bits - 53 - 149);                        // exact: q <= 2^53, the result is a normal f64
    }
    uint32_t Q[kMeanWords];
    uint64_t rem = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = kMeanWords - 1; k >= 0; --k) {
        const uint64_t cur = (rem << 32) | I[k];
        if (c == 1 || cur < c) { Q[k] = c == 1 ? I[k] : 0u; rem = c == 1 ? 0 : cur; }
        else { const uint64_t d = cur / c; Q[k] = (uint32_t)d; rem = cur - d * c; }
    }
    mean_leading(Q, &top, &sticky, &bits);
    if (bits <= 24) {
        const uint32_t q = bits ? (uint32_t)(top >> (64 - bits)) : 0u;
        *mean_bits = q + ((2 * rem > c || (2 * rem == c && (q & 1))) ? 1u : 0u);
    } else {
        const uint32_t q = (uint32_t)(top >> 40);
        const uint64_t r = top & 0xffffffffffull, half = 1ull << 39;
        sticky = sticky || rem != 0;
        *mean_bits = ((uint32_t)(bits - 24) << 23) + q + ((r > half || (r == half && (sticky || (q & 1)))) ? 1u : 0u);
    }
}

// the mean's cell for the limb fold (qd_limbs.h)
struct MeanCell {
    static constexpr int kWords = kMeanWords;
    struct Out { float *mean; double *sum; uint32_t *count; };                          // R x W each; any may be nullptr
    QD_MEAN_HD static void add(uint64_t *acc, uint32_t bits) { mean_add(acc, bits); }
#if defined(__HIPCC__)
    __device__ static void round_to(const uint64_t *acc, const Out &out, uint64_t at) {
        uint32_t mb, cnt; double s;
        mean_finish_cell(acc, &mb, &s, &cnt);
        if (out.mean) out.mean[at] = __uint_as_float(mb);
        if (out.sum) out.sum[at] = s;
        if (out.count) out.count[at] = cnt;
    }
#endif
};

}  // namespace qd

#if defined(__HIPCC__)
#include "qd_limbs.h"

namespace qd {

// k_mean is the limb fold (qd_limbs.h) with ten words a cell on pool_geometry: V = 4 bins a lane (one 16-byte load a window), V = 1 below W = 4.
template <int V>
__global__ __launch_bounds__(kPoolThreads) void k_mean(const LimbParams<MeanCell> M) { limb_fold<MeanCell, V, kPoolThreads * V>(M); }

__global__ __launch_bounds__(kPoolThreads) void k_mean_finish(const unsigned long long *accg, const uint32_t *flags, uint64_t cells, uint64_t r_base,
                                                              uint64_t n_rows, uint32_t W, const MeanCell::Out out) {
    limb_finish<MeanCell>(accg, flags, cells, r_base, n_rows, W, out);
}

}  // namespace qd
#endif  // __HIPCC__
#endif
