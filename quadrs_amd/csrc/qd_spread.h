// qd_spread.h — deviation-trace rows of norms rows (qd_plan_spread): k_spread folds a batch of the norms sink's
// windows, each group of `pool` consecutive windows per bin, into the EXACT fixed-point sum AND sum of squares of one cell;
// spread_finish_cell rounds a cell once into its standard deviation (f32), its sum of squared deviations (f64) and, through
// mean_finish_cell and power_finish_cell, its mean and its RMS.  qd_spread_fold / qd_spread_finish (quadrs_hip.hip) are the CPU twins and
// use the same functions.
//
// A cell is qd_mean.h's nine limbs (words 0-8, units of 2^-149), qd_power.h's eighteen (words 9-26, units of 2^-298) and their one
// count word (word 27).  With n values, A their carried sum and B their carried sum of squares, D = n B - A^2 is an integer below 2^616
// (twenty limbs of 32 bits), never negative, and the deviation is sqrt(D) / n: a difference of two exact integers, so nothing cancels.
#ifndef QD_SPREAD_H
#define QD_SPREAD_H

#include "qd_power.h"

namespace qd {

constexpr int kSpreadWords = 28;                 // QD_SPREAD_WORDS: mean limbs 0..8, power limbs 9..26, count word 27
constexpr int kSpreadDLimbs = 20;                // 32-bit limbs of n B, A^2, D and 4 D
constexpr int kSpreadQLimbs = 23;                // D 2^96 / n
constexpr uint64_t kSpreadNanBits64 = 0x7ff8000000000000ull;

// which results spread_finish_cell works out (count always)
enum : uint32_t { kSpreadStd = 1u, kSpreadSsd = 2u, kSpreadMean = 4u, kSpreadRms = 8u, kSpreadAll = 15u };
struct SpreadRounded { uint32_t std_bits, mean_bits, rms_bits, count; double ssd; };

// acc[0..27] += one value: mean_term's two addends and power_term's three.  The limb indices are data dependent: unrolled selects over
// the nine and the eighteen limbs keep the cell in registers.
QD_MEAN_HD inline void spread_add(uint64_t *acc, uint32_t bits) {
    const MeanTerm t = mean_term(bits);
    const PowerTerm p = power_term(bits);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)kMeanLimbs; ++k) acc[k] += k == t.j ? t.lo : (k == t.j + 1 ? t.hi : 0u);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)kPowerLimbs; ++k) acc[9 + k] += k == p.j ? p.w0 : (k == p.j + 1 ? p.w1 : (k == p.j + 2 ? p.w2 : 0u));
    acc[27] += t.cnt;
}

// a b as 128 bits
struct Spread128 { uint32_t x0, x1, x2, x3; };
QD_MEAN_HD inline Spread128 spread_mul128(uint64_t a, uint64_t b) {
    const uint64_t a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
    const uint64_t hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    Spread128 x;
    x.x0 = (uint32_t)p00; x.x1 = (uint32_t)mid; x.x2 = (uint32_t)hi; x.x3 = (uint32_t)(hi >> 32);
    return x;
}

// The sign of J - (X << sh) for the integer J[19..0] and sh <= 508: power_cmp one word wider.  The 160 bits of J from bit sh on are picked
// with an unrolled select, what lies above them must be zero and what lies below them decides equality: fixed trip count, no indexed store.
QD_MEAN_HD inline int spread_cmp(const uint32_t *J, Spread128 X, uint32_t sh) {
    const uint32_t j = sh >> 5, t = sh & 31;
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, above = 0, below = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < (uint32_t)kSpreadDLimbs; ++k) {
        w0 = k == j ? J[k] : w0; w1 = k == j + 1 ? J[k] : w1; w2 = k == j + 2 ? J[k] : w2; w3 = k == j + 3 ? J[k] : w3; w4 = k == j + 4 ? J[k] : w4;
        above |= k > j + 4 ? J[k] : 0u;
        below |= k < j ? J[k] : 0u;
    }
    below |= w0 & ((1u << t) - 1u);
    const uint32_t h0 = (uint32_t)((((uint64_t)w1 << 32) | w0) >> t), h1 = (uint32_t)((((uint64_t)w2 << 32) | w1) >> t),
                   h2 = (uint32_t)((((uint64_t)w3 << 32) | w2) >> t), h3 = (uint32_t)((((uint64_t)w4 << 32) | w3) >> t), h4 = w4 >> t;
    if (above | h4) return 1;
    if (h3 != X.x3) return h3 > X.x3 ? 1 : -1;
    if (h2 != X.x2) return h2 > X.x2 ? 1 : -1;
    if (h1 != X.x1) return h1 > X.x1 ? 1 : -1;
    if (h0 != X.x0) return h0 > X.x0 ? 1 : -1;
    return below ? 1 : 0;
}

// the sign of 4 D - n^2 (2 (M << s))^2: where the f32 of pattern p, times n, stands against the root of D
QD_MEAN_HD inline int spread_side(const uint32_t *J, uint32_t p, uint64_t n2) {
    uint64_t M; uint32_t s;
    power_units(p, &M, &s);
    return spread_cmp(J, spread_mul128(4 * M * M, n2), 2 * s);
}

QD_MEAN_HD inline double spread_f64_of_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }

// The deviation half of a cell of n >= 2 finite values: D = n B - A^2 from the carried sums, then
//   ssd   D / n, the exact rational, as f64: long division of D 2^96 by n limb by limb (the quotient then has 66 bits at least), its
//         leading 53 bits rounded with a sticky bit over the lower quotient bits and the remainder
//   std   sqrt(D) / n as f32.  In units of 2^-149 every f32 is an integer M << s.  A candidate pattern comes from an f64 estimate and is
//         walked (two steps; the estimate is one off at the most) until its f32 `lo` and the next one `up` hold lo^2 n^2 <= D < up^2 n^2;
//         then 4 D against n^2 (lo + up)^2 says which of the two is nearer, and the even pattern wins a tie.  The estimate only starts
//         the walk: every decision is an integer comparison (spread_cmp).
// Kept out of spread_finish_cell so that the mean's and the power's limbs are dead before D's twenty are formed.
QD_MEAN_HD inline void spread_deviation(const uint64_t *acc, uint32_t n, uint32_t want, uint32_t *std_bits, double *ssd) {
    uint32_t A[kMeanWords], B[kPowerSumLimbs];
    uint64_t carry = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kMeanLimbs; ++k) { carry += acc[k]; A[k] = (uint32_t)carry; carry >>= 32; }
    A[9] = (uint32_t)carry;
    carry = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kPowerLimbs; ++k) { carry += acc[9 + k]; B[k] = (uint32_t)carry; carry >>= 32; }
    B[18] = (uint32_t)carry;
    // n B: below 2^31 2^585
    uint32_t D[kSpreadDLimbs];
    carry = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kPowerSumLimbs; ++k) { carry += (uint64_t)B[k] * n; D[k] = (uint32_t)carry; carry >>= 32; }
    D[19] = (uint32_t)carry;
    // A^2: A is below 2^308
    uint32_t P[kSpreadDLimbs];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < kSpreadDLimbs; ++k) P[k] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < kMeanWords; ++i) {
        carry = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < kMeanWords; ++j) {
            const uint64_t t = (uint64_t)A[i] * A[j] + P[i + j] + carry;                // at most 2^64 - 1
            P[i + j] = (uint32_t)t; carry = t >> 32;
        }
        P[i + kMeanWords] = (uint32_t)carry;
    }
    // D = n B - A^2: never negative (Cauchy-Schwarz)
    uint32_t any = 0;
    {
        uint64_t borrow = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < kSpreadDLimbs; ++k) {
            const uint64_t t = (uint64_t)D[k] - P[k] - borrow;
            D[k] = (uint32_t)t; borrow = (t >> 32) & 1u;
            any |= D[k];
        }
    }
    *std_bits = 0; *ssd = 0.0;
    if (!any) return;                                                    // all values equal
    double S;
    {
        uint32_t Q[kSpreadQLimbs];
        uint64_t rem = 0;
        const uint64_t c = n;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = kSpreadQLimbs - 1; k >= 0; --k) {
            const uint64_t cur = (rem << 32) | (k >= 3 ? D[k >= 3 ? k - 3 : 0] : 0u);
            if (cur < c) { Q[k] = 0u; rem = cur; }
            else { const uint64_t d = cur / c; Q[k] = (uint32_t)d; rem = cur - d * c; }
        }
        uint64_t top; bool sticky; int bits;
        limbs_leading<kSpreadQLimbs>(Q, &top, &sticky, &bits);
        sticky = sticky || rem != 0;
        uint64_t q = top >> 11;
        const uint64_t r = top & 0x7ffull;
        if (r > 0x400ull || (r == 0x400ull && (sticky || (q & 1)))) ++q;
        S = ldexp((double)q, bits - 53 - 298 - 96);                     // exact: q <= 2^53, the result is a normal f64 (2^-329 ... < 2^287)
    }
    *ssd = S;
    if (!(want & kSpreadStd)) return;
    // the candidate: sqrt(S / n), cut to an f32 pattern with integers (no f32 rounding mode or denormal mode enters); below 2^-149: 0
    uint32_t p = 0;
    {
        const double x = sqrt(S / (double)n);
        uint64_t xb;
        memcpy(&xb, &x, 8);
        const int E = (int)(xb >> 52) - 1023;
        const uint64_t f = (xb & 0xfffffffffffffull) | (1ull << 52);
        if (E >= -126) p = ((uint32_t)(E + 127) << 23) | ((uint32_t)(f >> 29) & 0x7fffffu);
        else if (E >= -149) p = (uint32_t)(f >> (52 - (E + 149)));
        if (p > 0x7f7fffffu) p = 0x7f7fffffu;
    }
    uint32_t J[kSpreadDLimbs];                                           // 4 D: below 2^618
    J[0] = D[0] << 2;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 1; k < kSpreadDLimbs; ++k) J[k] = (D[k] << 2) | (D[k - 1] >> 30);
    const uint64_t n2 = (uint64_t)n * n;                                 // at most 2^62
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int step = 0; step < 2; ++step) {
        if (spread_side(J, p, n2) < 0) --p;                              // lo^2 n^2 > D (never at p == 0)
        else if (p < 0x7f7fffffu && spread_side(J, p + 1, n2) >= 0) ++p; // up^2 n^2 <= D
    }
    uint64_t M; uint32_t s;
    power_units(p, &M, &s);
    const int half = spread_cmp(J, spread_mul128((2 * M + 1) * (2 * M + 1), n2), 2 * s);   // lo + up is (2 M + 1) << s
    *std_bits = p + ((half > 0 || (half == 0 && (p & 1))) ? 1u : 0u);
}

// A cell's words into its results, each rounded once, to nearest, ties to even; `want` names the ones to work out (kSpread*):
//   count  finite + inf values
//   mean   mean_finish_cell on words 0-8 and the count word;  rms  power_finish_cell on words 9-26 and the count word
//   std, ssd   none: std the quiet NaN 0x7fc00000, ssd 0.0;  any +inf: both the quiet NaN (the deviation of a set that holds an infinity
//          is undefined);  one value: +0 and 0.0;  else spread_deviation
QD_MEAN_HD inline void spread_finish_cell(const uint64_t *acc, uint32_t want, SpreadRounded *out) {
    const uint64_t n_inf = acc[27] >> 32, c64 = (acc[27] & 0xffffffffull) + n_inf;
    const uint32_t c = (uint32_t)c64;
    out->count = c;
    out->mean_bits = out->rms_bits = out->std_bits = kMeanNanBits;
    out->ssd = 0.0;
    if (c == 0) return;
    if (want & kSpreadMean) {
        uint64_t m[kMeanWords];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < kMeanLimbs; ++k) m[k] = acc[k];
        m[9] = acc[27];
        double s; uint32_t cnt;
        mean_finish_cell(m, &out->mean_bits, &s, &cnt);
    }
    if (want & kSpreadRms) {
        uint64_t q[kPowerWords];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < kPowerLimbs; ++k) q[k] = acc[9 + k];
        q[18] = acc[27];
        double s; uint32_t cnt;
        power_finish_cell(q, &out->rms_bits, &s, &cnt);
    }
    if (n_inf) { out->ssd = spread_f64_of_bits(kSpreadNanBits64); return; }
    out->std_bits = 0;
    if (c == 1 || !(want & (kSpreadStd | kSpreadSsd))) return;
    spread_deviation(acc, c, want, &out->std_bits, &out->ssd);
}

// the spread's cell for the host path the three sinks share (quadrs_hip.hip); k_spread has its own parameters below
struct SpreadCell {
    static constexpr int kWords = kSpreadWords;
    struct Out {
        float *std; double *ssd; uint32_t *count; float *mean; float *rms;              // R x W each; any may be nullptr
        uint32_t want;                                                                  // kSpread* of the outputs that are not nullptr
    };
    QD_MEAN_HD static void add(uint64_t *acc, uint32_t bits) { spread_add(acc, bits); }
};

}  // namespace qd

#if defined(__HIPCC__)
namespace qd {

// k_spread folds as limb_fold (qd_limbs.h) does, with twenty-eight words a cell on power_geometry's V = 1 column layout, and keeps its
// own text: entered through the shared body its legs at one row of everything measured 0.4-0.8 % above this text's (one MI355X,
// ROCm 7.2, October 2026) and the cause was not found.  A change to limb_fold's meeting or row endings has to
// be made here too.
// Twenty-eight u64 a bin are 56 VGPRs a bin: one bin a lane is the only form (four would be 224 VGPRs of accumulator alone).
struct SpreadParams {
    const float *norms;                          // the batch's windows, nw x W
    PieceGeometry G;
    float *std; double *ssd; uint32_t *count; float *mean; float *rms;   // R x W each; any may be nullptr
    unsigned long long *acc;                     // planar limbs, kSpreadWords x cells
    uint32_t *flags;                             // acc_rows: the row went through the accumulator
    uint64_t r_base, acc_rows, cells;            // acc_rows 0: the host found that this launch cuts no row
    uint32_t want;                               // kSpread* of the outputs that are not nullptr
};

__device__ inline void spread_store(const SpreadRounded &c, uint64_t o, float *std, double *ssd, uint32_t *count, float *mean, float *rms) {
    if (std) std[o] = __uint_as_float(c.std_bits);
    if (ssd) ssd[o] = c.ssd;
    if (count) count[o] = c.count;
    if (mean) mean[o] = __uint_as_float(c.mean_bits);
    if (rms) rms[o] = __uint_as_float(c.rms_bits);
}

__global__ __launch_bounds__(kPoolThreads) void k_spread(const SpreadParams M) {
    __shared__ unsigned long long s_meet[kPoolThreads];
    const PieceGeometry &P = M.G;
    const uint32_t tid = threadIdx.x;
    const uint32_t grp = tid / P.lanes_per_win;
    const uint32_t lcol = tid % P.lanes_per_win;                                       // the lane's bin inside the slab
    const PieceLane l = piece_lane(P, blockIdx.x, grp);

    uint64_t acc[kSpreadWords];
#pragma unroll
    for (int j = 0; j < kSpreadWords; ++j) acc[j] = 0;

    walk_piece<1>(M.norms + (l.wa - P.g0) * P.W + (uint64_t)l.slab * P.cols + lcol, l.wa, l.wb, P.W, [&](int, uint32_t bits) { spread_add(acc, bits); });

    // the pieces of this workgroup that share the row r meet in the LDS slot of the first of them, one word at a time
    if (P.spr > 1 && P.pieces_per_group > 1) {
        const uint32_t slot = l.lead * P.lanes_per_win + lcol;
        s_meet[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSpreadWords; ++j) {
            if (l.active && acc[j]) atomicAdd(&s_meet[slot], (unsigned long long)acc[j]);
            __syncthreads();
            // slot tid is read and cleared by lane tid alone
            acc[j] = s_meet[tid]; s_meet[tid] = 0;
            __syncthreads();
        }
    }
    if (!l.active || l.lead != grp) return;
    const uint64_t col = (uint64_t)l.slab * P.cols + lcol;
    if (l.whole(P)) {
        SpreadRounded c;
        spread_finish_cell(acc, M.want, &c);
        spread_store(c, l.r * P.W + col, M.std, M.ssd, M.count, M.mean, M.rms);
    } else {
        const uint64_t ra = l.r - M.r_base, cell = ra * P.W + col;
        if (ra >= M.acc_rows) return;                                    // never past the accumulator
        if (lcol == 0) M.flags[ra] = 1u;
#pragma unroll
        for (int j = 0; j < kSpreadWords; ++j)
            if (acc[j]) atomicAdd(&M.acc[(uint64_t)j * M.cells + cell], (unsigned long long)acc[j]);
    }
}

// the flagged rows of the accumulator, rows [r_base, r_base + n_rows) of the range, into the outputs: one lane per cell
__global__ __launch_bounds__(kPoolThreads) void k_spread_finish(const unsigned long long *accg, const uint32_t *flags, uint64_t cells, uint64_t r_base,
                                                                uint64_t n_rows, uint32_t W, uint32_t want, float *std, double *ssd, uint32_t *count,
                                                                float *mean, float *rms) {
    const uint64_t c = (uint64_t)blockIdx.x * kPoolThreads + threadIdx.x;
    if (c >= n_rows * W) return;
    if (!flags[c / W]) return;
    uint64_t acc[kSpreadWords];
#pragma unroll
    for (int j = 0; j < kSpreadWords; ++j) acc[j] = accg[(uint64_t)j * cells + c];
    SpreadRounded r;
    spread_finish_cell(acc, want, &r);
    spread_store(r, r_base * W + c, std, ssd, count, mean, rms);
}

}  // namespace qd
#endif  // __HIPCC__
#endif
