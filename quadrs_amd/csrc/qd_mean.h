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

}  // namespace qd

#if defined(__HIPCC__)
#include "qd_pool.h"

namespace qd {

// k_mean runs on k_pool's geometry (pool_geometry, qd_pool.h; the rule is qd_pieces.h) with k_pool's window walker (walk_piece) and reads
// the carrier once.  A lane owns V bins down a piece and adds each value into its own nine limbs and count word, in registers.  Pieces of a workgroup that share a row meet in LDS, word by word (one u64 per bin: 8 KiB),
// with u64 LDS adds into the slot of the first of them.  A row then ends in one of two ways:
//   whole   all of the row's windows lie in this batch and all of its pieces in this workgroup (PieceLane::whole): the leader rounds
//           the cells and stores mean / sum / count; no global accumulator is touched.
//   cut     every other row (cut by a batch seam, or split over workgroups because the rows are few): the leader adds its non-zero
//           words with 64-bit global atomicAdd — one per word per workgroup — into the limb accumulator and raises the row's flag;
//           k_mean_finish, one lane per cell, rounds the flagged rows once all of their batches are through.
// The limb accumulator is planar (word k of cell c at k cells + c, cells = acc_rows W, so the lanes of a wave touch consecutive words)
// and holds rows [r_base, r_base + acc_rows) of the range.
// Workspace rule (qd_plan_mean): the accumulator is at most max(2 chunk_bytes, 80 W bytes), whatever R is.  Batches end on multiples of
// pool whenever pool <= chunk windows, so rows of small pools are whole and need no accumulator; a batch that can cut rows is clipped to
// the rows the accumulator holds, and when its rows pass the accumulator's end the span is finished, the accumulator zeroed and moved.
struct MeanParams {
    const float *norms;                          // the batch's windows, nw x W
    PieceGeometry G;
    float *mean; double *sum; uint32_t *count;   // R x W each; any may be nullptr
    unsigned long long *acc;                     // planar limbs, kMeanWords x cells
    uint32_t *flags;                             // acc_rows: the row went through the accumulator
    uint64_t r_base, acc_rows, cells;           // acc_rows 0: the host found that this launch cuts no row
};

template <int V>
__global__ __launch_bounds__(kPoolThreads) void k_mean(const MeanParams M) {
    __shared__ unsigned long long s_meet[kPoolSlabCols];
    const PieceGeometry &P = M.G;
    const uint32_t tid = threadIdx.x;
    const uint32_t grp = tid / P.lanes_per_win;
    const uint32_t lcol = (tid % P.lanes_per_win) * V;                                 // the lane's first bin inside the slab
    const PieceLane l = piece_lane(P, blockIdx.x, grp);

    uint64_t acc[V][kMeanWords];
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
        for (int j = 0; j < kMeanWords; ++j) acc[i][j] = 0;

    walk_piece<V>(M.norms + (l.wa - P.g0) * P.W + (uint64_t)l.slab * P.cols + lcol, l.wa, l.wb, P.W, [&](int i, uint32_t bits) { mean_add(acc[i], bits); });

    // the pieces of this workgroup that share the row r meet in the LDS slot of the first of them, one word at a time; with one piece
    // a row (spr == 1) or one piece a workgroup every lane group leads its own row and nothing meets
    if (P.spr > 1 && P.pieces_per_group > 1) {
        const uint32_t slot = l.lead * P.lanes_per_win * V + lcol;
#pragma unroll
        for (int i = 0; i < V; ++i) s_meet[tid * V + i] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kMeanWords; ++j) {
            if (l.active) {
#pragma unroll
                for (int i = 0; i < V; ++i)
                    if (acc[i][j]) atomicAdd(&s_meet[slot + i], (unsigned long long)acc[i][j]);
            }
            __syncthreads();
            // slot tid V + i is read and cleared by lane tid alone
#pragma unroll
            for (int i = 0; i < V; ++i) { acc[i][j] = s_meet[tid * V + i]; s_meet[tid * V + i] = 0; }
            __syncthreads();
        }
    }
    if (!l.active || l.lead != grp) return;
    const uint64_t col = (uint64_t)l.slab * P.cols + lcol;
    if (l.whole(P)) {
        const uint64_t o = l.r * P.W + col;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            uint32_t mb, cnt; double s;
            mean_finish_cell(acc[i], &mb, &s, &cnt);
            if (M.mean) M.mean[o + i] = __uint_as_float(mb);
            if (M.sum) M.sum[o + i] = s;
            if (M.count) M.count[o + i] = cnt;
        }
    } else {
        const uint64_t ra = l.r - M.r_base, cell = ra * P.W + col;
        if (ra >= M.acc_rows) return;                                    // never past the accumulator
        if (lcol == 0) M.flags[ra] = 1u;
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int j = 0; j < kMeanWords; ++j)
                if (acc[i][j]) atomicAdd(&M.acc[(uint64_t)j * M.cells + cell + i], (unsigned long long)acc[i][j]);
    }
}

// the flagged rows of the accumulator, rows [r_base, r_base + n_rows) of the range, into the outputs: one lane per cell
__global__ __launch_bounds__(kPoolThreads) void k_mean_finish(const unsigned long long *accg, const uint32_t *flags, uint64_t cells, uint64_t r_base,
                                                              uint64_t n_rows, uint32_t W, float *mean, double *sum, uint32_t *count) {
    const uint64_t c = (uint64_t)blockIdx.x * kPoolThreads + threadIdx.x;
    if (c >= n_rows * W) return;
    if (!flags[c / W]) return;
    uint64_t acc[kMeanWords];
#pragma unroll
    for (int j = 0; j < kMeanWords; ++j) acc[j] = accg[(uint64_t)j * cells + c];
    uint32_t mb, cnt; double s;
    mean_finish_cell(acc, &mb, &s, &cnt);
    const uint64_t o = r_base * W + c;
    if (mean) mean[o] = __uint_as_float(mb);
    if (sum) sum[o] = s;
    if (count) count[o] = cnt;
}

}  // namespace qd
#endif  // __HIPCC__
#endif
