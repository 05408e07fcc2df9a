// qd_nco.h — the NCO's f64 arithmetic (src/shift.rs:49-50): table entries and the per-sample rotation, stated once.
//
// Plain C++17 with no HIP types: qd_device.h includes it for every kernel (hipcc and hiprtc), and scripts/nco_host_check.cpp
// compiles the same text with the host compiler to hold it to __float128 (tests/test_nco_rotation_cpu.py).
//
// Reference: place = fl((n as f64) * ratio); mul = (cos(place) as f32, sin(place) as f32).
// A libm-grade f64 sincos per sample costs more f64 issue slots than the chip has at HBM rate, and f64 work also
// lowers the clock the chip holds.  Scheme: the EXACT product X = n*ratio splits as n_r*ratio + j*ratio (n = n_r + j,
// n_r the first sample of a row of ROW samples).  Tables hold cos/sin of those two exact products (each the libm
// sincos of the rounded product, corrected to first order by the product's exactly known rounding residual), so one
// rotation gives cos/sin(X).  The reference's argument is place = fl(X) = X - r with r = fma(n, ratio, -place) the exact
// residual of ITS multiplication (|r| <= ulp(place)/2), so cos(place) = cos(X - r) = C + r*S, sin(place) = S - r*C to
// first order (the dropped r^2/2 is <= 1.1e-16 for |place| < 2^28 rad; beyond that the second-order form is used).
//
// The rotation (C, S) = (rc lc - rs ls, rs lc + rc ls) of the row entry (rc, rs) by the lane entry (lc, ls) takes three
// multiplications, not four: with k = lc (rc + rs),
//     C = k - rs (lc + ls),   S = k + rc (ls - lc).
// Both sums hold table values only.  rc + rs is uniform over a row and is stored in the row table (RowBase::cs); lc + ls and
// ls - lc are a lane's constants and are stored in the lane table (LaneEntry::sum, dif), each rounded once from the final
// entries.  Per sample that is one multiplication and two fmas where the four-multiplication form had two and two:
// 8 f64 operations per sample (nf, place, r, k, C, S, c, s; 11 second-order: + h and the two inner fmas) + two f64->f32 converts.
//
// Error budget of a multiplier component before the f32 cast, against glibc's f64 cos/sin(place) (tests/util.py NCO_ABS_ERR
// = 2e-15); every value has magnitude <= 1 (k, cs, sum, dif <= sqrt 2), 1 ulp of f64 in [1, 2) is 2.2e-16, in [0.5, 1) 1.1e-16:
//   * table entries: the platform sincos of the rounded product, <= 2 ulp = 2.2e-16, plus the final rounding of the
//     lo-correction, 0.56e-16: <= 2.8e-16 per entry; the rotation weighs them by |lc| + |ls| and |rc| + |rs|, both <= sqrt 2
//     (the partial derivatives of C and S are those of the four-multiplication form): 2 sqrt 2 * 2.8e-16 = 7.9e-16;
//   * the rotation's own roundings: fl(rc + rs) <= 1.1e-16, weighted by |lc|; fl(lc + ls) or fl(ls - lc) <= 1.1e-16, weighted by
//     |rs| or |rc|; the product k <= 1.1e-16; the fma's result (|C|, |S| <= 1) <= 0.56e-16:
//     1.1e-16 + 0.56e-16 + 1.1e-16 (|lc| + |rs|) <= 3.9e-16 (the four-multiplication form: 1.1e-16);
//   * residual correction: at most two roundings, 1.1e-16; the dropped r^2/2 <= 1.1e-16 first order, r^3/6 < 1e-17 second order;
//   * glibc's own cos/sin, < 1 ulp: 1.1e-16.
// Sum 1.51e-15 (7.9 + 3.9 + 1.1 + 1.1 + 1.1), a margin of 1.3x below the rule's 2e-15.  So the f32 rounding equals glibc's except
// when the f64 value lies within ~1e-8 f32-ulp of a rounding boundary.
#pragma once

#if defined(__HIPCC_RTC__) || defined(__HIPCC__)
#define QD_NCO_FN __device__ __forceinline__
#else
#include <math.h>
#define QD_NCO_FN inline
#endif

namespace qd {

// Row-base entry: everything that is uniform over one row of ROW consecutive samples.
struct __attribute__((aligned(32))) RowBase {
    double c, s;     // cos/sin of the exact product (row*ROW) * ratio
    double nf;       // (double)(row*ROW)
    double cs;       // fl(c + s)
};

// Lane-table entry of sample slot j inside a row: (lc, ls) = cos/sin of the exact product j * ratio, stored as the three values
// the rotation reads
struct LaneEntry {
    double c;        // lc
    double sum;      // fl(lc + ls)
    double dif;      // fl(ls - lc)
};

// Per-lane constants for one sample slot: the slot index and its lane-table entry.
struct LaneRot { double jf, c, sum, dif; };

// table entry: cos/sin of the exact product k * ratio, from the platform sincos of the rounded product
QD_NCO_FN void nco_table_entry(double kf, double ratio, double *c, double *s) {
    const double th = kf * ratio;
    const double lo = __builtin_fma(kf, ratio, -th);     // exact: k*ratio = th + lo
    double s0, c0;
    sincos(th, &s0, &c0);
    // cos / sin(th + lo), |lo| <= ulp(th)/2 (up to ~4e-6 at the far end of a 2^34-sample stream): third order in lo, the
    // small terms gathered first so that each entry takes one final rounding
    const double q = 0.5 * lo * lo, sl = __builtin_fma(-lo * lo * lo, 1.0 / 6.0, lo);     // 1 - cos lo, sin lo
    *c = c0 + __builtin_fma(-q, c0, -sl * s0);
    *s = s0 + __builtin_fma(-q, s0, sl * c0);
}

// the row table's entry of the row that starts at sample nf
QD_NCO_FN RowBase nco_row_entry(double nf, double ratio) {
    RowBase rb;
    rb.nf = nf;
    nco_table_entry(nf, ratio, &rb.c, &rb.s);
    rb.cs = rb.c + rb.s;
    return rb;
}

// the lane table's entry of slot j
QD_NCO_FN LaneEntry nco_lane_entry(double jf, double ratio) {
    double c, s;
    nco_table_entry(jf, ratio, &c, &s);
    LaneEntry e;
    e.c = c; e.sum = c + s; e.dif = s - c;
    return e;
}

QD_NCO_FN LaneRot nco_lane_rot(double jf, const LaneEntry &e) {
    LaneRot lr;
    lr.jf = jf; lr.c = e.c; lr.sum = e.sum; lr.dif = e.dif;
    return lr;
}

// the rotation: (C, S) = cos / sin of the exact product (rb.nf + lr.jf) * ratio, from the two table entries
QD_NCO_FN void nco_rotate(const RowBase &rb, const LaneRot &lr, double *C, double *S) {
    const double k = lr.c * rb.cs;
    *C = __builtin_fma(-rb.s, lr.sum, k);
    *S = __builtin_fma(rb.c, lr.dif, k);
}

// the reference's multiplier of sample rb.nf + lr.jf before the f32 casts
template <bool SECOND_ORDER>
QD_NCO_FN void nco_mul_f64(const RowBase &rb, const LaneRot &lr, double ratio, double *c, double *s) {
    const double nf = rb.nf + lr.jf;                     // exact (integers < 2^53)
    const double place = nf * ratio;                     // == reference `place`
    const double r = __builtin_fma(nf, ratio, -place);   // exact: n*ratio = place + r
    double C, S;
    nco_rotate(rb, lr, &C, &S);
    if constexpr (SECOND_ORDER) {
        const double h = 0.5 * r;
        *c = __builtin_fma(r, __builtin_fma(-h, C, S), C);         // C (1 - r^2/2) + r S
        *s = __builtin_fma(-r, __builtin_fma(h, S, C), S);         // S (1 - r^2/2) - r C
    } else {
        *c = __builtin_fma(r, S, C);
        *s = __builtin_fma(-r, C, S);
    }
}

// ... as f32 (re, im)
template <bool SECOND_ORDER>
QD_NCO_FN void nco_mul(const RowBase &rb, const LaneRot &lr, double ratio, float *re, float *im) {
    double c, s;
    nco_mul_f64<SECOND_ORDER>(rb, lr, ratio, &c, &s);
    *re = (float)c; *im = (float)s;
}

// The same arithmetic for the N samples a lane owns, written step-by-step across the samples so
// that the N independent f64 dependency chains are issued interleaved.  F2: any pair of floats named x, y.
template <bool SECOND_ORDER, int N, class F2>
QD_NCO_FN void nco_mul_n(const RowBase &rb, const LaneRot *lr, double ratio, F2 *m) {
    double nf[N], pl[N], r[N], k[N], C[N], S[N], c[N], s[N];
#pragma unroll
    for (int u = 0; u < N; ++u) nf[u] = rb.nf + lr[u].jf;
#pragma unroll
    for (int u = 0; u < N; ++u) { pl[u] = nf[u] * ratio; k[u] = lr[u].c * rb.cs; }
#pragma unroll
    for (int u = 0; u < N; ++u) { r[u] = __builtin_fma(nf[u], ratio, -pl[u]); C[u] = __builtin_fma(-rb.s, lr[u].sum, k[u]); S[u] = __builtin_fma(rb.c, lr[u].dif, k[u]); }
    if constexpr (SECOND_ORDER) {
        double h[N], uu[N], vv[N];
#pragma unroll
        for (int u = 0; u < N; ++u) h[u] = 0.5 * r[u];
#pragma unroll
        for (int u = 0; u < N; ++u) { uu[u] = __builtin_fma(-h[u], C[u], S[u]); vv[u] = __builtin_fma(h[u], S[u], C[u]); }
#pragma unroll
        for (int u = 0; u < N; ++u) { c[u] = __builtin_fma(r[u], uu[u], C[u]); s[u] = __builtin_fma(-r[u], vv[u], S[u]); }
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) { c[u] = __builtin_fma(r[u], S[u], C[u]); s[u] = __builtin_fma(-r[u], C[u], S[u]); }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) { m[u].x = (float)c[u]; m[u].y = (float)s[u]; }
}

}  // namespace qd
