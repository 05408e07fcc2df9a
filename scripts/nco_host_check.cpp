// nco_host_check.cpp — the NCO's arithmetic (quadrs_amd/csrc/qd_nco.h: nco_row_entry, nco_lane_entry, nco_rotate, nco_mul_f64, nco_mul,
// nco_mul_n) in a stand-alone host program, held to __float128.
//   g++ -O2 -ffp-contract=off -std=c++17 -Wall -Wno-unknown-pragmas -o nco_host_check scripts/nco_host_check.cpp -lquadmath
//   ./nco_host_check <NCO_ABS_ERR of tests/util.py> [--mutate cs32]
// (the same program is the one to build with -fsanitize=address,undefined)
//
// Blocks of 2^16 consecutive samples at five depths — sample 0, the last block below and the first above the 2^28 rad switch of the NCO
// order, about 2^32 rad, the last block below sample 2^34 (depths past it fold onto it) — for four ratios: the headline chain's
// (280 kHz at 21 Msps), +-(rate/2 - 1)/rate 2 pi, and a small one (50 Hz at 21 Msps); rows of 512 and of 1024 samples.  Per sample:
//   * the multiplier before its f32 casts (nco_mul_f64, second order everywhere, first order where |place| <= 2^28 rad) against
//     sincosq of place = fl(n ratio), the value glibc's f64 cos / sin approximate;
//   * the rotation (nco_rotate) against the exact product of the four table values it stands for (106-bit products, exact in 113);
//   * nco_mul and nco_mul_n<.., 4> give the same f32 words.
// Bounds (derivation: qd_nco.h).  total = 2 sqrt 2 * 2.8e-16 + 3.9e-16 + 1.1e-16 + 1.1e-16 + 1.1e-16 = 1.51e-15 must lie below NCO_ABS_ERR.
// Here the host's sincos stands in for the device's, so the multiplier is asserted against total less the device-libm term
// (2 sqrt 2 * 2.2e-16 = 6.2e-16): 8.9e-16.  What the host's own sincos adds (glibc: below 1 ulp, in practice 0.55) comes out of glibc's
// own 1.1e-16 in the total, which a comparison against __float128 does not spend.  The rotation's roundings: 3.9e-16.
// --mutate cs32: the row entry's cs taken as an f32-rounded sum (a dropped rounding guard); the rotation assertion must then fail.
#include "../quadrs_amd/csrc/qd_nco.h"

#include <quadmath.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace qd;

struct F2 { float x, y; };

static const double kSqrt2 = 1.4142135623730951;
static const double kEntry = 2.8e-16, kRotation = 3.9e-16, kResidual = 1.1e-16, kDropped = 1.1e-16, kGlibc = 1.1e-16, kDevSincos = 2.2e-16;
static const double kTotal = 2 * kSqrt2 * kEntry + kRotation + kResidual + kDropped + kGlibc;
static const double kHostBound = kTotal - 2 * kSqrt2 * kDevSincos;
static const uint64_t kBlock = 1ull << 16, kStreamEnd = 1ull << 34;
static const double kOrderSwitch = 268435456.0;      // 2^28 rad (quadrs_hip.hip: the plan's NCO order)

static bool g_mutate_cs32 = false;

static RowBase row_entry(uint64_t n_row, double ratio) {
    RowBase rb = nco_row_entry((double)n_row, ratio);
    if (g_mutate_cs32) rb.cs = (double)(float)(rb.c + rb.s);
    return rb;
}

struct Worst { double mul1 = 0, mul2 = 0, rot = 0; };

static int check_block(double ratio, uint64_t n0, Worst *w) {
    std::vector<__float128> tc(kBlock), ts(kBlock);
    bool first_ok = true;
    for (uint64_t i = 0; i < kBlock; ++i) {
        const double place = (double)(n0 + i) * ratio;
        if (fabs(place) > kOrderSwitch) first_ok = false;
        sincosq((__float128)place, &ts[i], &tc[i]);
    }
    for (uint32_t ROW : {512u, 1024u}) {
        std::vector<LaneEntry> lane(ROW);
        std::vector<double> lc(ROW), ls(ROW);
        for (uint32_t j = 0; j < ROW; ++j) { lane[j] = nco_lane_entry((double)j, ratio); nco_table_entry((double)j, ratio, &lc[j], &ls[j]); }
        uint64_t cur_row = ~0ull;
        RowBase rb{};
        for (uint64_t i = 0; i < kBlock; ++i) {
            const uint64_t n = n0 + i, row = n / ROW;
            const uint32_t j = (uint32_t)(n % ROW);
            if (row != cur_row) { rb = row_entry(row * ROW, ratio); cur_row = row; }
            const LaneRot lr = nco_lane_rot((double)j, lane[j]);
            double C, S;
            nco_rotate(rb, lr, &C, &S);
            const __float128 Cx = (__float128)rb.c * lc[j] - (__float128)rb.s * ls[j], Sx = (__float128)rb.s * lc[j] + (__float128)rb.c * ls[j];
            w->rot = std::max(w->rot, std::max((double)fabsq(C - Cx), (double)fabsq(S - Sx)));
            double c2, s2;
            nco_mul_f64<true>(rb, lr, ratio, &c2, &s2);
            w->mul2 = std::max(w->mul2, std::max((double)fabsq(c2 - tc[i]), (double)fabsq(s2 - ts[i])));
            float re, im;
            nco_mul<true>(rb, lr, ratio, &re, &im);
            if (re != (float)c2 || im != (float)s2) { printf("nco_host_check: FAILED nco_mul<true> casts (n %llu)\n", (unsigned long long)n); return 1; }
            if (first_ok) {
                double c1, s1;
                nco_mul_f64<false>(rb, lr, ratio, &c1, &s1);
                w->mul1 = std::max(w->mul1, std::max((double)fabsq(c1 - tc[i]), (double)fabsq(s1 - ts[i])));
            }
            if (j % 4 == 0 && j + 4 <= ROW && i + 4 <= kBlock) {         // a lane's four slots through the interleaved form
                LaneRot l4[4];
                F2 m2[4], m1[4];
                for (int u = 0; u < 4; ++u) l4[u] = nco_lane_rot((double)(j + u), lane[j + u]);
                nco_mul_n<true, 4>(rb, l4, ratio, m2);
                nco_mul_n<false, 4>(rb, l4, ratio, m1);
                for (int u = 0; u < 4; ++u) {
                    float a, b, c, d;
                    nco_mul<true>(rb, l4[u], ratio, &a, &b);
                    nco_mul<false>(rb, l4[u], ratio, &c, &d);
                    if (memcmp(&a, &m2[u].x, 4) || memcmp(&b, &m2[u].y, 4) || memcmp(&c, &m1[u].x, 4) || memcmp(&d, &m1[u].y, 4)) {
                        printf("nco_host_check: FAILED nco_mul_n differs from nco_mul (n %llu)\n", (unsigned long long)(n + u));
                        return 1;
                    }
                }
            }
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: nco_host_check <NCO_ABS_ERR> [--mutate cs32]\n"); return 2; }
    const double rule = atof(argv[1]);
    if (argc >= 4 && !strcmp(argv[2], "--mutate") && !strcmp(argv[3], "cs32")) g_mutate_cs32 = true;
    printf("derived total %.3e (rule %.3e), host bound %.3e, rotation bound %.3e\n", kTotal, rule, kHostBound, kRotation);
    if (!(kTotal < rule)) { printf("nco_host_check: FAILED derived total not below the rule\n"); return 1; }
    const double tau = 6.283185307179586, rate = 21000000.0;
    const double ratios[4] = {tau * 280000.0 / rate, tau * (rate / 2 - 1) / rate, -tau * (rate / 2 - 1) / rate, tau * 50.0 / rate};
    int rc = 0;
    Worst all;
    for (double ratio : ratios) {
        const double a = fabs(ratio);
        const uint64_t last = kStreamEnd - kBlock;
        const double n_sw = floor(kOrderSwitch / a), n_32 = floor(4294967296.0 / a);
        std::vector<uint64_t> depths = {0};
        // first sample whose |place| can exceed 2^28 rad is n_sw + 1: the block below ends at n_sw inclusive
        if (n_sw >= (double)kBlock) depths.push_back(std::min<uint64_t>((uint64_t)n_sw + 1 - kBlock, last));
        depths.push_back(n_sw + 1 < (double)last ? (uint64_t)n_sw + 1 : last);
        depths.push_back(n_32 < (double)last ? (uint64_t)n_32 : last);
        depths.push_back(last);
        std::sort(depths.begin(), depths.end());
        depths.erase(std::unique(depths.begin(), depths.end()), depths.end());
        for (uint64_t n0 : depths) {
            Worst w;
            rc |= check_block(ratio, n0, &w);
            printf("ratio %+.17g n0 %11llu: first order %.3e  second order %.3e  rotation %.3e\n", ratio, (unsigned long long)n0, w.mul1, w.mul2, w.rot);
            all.mul1 = std::max(all.mul1, w.mul1); all.mul2 = std::max(all.mul2, w.mul2); all.rot = std::max(all.rot, w.rot);
        }
    }
    printf("worst: first order %.3e  second order %.3e  rotation %.3e\n", all.mul1, all.mul2, all.rot);
    if (rc) return 1;
    if (!(all.rot <= kRotation)) { printf("nco_host_check: FAILED rotation rounding %.3e > %.3e\n", all.rot, kRotation); return 1; }
    if (!(all.mul1 <= kHostBound && all.mul2 <= kHostBound)) { printf("nco_host_check: FAILED multiplier %.3e / %.3e > %.3e\n", all.mul1, all.mul2, kHostBound); return 1; }
    printf("nco_host_check: ok\n");
    return 0;
}
