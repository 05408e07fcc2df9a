// Stand-alone host check of qd_spread.h: spread_add + spread_finish_cell over planted cells and random ones
// against a big-integer referee written here (no floating-point decision).  Built without HIP; meant to run under
// -fsanitize=address,undefined (scripts/sanitize_cpu.sh, leg 4).  usage: spread_host_check [random cells, default 4000]
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../quadrs_amd/csrc/qd_spread.h"

namespace {
struct Big {
    std::vector<uint32_t> w;
    Big(uint64_t v = 0) { while (v) { w.push_back((uint32_t)v); v >>= 32; } }
    void trim() { while (!w.empty() && !w.back()) w.pop_back(); }
};
Big add(const Big &a, const Big &b) {
    Big r; uint64_t c = 0;
    for (size_t i = 0; i < std::max(a.w.size(), b.w.size()) || c; ++i) {
        c += (i < a.w.size() ? a.w[i] : 0ull) + (i < b.w.size() ? b.w[i] : 0ull);
        r.w.push_back((uint32_t)c); c >>= 32;
    }
    r.trim(); return r;
}
int cmp(const Big &a, const Big &b) {
    if (a.w.size() != b.w.size()) return a.w.size() > b.w.size() ? 1 : -1;
    for (size_t i = a.w.size(); i-- > 0;) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i] ? 1 : -1;
    return 0;
}
Big sub(const Big &a, const Big &b) {                                    // a >= b
    Big r; int64_t c = 0;
    for (size_t i = 0; i < a.w.size(); ++i) {
        int64_t t = (int64_t)a.w[i] - (i < b.w.size() ? b.w[i] : 0) + c;
        c = t < 0 ? -1 : 0;
        r.w.push_back((uint32_t)(t & 0xffffffffll));
    }
    if (c) { fprintf(stderr, "sub: negative\n"); exit(2); }
    r.trim(); return r;
}
Big mul(const Big &a, const Big &b) {
    Big r; r.w.assign(a.w.size() + b.w.size() + 1, 0);
    for (size_t i = 0; i < a.w.size(); ++i) {
        uint64_t c = 0;
        for (size_t j = 0; j < b.w.size() || c; ++j) {
            c += r.w[i + j] + (uint64_t)a.w[i] * (j < b.w.size() ? b.w[j] : 0u);
            r.w[i + j] = (uint32_t)c; c >>= 32;
        }
    }
    r.trim(); return r;
}
Big shl(const Big &a, unsigned n) {
    if (a.w.empty()) return a;
    Big r; r.w.assign(n / 32, 0);
    const unsigned t = n % 32; uint64_t c = 0;
    for (uint32_t x : a.w) { c |= (uint64_t)x << t; r.w.push_back((uint32_t)c); c >>= 32; }
    if (c) r.w.push_back((uint32_t)c);
    r.trim(); return r;
}
// the f32 pattern p (finite, sign dropped) in units of 2^-149
Big units(uint32_t p) {
    const uint32_t e = p >> 23, m = (p & 0x7fffffu) | (e ? 1u << 23 : 0u);
    return shl(Big(m), (e ? e : 1u) - 1u);
}

struct Ref { uint32_t std_bits, count; bool nan, zero; Big D; uint32_t n; };
Ref referee(const std::vector<uint32_t> &vals) {
    Ref r{}; Big A, B; uint64_t n = 0, inf = 0;
    for (uint32_t b : vals) {
        b &= 0x7fffffffu;
        if (b > 0x7f800000u) continue;
        if (b == 0x7f800000u) { ++inf; continue; }
        const Big u = units(b);
        A = add(A, u); B = add(B, mul(u, u)); ++n;
    }
    r.count = (uint32_t)(n + inf); r.n = (uint32_t)n;
    if (r.count == 0 || inf) { r.nan = true; return r; }
    r.D = sub(mul(Big(n), B), mul(A, A));
    const Big n2 = Big(n * n);
    uint32_t lo = 0, hi = 0x7f7fffffu;                                   // the largest pattern with val^2 n^2 <= D
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        const Big u = units(mid);
        if (cmp(mul(mul(u, u), n2), r.D) <= 0) lo = mid; else hi = mid - 1;
    }
    const Big s = add(units(lo), units(lo + 1));
    const int half = cmp(shl(r.D, 2), mul(mul(s, s), n2));
    r.std_bits = lo + ((half > 0 || (half == 0 && (lo & 1))) ? 1u : 0u);
    r.zero = r.D.w.empty();
    return r;
}
// is the f64 x the rational D / n (units of 2^-298) rounded to nearest, ties to even?
bool ssd_right(double x, const Ref &r) {
    if (r.zero) return x == 0.0;
    uint64_t xb; memcpy(&xb, &x, 8);
    const int E = (int)(xb >> 52);
    if (E == 0 || E == 2047 || (xb >> 63)) return false;
    const uint64_t m = (xb & 0xfffffffffffffull) | (1ull << 52);
    const int e = E - 1075 + 298 + 500;                                  // x 2^798 = m 2^e with e > 0
    if (e < 1) return false;
    const Big lhs = shl(r.D, 501);                                       // 2 D 2^500
    const Big nn = Big(r.n);
    const Big dn = mul(shl(Big(2 * m - 1), e), nn), up = mul(shl(Big(2 * m + 1), e), nn);
    const int a = cmp(lhs, dn), b = cmp(lhs, up);
    // the lower neighbour of a power of two is half as far: m == 2^52 then needs 4 D against (4 m - 1)
    if (m == (1ull << 52)) { const Big d2 = mul(shl(Big(4 * m - 1), e), nn); const int a2 = cmp(shl(r.D, 502), d2); return a2 >= 0 && (b < 0 || (b == 0 && !(m & 1))); }
    return (a > 0 || (a == 0 && !(m & 1))) && (b < 0 || (b == 0 && !(m & 1)));
}

int failures = 0;
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

void check(const std::vector<uint32_t> &vals, const char *what, long want_std = -1) {
    uint64_t acc[qd::kSpreadWords] = {0}, ma[qd::kMeanWords] = {0}, pa[qd::kPowerWords] = {0};
    for (uint32_t b : vals) { qd::spread_add(acc, b); qd::mean_add(ma, b); qd::power_add(pa, b); }
    qd::SpreadRounded c;
    qd::spread_finish_cell(acc, qd::kSpreadAll, &c);
    uint32_t mb, rb, cnt; double s;
    qd::mean_finish_cell(ma, &mb, &s, &cnt);
    qd::power_finish_cell(pa, &rb, &s, &cnt);
    const Ref r = referee(vals);
    uint64_t sb; memcpy(&sb, &c.ssd, 8);
    bool ok = c.count == r.count && c.mean_bits == mb && c.rms_bits == rb;
    if (r.count == 0) ok = ok && c.std_bits == 0x7fc00000u && sb == 0;
    else if (r.nan) ok = ok && c.std_bits == 0x7fc00000u && sb == 0x7ff8000000000000ull;
    else ok = ok && c.std_bits == r.std_bits && ssd_right(c.ssd, r);
    if (want_std >= 0 && c.std_bits != (uint32_t)want_std) ok = false;
    // each half alone gives the same bits
    qd::SpreadRounded d;
    qd::spread_finish_cell(acc, qd::kSpreadSsd, &d);
    uint64_t db; memcpy(&db, &d.ssd, 8);
    ok = ok && db == sb;
    qd::spread_finish_cell(acc, qd::kSpreadStd, &d);
    ok = ok && d.std_bits == c.std_bits;
    if (!ok) {
        ++failures;
        fprintf(stderr, "MISMATCH %s: n=%zu std %08x (referee %08x, planted %lx) ssd %a count %u (%u) mean %08x (%08x) rms %08x (%08x)\n", what, vals.size(),
                c.std_bits, r.std_bits, want_std, c.ssd, c.count, r.count, c.mean_bits, mb, c.rms_bits, rb);
    }
}
std::vector<uint32_t> rep(std::vector<uint32_t> v, size_t times) {
    std::vector<uint32_t> o;
    for (size_t i = 0; i < times; ++i) o.insert(o.end(), v.begin(), v.end());
    return o;
}
}  // namespace

int main(int argc, char **argv) {
    const int n_random = argc > 1 ? atoi(argv[1]) : 4000;
    const long tie[5][2] = {{1, 0}, {2, 1}, {3, 2}, {5, 2}, {7, 4}};
    for (auto &t : tie) check({0u, (uint32_t)t[0]}, "subnormal tie", t[1]);
    check(rep({0x4b7ffffeu, 0x4b7fffffu}, 2048), "2^24 pair", 0x3f000000);
    check(rep({0x3fb504f3u, 0x3fb504f4u}, 1500), "sqrt2 pair", 0x33800000);
    check(rep({0x7f7ffffeu, 0x7f7fffffu}, 2048), "max pair", 0x73000000);
    check({0x7f7fffffu, 0x7f7fffffu, 0x7f7fffffu, 0u}, "three max and a zero", 0x7eddb3d6);
    check({0x7f7fffffu, 0u}, "max and zero", 0x7effffff);
    for (uint32_t b : {0u, 1u, 0x00800000u, 0x3f800000u, 0x4b7fffffu, 0x7f7fffffu}) { check(rep({b}, 7), "all equal", 0); check({b}, "one value", 0); }
    check({0x80000000u, 0xbf800000u, 0x3f800000u, 0xc0000000u}, "negative patterns");
    check({0x7fc00000u, 0x3f800000u, 0xffc00001u, 0x40000000u}, "NaNs skipped");
    check({0x3f800000u, 0x7f800000u, 0x40000000u}, "a +inf");
    check({0x7fc00000u}, "only NaN");
    check({}, "empty");
    const int ns[4] = {2, 3, 17, 100};
    for (int i = 0; i < n_random; ++i) {
        const int n = ns[i & 3];
        const uint32_t e0 = rnd() % 255;                                 // a random binade, the values within three of it
        std::vector<uint32_t> v;
        for (int k = 0; k < n; ++k) {
            uint32_t e = e0 + rnd() % 4; if (e > 254) e = 254;
            uint32_t b = (e << 23) | (rnd() & 0x7fffffu);
            if (i % 7 == 3 && k) b = v[0] + (rnd() % 3);                 // near-equal cells: heavy cancellation
            if (b > 0x7f7fffffu) b = 0x7f7fffffu;
            v.push_back(b);
        }
        check(v, "random");
    }
    for (int i = 0; i < n_random / 8; ++i) {                             // the whole range in one cell
        std::vector<uint32_t> v;
        for (int k = 0; k < 5; ++k) v.push_back(rnd() % 0x7f800000u);
        check(v, "wide random");
    }
    printf("spread_host_check: %s (%d mismatches)\n", failures ? "FAILED" : "clean", failures);
    return failures ? 1 : 0;
}
