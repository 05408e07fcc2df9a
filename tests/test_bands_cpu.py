"""The band traces' host half (include/quadrs_hip.h, "band traces"): qd_bands_fold against a referee written here with Python integers and
fractions — the exact sum of a band in units of 2^-149, Fraction -> f64 for the sum, and an f32 rounding of sum / count done on the
fraction itself (nearest, ties to even) —, against the existing folds on transposed data, the peak bin's and the pick's tie rules, the
error codes, and the launch geometry of k_bands (quadrs_amd/csrc/qd_bands.h) walked by a stand-alone host program.  No GPU."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_mean_cpu import PLANTED_CASES
from test_power_cpu import PLANTED_TIES

F32 = np.float32
NAN_BITS, INF_BITS, NONE = 0x7FC00000, 0x7F800000, 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrs_amd", "csrc")


def units(bits):
    """a finite non-negative f32's value as an integer count of 2^-149"""
    e, m = bits >> 23, bits & 0x7FFFFF
    return (m | (1 << 23) if e else m) << (max(e, 1) - 1)


def rne_f32(x):
    """the bit pattern of the non-negative Fraction x (below 2^128) rounded to f32, nearest, ties to even: x in units of the quantum of its
    binade (2^-149 below 2^-126), the integer part kept, the remainder compared with one half exactly"""
    if x == 0:
        return 0
    e = max(x.numerator.bit_length() - x.denominator.bit_length(), -127)
    while e > -126 and Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    e = max(e, -126)
    q = x / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    # n quanta: n < 2^23 is a subnormal's pattern; else the pattern carries by itself (n == 2^24 is the next binade's 1.0)
    return n if e == -126 and n < (1 << 23) else ((e + 127 - 1) << 23) + n


def ref_bands(bits, bands):
    """(level bits u32, sum f64, count u32, peak bits u32, peak_bin u32)[n, K] and pick u8[n] of u32 bit patterns [n, W], by the definition"""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    n, K = bits.shape[0], len(bands)
    level, total, count = np.empty((n, K), np.uint32), np.empty((n, K), np.float64), np.empty((n, K), np.uint32)
    peak, peak_bin, pick = np.empty((n, K), np.uint32), np.empty((n, K), np.uint32), np.empty(n, np.uint8)
    for i in range(n):
        for k, (lo, hi) in enumerate(bands):
            vals = [(int(b) & 0x7FFFFFFF, lo + j) for j, b in enumerate(bits[i, lo:hi])]
            vals = [(b, at) for b, at in vals if b <= INF_BITS]
            count[i, k] = len(vals)
            if not vals:
                level[i, k], total[i, k], peak[i, k], peak_bin[i, k] = NAN_BITS, 0.0, 0, NONE
                continue
            top = max(b for b, _ in vals)
            peak[i, k], peak_bin[i, k] = top, min(at for b, at in vals if b == top)
            if top == INF_BITS:
                level[i, k], total[i, k] = INF_BITS, math.inf
                continue
            S = sum(units(b) for b, _ in vals)
            total[i, k] = float(Fraction(S, 1 << 149))                     # int / int: correctly rounded
            level[i, k] = rne_f32(Fraction(S, len(vals) << 149))
        best = 255
        for k in range(K):
            if count[i, k] and (best == 255 or level[i, k] > level[i, best]):
                best = k
        pick[i] = best
    return level, total, count, peak, peak_bin, pick


def same6(got, ref):
    """all six outputs byte for byte (ref's level and peak are bit patterns)"""
    assert len(got) == len(ref) == 6
    for name, g, r in zip(("level", "sum", "count", "peak", "peak_bin", "pick"), got, ref):
        assert g.shape == r.shape and g.tobytes() == r.tobytes(), name
    return True


def band_sets(W):
    sets = [[(0, W)], [(b, b + 1) for b in range(min(W, 255))]]
    if W >= 2:
        sets.append([(0, W // 2), (W // 2, W)])
    if W >= 4:
        sets += [[(1, W - 1)], [(0, W // 2 + 1), (W // 4, W), (1, 2), (W // 4, W), (W - 1, W), (2, W - 1)]]
    return sets


def patterns(n, W, seed):
    """arbitrary f32 bit patterns: both signs, NaN payloads, +-inf, zeros, subnormals, every exponent"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, size=(n, W), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0, 0x80000000, 1, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF],
                       dtype=np.uint32)
    idx = rng.integers(0, n * W, size=n * W // 4)
    bits.reshape(-1)[idx] = special[rng.integers(0, special.size, size=idx.size)]
    # near values, so that sums carry and means round: one binade
    bits[n // 2:] = (bits[n // 2:] & np.uint32(0x807FFFFF)) | np.uint32(0x3F800000)
    bits[n // 2, : W // 2] = NAN_BITS
    bits[n - 1] = 0xFFC00000                                             # a window without a value
    return bits


@pytest.mark.parametrize("W", [1, 2, 4, 64, 256])
def test_fold_matches_the_integer_referee(engine, W):
    bits = patterns(12, W, 77 + W)
    for bands in band_sets(W):
        got = engine.bands_fold(bits.view(F32), bands)
        assert got[0].dtype == F32 and got[1].dtype == np.float64 and got[2].dtype == np.uint32 and got[4].dtype == np.uint32 and got[5].dtype == np.uint8
        assert same6(got, ref_bands(bits, bands))
    if W >= 64:
        # teeth: a sequential f32 sum over the band divided by the count is not the level somewhere in this very input
        got = engine.bands_fold(bits.view(F32), [(0, W)])[0]
        a = np.abs(bits.view(F32))
        naive = np.zeros(bits.shape[0], F32)
        with np.errstate(all="ignore"):
            for i, row in enumerate(a):
                acc = F32(0)
                for v in row[~np.isnan(row)]:
                    acc = F32(acc + v)
                naive[i] = acc / F32(max((~np.isnan(row)).sum(), 1))
        finite = np.isfinite(got[:, 0]) & np.isfinite(naive)
        assert finite.any() and (naive.view(np.uint32)[finite] != got[:, 0].view(np.uint32)[finite]).any()


def test_one_band_spans_all_nine_limbs(engine):
    # every biased exponent 0 ... 254 in one band: an addend in every limb; and the two ends of the range alone
    e = np.arange(255, dtype=np.uint32)
    bits = np.stack([(e << 23) | 1, (e << 23) | 0x7FFFFF, np.where(e % 2 == 0, (e << 23) | 0x400000, 0xFFC00000).astype(np.uint32)])
    bands = [(0, 255), (0, 32), (31, 33), (200, 255), (0, 1), (254, 255), (0, 2)]
    assert same6(engine.bands_fold(bits.view(F32), bands), ref_bands(bits, bands))


def test_planted_rounding_cases_along_the_bin_axis(engine):
    cases = [c[0] for c in PLANTED_CASES] + PLANTED_TIES
    W = 8
    bits = np.full((len(cases), W), NAN_BITS, dtype=np.uint32)
    for i, vals in enumerate(cases):
        bits[i, 2:2 + len(vals)] = vals                                    # lo = 2: not a multiple of 4
    bands = [(2, W), (0, W)]
    got = engine.bands_fold(bits.view(F32), bands)
    assert same6(got, ref_bands(bits, bands))
    for i, (vals, want_mean, want_sum, want_count) in enumerate(PLANTED_CASES):
        assert got[2][i, 0] == want_count
        assert want_mean is None or got[0].view(np.uint32)[i, 0] == want_mean, (i, hex(got[0].view(np.uint32)[i, 0]))
        assert want_sum is None or got[1][i, 0] == want_sum, (i, got[1][i, 0])


@pytest.mark.parametrize("W", [4, 64])
def test_bit_for_bit_the_existing_folds_on_transposed_data(engine, W):
    bits = patterns(9, W, 5 + W)
    bands = band_sets(W)[-1] + [(0, W), (2, 3)]
    level, total, count, peak, _, _ = engine.bands_fold(bits.view(F32), bands)
    for i in range(bits.shape[0]):
        for k, (lo, hi) in enumerate(bands):
            column = bits[i, lo:hi].view(F32).reshape(-1, 1)
            m, s, c = engine.mean_finish(engine.mean_fold(column, hi - lo))
            assert (m.tobytes(), s.tobytes(), c.tobytes()) == (level[i, k].tobytes(), total[i, k].tobytes(), count[i, k].tobytes()), (i, k)
            # qd_pool_fold compares values; the band's peak drops the sign bit as k_pool does: the same for norms, which have none
            pk, _ = engine.pool_fold(np.abs(column), hi - lo)
            assert pk.tobytes() == peak[i, k].tobytes(), (i, k)


def test_peak_bin_rules(engine):
    nan, inf = np.uint32(NAN_BITS).view(F32), F32(np.inf)
    a = np.array([[1, 5, 2, 5, 5, 0, 0, 1],                        # ties go to the lowest bin
                  [0, 0, 0, -0.0, 0, 0, 0, 0],                     # all zero: lo
                  [nan] * 8,                                       # no value
                  [3, nan, inf, 9, inf, nan, 1, 2],                # +inf wins, the lower one
                  [nan, nan, nan, 2, nan, 2, nan, nan]], dtype=F32)
    bands = [(0, 8), (2, 8), (4, 6), (5, 7), (7, 8)]
    level, total, count, peak, peak_bin, pick = engine.bands_fold(a, bands)
    assert peak_bin.tolist() == [[1, 3, 4, 5, 7], [0, 2, 4, 5, 7], [NONE] * 5, [2, 2, 4, 6, 7], [3, 3, 5, 5, NONE]]
    assert peak.tolist()[0] == [5, 5, 5, 0, 1] and peak.tolist()[3] == [np.inf, np.inf, np.inf, 1, 2] and not peak[2].any()
    assert not np.signbit(peak).any()
    assert count[2].tolist() == [0] * 5 and (level[2].view(np.uint32) == NAN_BITS).all() and not total[2].any()
    assert same6((level, total, count, peak, peak_bin, pick), ref_bands(a.view(np.uint32), bands))


def test_pick_rules(engine):
    nan = np.uint32(NAN_BITS).view(F32)
    a = np.array([[2, 2, 2, 2, 1, 3, 4, 0],                        # bands 0 and 1 tie at 2.0: the lowest k
                  [nan, nan, 1, 1, nan, nan, 0, 0],                # empty bands are never picked, whatever their NaN's bits
                  [nan] * 8,                                       # all empty: 255
                  [0, 0, 0, 0, 0, 0, 0, 0],                        # a level of 0.0 is a level
                  [nan, nan, nan, nan, nan, nan, np.inf, 5]], dtype=F32)
    bands = [(0, 2), (2, 4), (4, 6), (6, 8)]
    out = engine.bands_fold(a, bands)
    assert out[5].tolist() == [0, 1, 255, 0, 3]
    # recomputable from the level and count rows alone
    level, count = out[0].view(np.uint32), out[2]
    for i in range(a.shape[0]):
        live = [k for k in range(len(bands)) if count[i, k]]
        want = min(live, key=lambda k: (-int(level[i, k]), k)) if live else 255
        assert out[5][i] == want
    # ... and alone: the pick needs none of the other rows
    only = engine.bands_fold(a, bands, outputs=("pick",))
    assert only[5].tobytes() == out[5].tobytes() and all(o is None for o in only[:5])
    bits = patterns(12, 64, 3)
    b = [(0, 16), (16, 32), (8, 40), (63, 64), (16, 32)]
    assert engine.bands_fold(bits.view(F32), b, outputs=("pick",))[5].tobytes() == ref_bands(bits, b)[5].tobytes()


def test_identical_overlapping_and_one_bin_bands(engine):
    bits = patterns(10, 64, 11)
    a = bits.view(F32)
    got = engine.bands_fold(a, [(3, 20), (3, 20), (3, 12), (12, 20)])
    for o in got[:5]:
        assert o[:, 0].tobytes() == o[:, 1].tobytes()
    level, total, count, peak, peak_bin, _ = got
    assert (count[:, 2] + count[:, 3] == count[:, 0]).all()
    assert (np.maximum(peak[:, 2], peak[:, 3]) == peak[:, 0]).all()
    lower = (count[:, 2] > 0) & ((peak[:, 2] >= peak[:, 3]) | (count[:, 3] == 0))      # the lower half holds the peak, or ties
    assert (np.where(lower, peak_bin[:, 2], peak_bin[:, 3]) == peak_bin[:, 0]).all()
    # a one-bin band returns the norm itself
    level, total, count, peak, peak_bin, _ = engine.bands_fold(a, [(b, b + 1) for b in range(64)])
    keep = (bits & 0x7FFFFFFF) <= INF_BITS
    mag = np.abs(a)
    assert level[keep].tobytes() == mag[keep].tobytes() and total[keep].tobytes() == mag[keep].astype(np.float64).tobytes()
    assert peak[keep].tobytes() == mag[keep].tobytes() and (count == keep).all()
    assert (peak_bin[keep] == np.broadcast_to(np.arange(64, dtype=np.uint32), bits.shape)[keep]).all() and (peak_bin[~keep] == NONE).all()
    assert (level.view(np.uint32)[~keep] == NAN_BITS).all() and not total[~keep].any() and not peak[~keep].any()


def test_refusals(engine):
    from quadrs_amd import _ffi
    L, INVALID = _ffi.lib(), _ffi.ERR_INVALID
    a = np.ones((2, 8), F32)
    norms = a.ctypes.data_as(C.c_void_p)
    out = np.full(2 * 255, F32(-7.5))
    rows = _ffi.BandRows(out.ctypes.data_as(C.c_void_p).value, None, None, None, None, None)

    def table(*pairs):
        return (_ffi.Band * len(pairs))(*[_ffi.Band(lo, hi) for lo, hi in pairs])
    ok = table((0, 8))
    assert L.qd_bands_fold(norms, 8, 2, ok, 0, C.byref(rows)) == INVALID                                 # no bands
    assert L.qd_bands_fold(norms, 8, 2, table(*[(0, 1)] * 256), 256, C.byref(rows)) == INVALID           # too many
    assert L.qd_bands_fold(norms, 8, 2, None, 1, C.byref(rows)) == INVALID
    for bad in ((3, 3), (4, 3), (0, 9), (8, 9)):
        assert L.qd_bands_fold(norms, 8, 2, table((0, 8), bad), 2, C.byref(rows)) == INVALID, bad
    assert L.qd_bands_fold(norms, 0, 2, ok, 1, C.byref(rows)) == INVALID                                 # no width
    assert L.qd_bands_fold(norms, 8, 2, ok, 1, None) == INVALID
    assert L.qd_bands_fold(norms, 8, 2, ok, 1, C.byref(_ffi.BandRows())) == INVALID                      # every row NULL
    assert L.qd_bands_fold(None, 8, 2, ok, 1, C.byref(rows)) == INVALID
    assert (out == F32(-7.5)).all()
    assert L.qd_bands_fold(None, 8, 0, ok, 1, C.byref(rows)) == 0 and (out == F32(-7.5)).all()           # nothing to fold
    assert L.qd_bands_fold(norms, 8, 2, table(*[(0, 8)] * 255), 255, C.byref(rows)) == 0 and (out == F32(1)).all()
    with pytest.raises(ValueError):
        engine.bands_fold(a, [(0, 8)], outputs=("level", "median"))
    # qd_plan_bands without a plan is refused before anything else is looked at, as every plan call is
    out[:] = F32(-7.5)
    assert L.qd_plan_bands(None, None, _ffi.MEM_HOST, 0, 0, 0, 1, ok, 1, C.byref(rows), _ffi.MEM_HOST, None) == INVALID and (out == F32(-7.5)).all()
    assert _ffi.BANDS_MAX == 255 and _ffi.BAND_NONE == NONE


def test_band_rules_live_in_one_host_clean_header(tmp_path):
    tu = tmp_path / "only_bands.cpp"
    tu.write_text('#include "qd_bands.h"\nint main() { qd::BandsGeometry G; uint64_t grid; qd::bands_split(0, 1, 4, 1, 4, &G, &grid);\n'
                  '    return qd::bands_lane(G, 0, 0).active && qd::bands_key(0, 0) ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the host source takes the indices from the header: it carries no copy of the item arithmetic
    text = open(os.path.join(CSRC, "quadrs_hip.hip"), encoding="utf-8").read()
    for phrase in ("items_per_group", "/ G.K", "% G.K", "log2_L", "kBandsReach"):
        assert phrase not in text, phrase


WALKER = r"""
#include "qd_bands.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace qd;

static unsigned long long g_ctx[8];
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s\n  W %llu K %llu n %llu batch %llu longest %llu g0 %llu block %llu tid %llu\n", #c, \
    g_ctx[0], g_ctx[1], g_ctx[2], g_ctx[3], g_ctx[4], g_ctx[5], g_ctx[6], g_ctx[7]); std::exit(1); } } while (0)

static unsigned long long g_launches = 0, g_bins = 0;

// every (workgroup, lane) of every launch of a range of n windows cut into batches of bw: the bins each lane takes, counted per
// (window, band, bin), and the item each lane group stores
static void walk(uint32_t W, const std::vector<Band> &bands, uint64_t n, uint64_t bw, uint32_t want_L) {
    const uint32_t K = (uint32_t)bands.size();
    uint32_t longest = 0;
    std::vector<uint64_t> first(K + 1, 0);                    // band k's counters start at first[k] within a window
    for (uint32_t k = 0; k < K; ++k) {
        longest = bands[k].hi - bands[k].lo > longest ? bands[k].hi - bands[k].lo : longest;
        first[k + 1] = first[k] + (bands[k].hi - bands[k].lo);
    }
    g_ctx[0] = W; g_ctx[1] = K; g_ctx[2] = n; g_ctx[3] = bw; g_ctx[4] = longest;
    std::vector<uint8_t> seen(n * first[K], 0), stored(n * K, 0);
    for (uint64_t g0 = 0; g0 < n; g0 += bw) {
        const uint64_t nw = n - g0 < bw ? n - g0 : bw;
        g_ctx[5] = g0;
        BandsGeometry G;
        uint64_t grid = 0;
        bands_split(g0, nw, W, K, longest, &G, &grid);
        ++g_launches;
        CHECK(G.L == want_L && (G.L == 1 || G.L == 4 || G.L == 16 || G.L == 64 || G.L == 256));
        CHECK(G.L == 256 || (uint64_t)kBandsReach * G.L >= longest);
        CHECK(G.L == 1 || (uint64_t)kBandsReach * (G.L / 4) < longest);
        CHECK(G.items_per_group * G.L == kBandsThreads && (1u << G.log2_L) == G.L && G.n_items == nw * K);
        CHECK(grid > 0 && grid <= 0x7fffffffull && (grid - 1) * G.items_per_group < G.n_items && grid * G.items_per_group >= G.n_items);
        for (uint64_t block = 0; block < grid; ++block) {
            g_ctx[6] = block;
            BandsLane lead{};
            for (uint32_t tid = 0; tid < kBandsThreads; ++tid) {
                g_ctx[7] = tid;
                const BandsLane l = bands_lane(G, (uint32_t)block, tid);
                CHECK(l.lane == tid % G.L);
                if (l.lane == 0) lead = l;
                // the lanes of a group share the item
                CHECK(l.active == lead.active && l.win == lead.win && l.band == lead.band && l.out == lead.out);
                CHECK(l.active == (block * G.items_per_group + tid / G.L < G.n_items));
                if (!l.active) continue;                       // a masked lane reads and stores nothing
                CHECK(l.win < nw && l.band < K && l.out == (g0 + l.win) * K + l.band && l.out < n * K);
                const Band b = bands[l.band];
                uint32_t prev = 0, taken = 0;
                for (uint32_t bin = bands_first_bin(l, b.lo); bin < b.hi; bin += bands_step(G)) {
                    CHECK(bin >= b.lo && bin < W && bin - b.lo == l.lane + taken * G.L);      // consecutive lanes, consecutive words
                    CHECK(taken == 0 || bin > prev);
                    uint8_t &c = seen[(g0 + l.win) * first[K] + first[l.band] + (bin - b.lo)];
                    CHECK(c == 0);
                    c = 1; prev = bin; ++taken; ++g_bins;
                }
                if (l.lane == 0) { CHECK(stored[l.out] == 0); stored[l.out] = 1; }
            }
        }
    }
    g_ctx[5] = g_ctx[6] = g_ctx[7] = ~0ull;
    for (uint8_t c : seen) CHECK(c == 1);
    for (uint8_t c : stored) CHECK(c == 1);
}

static uint32_t lanes_for(uint32_t longest) { return longest <= 16 ? 1 : longest <= 64 ? 4 : longest <= 256 ? 16 : longest <= 1024 ? 64 : 256; }

int main() {
    CHECK(bands_lanes(1) == 1 && bands_lanes(16) == 1 && bands_lanes(17) == 4 && bands_lanes(64) == 4 && bands_lanes(65) == 16 && bands_lanes(256) == 16 && bands_lanes(257) == 64);
    CHECK(bands_pick_log2_lanes(1) == 0 && bands_pick_log2_lanes(2) == 1 && bands_pick_log2_lanes(3) == 2 && bands_pick_log2_lanes(33) == 6);
    CHECK(bands_pick_log2_lanes(64) == 6 && bands_pick_log2_lanes(65) == 6 && bands_pick_log2_lanes(255) == 6);
    CHECK(bands_lanes(1024) == 64 && bands_lanes(1025) == 256 && bands_lanes(1u << 20) == 256);
    {   // more than 2^32 items in a batch (W = 1, K = 255, 2^25 windows): the lane index by its 64-bit branch
        BandsGeometry G;
        uint64_t grid = 0;
        bands_split(7, 1ull << 25, 1, 255, 1, &G, &grid);
        CHECK((G.n_items >> 32) != 0 && G.L == 1 && grid <= 0x7fffffffull);
        const uint32_t blocks[] = {0u, 16777216u, 20000000u, (uint32_t)(grid - 1)}, tids[] = {0u, 1u, 255u};
        for (uint32_t block : blocks)
            for (uint32_t tid : tids) {
                const BandsLane l = bands_lane(G, block, tid);
                const uint64_t item = (uint64_t)block * 256 + tid;
                CHECK(l.active && l.lane == 0 && l.win == item / 255 && l.band == item % 255 && l.out == (7 + item / 255) * 255 + item % 255);
            }
    }
    const uint32_t Ws[] = {1, 2, 4, 128, 256, 2048, 1u << 17}, Ks[] = {1, 3, 255};
    for (uint32_t W : Ws)
        for (uint32_t K : Ks) {
            // the band lengths: L - 1, L and L + 1 for every lane-group width, the rule's thresholds 16 L and 16 L + 1, and the whole window
            std::vector<uint32_t> lens = {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 1025, 4096, 4097, W};
            for (uint32_t len : lens) {
                if (len > W) continue;
                std::vector<Band> bands;
                for (uint32_t k = 0; k < K; ++k) {
                    // band 0 is the long one and ends at W (lo is then not a multiple of 4 whenever len is not); the others are
                    // shorter, start off a multiple of 4 where they fit, overlap and repeat
                    uint32_t ln = k == 0 ? len : 1 + (k * 7) % len, lo = k == 0 ? W - len : (k * 5 + 1) % (W - ln + 1);
                    bands.push_back(Band{lo, lo + ln});
                }
                // window counts that leave the last workgroup partly filled, in one launch and cut into batches
                const uint64_t n = W > 4096 ? 2 : (K == 255 ? 3 : 5);
                walk(W, bands, n, n, lanes_for(len));
                walk(W, bands, n, 2, lanes_for(len));
                if (K == 1 && W <= 256) walk(W, bands, 67, 13, lanes_for(len));     // 67 items: no multiple of 64, 16 or 4
                if (K == 3 && W <= 256) walk(W, bands, 171, 171, lanes_for(len));   // 513 items: two workgroups and one item at L = 1
            }
        }
    std::printf("ok: %llu launches, %llu bins\n", g_launches, g_bins);
    return 0;
}
"""


def test_every_lane_of_every_launch(tmp_path):
    """Over W in {1, 2, 4, 128, 256, 2048, 2^17}, K in {1, 3, 255} and longest bands of L - 1, L, L + 1 bins for every lane-group width, at the
    rule's thresholds and of the whole window (hi = W, lo off a multiple of 4), the range in one launch and cut into batches, item
    counts that are no multiple of the items per workgroup: the lane-group width is the rule's; the lanes of a group share one item and
    an inactive group has none; a lane's bins lie inside its band, consecutive lanes on consecutive words; every (window, band, bin) is
    taken exactly once and nothing else is; every (window, band) is stored exactly once, at its place in the range's rows."""
    src = tmp_path / "walk_bands.cpp"
    src.write_text(WALKER)
    exe = tmp_path / "walk_bands"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
