// cuts_host_check.cpp — the cut list's host planning (quadrs_amd/csrc/qd_cuts_plan.h: cuts_check, cuts_batches, cuts_tiles,
// cut_of_emission) in a stand-alone program, for the sanitizers: random cut lists and budgets against brute force written here.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wextra -o cuts_host_check scripts/cuts_host_check.cpp
//   ./cuts_host_check [rounds = 200]
// Checked per round: every output of every cut lies in exactly one tile of exactly one batch, at the place in `out` (or in the batch's own
// buffer) the layout gives it; a tile's reads fit the LDS tile and its rows the row slots; a batch's merged spans are sorted, disjoint,
// exactly the union of its pieces' reads, within budget unless the batch is one tile; every sample a tile reads lies inside the upload
// (or the slab) at the element src_off says.  Then the emission arithmetic on its edges against loops.
#include "../quadrs_amd/csrc/qd_cuts_plan.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

using namespace qd;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(uint64_t n) { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (g_rng >> 24) % n; }

#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) { printf("cuts_host_check: FAILED %s (line %d, round %d)\n", #cond, __LINE__, g_round); exit(1); } \
    } while (0)
static int g_round = 0;

static void one_round() {
    const uint64_t n_samples = 1 + rnd(3) * 1000000 + rnd(400000);
    const size_t n_cuts = rnd(40);
    std::vector<qd_cut> cuts;
    static const uint64_t kD[] = {1, 2, 3, 4, 7, 32, 64, 100, 1024}, kT[] = {2, 40, 64, 200, 256, 4096};
    for (size_t k = 0; k < n_cuts; ++k) {
        qd_cut c{};
        c.decimate = kD[rnd(9)]; c.taps = kT[rnd(6)];
        c.shift_hz = rnd(2) ? (int64_t)rnd(1000) - 500 : 0;
        c.lowpass_hz = 1 + rnd(1000);
        if (n_samples <= c.taps + c.decimate) { c.count = 0; c.first = rnd(1000); cuts.push_back(c); continue; }
        const uint64_t room = (n_samples - c.taps) / c.decimate;                    // first + count <= room
        const uint64_t kinds[] = {0, 1, 255, 256, 257, 1 + rnd(3000), 1 + rnd(100000)};
        c.count = std::min<uint64_t>(kinds[rnd(7)], room);
        c.first = c.count < room ? rnd(room - c.count + 1) : 0;
        cuts.push_back(c);
    }
    std::vector<uint64_t> offs(n_cuts + 1);
    uint64_t hull0 = 0, hulln = 0;
    std::string err;
    CHECK(cuts_check(21000000, n_samples, cuts.data(), n_cuts, false, 0, 0, offs.data(), &hull0, &hulln, &err) == QD_OK);
    CHECK(cuts_check(21000000, n_samples, cuts.data(), n_cuts, true, hull0, hulln, nullptr, nullptr, nullptr, &err) == QD_OK);
    uint64_t lo = ~0ull, hi = 0, total = 0;
    for (size_t k = 0; k < n_cuts; ++k) {
        CHECK(offs[k] == total);
        total += cuts[k].count;
        if (!cuts[k].count) continue;
        lo = std::min(lo, cuts[k].first * cuts[k].decimate);
        hi = std::max(hi, cuts[k].first * cuts[k].decimate + cuts[k].count * cuts[k].decimate + cuts[k].taps);
        CHECK(hi <= n_samples);
    }
    CHECK(offs[n_cuts] == total && hull0 == (hi ? lo : 0) && hulln == (hi ? hi - lo : 0));
    if (hi) {                                                                        // a slab one sample short on either side is refused
        CHECK(cuts_check(21000000, n_samples, cuts.data(), n_cuts, true, hull0 + 1, hulln - 1, nullptr, nullptr, nullptr, &err) == QD_ERR_INVALID);
        CHECK(cuts_check(21000000, n_samples, cuts.data(), n_cuts, true, hull0, hulln - 1, nullptr, nullptr, nullptr, &err) == QD_ERR_INVALID);
        CHECK(cuts_check(21000000, hi - 1, cuts.data(), n_cuts, false, 0, 0, nullptr, nullptr, nullptr, &err) == QD_ERR_SHORT);
    }

    const uint64_t budgets[] = {1, 8192, 65536, 1 << 20, 8ull << 20};
    const uint64_t budget = budgets[rnd(5)];
    std::vector<CutBatch> batches;
    cuts_batches(cuts.data(), n_cuts, budget, &batches);
    std::vector<std::vector<uint8_t>> seen(n_cuts);
    for (size_t k = 0; k < n_cuts; ++k) seen[k].assign(cuts[k].count, 0);
    for (const bool direct_out : {false, true})
        for (const bool direct_src : {false, true}) {
            for (auto &s : seen) std::fill(s.begin(), s.end(), 0);
            for (const CutBatch &b : batches) {
                CHECK(!b.pieces.empty() && b.tiles <= kCutsBatchTiles);
                // the merged spans: sorted, disjoint, not adjacent, laid out back to back; exactly the union of the pieces' reads
                uint64_t at = 0;
                for (size_t s = 0; s < b.spans.size(); ++s) {
                    CHECK(b.spans[s].count > 0 && b.spans[s].at == at);
                    if (s) CHECK(b.spans[s].first > b.spans[s - 1].first + b.spans[s - 1].count);
                    at += b.spans[s].count;
                }
                CHECK(at == b.src_samples);
                std::map<uint64_t, int> edges;                                       // a sweep over the pieces' reads
                uint64_t out_at = 0, n_tiles = 0;
                for (const CutPiece &p : b.pieces) {
                    const qd_cut &c = cuts[p.cut];
                    uint64_t a, e;
                    cut_reads(c, p.first, p.count, &a, &e);
                    CHECK(a == p.lo && e == p.hi && a < e);
                    const CutSpan &sp = b.spans[p.span];
                    CHECK(sp.first <= a && e <= sp.first + sp.count);
                    edges[a] += 1; edges[e] -= 1;
                    CHECK(p.out_at == out_at);
                    out_at += p.count;
                    n_tiles += cut_piece_tiles(c, p);
                }
                CHECK(out_at == b.out_samples && n_tiles == b.tiles);
                uint64_t covered = 0, open_at = 0;
                int depth = 0;
                std::vector<std::pair<uint64_t, uint64_t>> uni;
                for (const auto &[x, d] : edges) {
                    if (depth == 0 && d > 0) open_at = x;
                    depth += d;
                    if (depth == 0 && d != 0) {
                        if (!uni.empty() && uni.back().second == open_at) uni.back().second = x; else uni.push_back({open_at, x});
                    }
                }
                CHECK(uni.size() == b.spans.size());
                for (size_t s = 0; s < uni.size(); ++s) { CHECK(uni[s].first == b.spans[s].first && uni[s].second - uni[s].first == b.spans[s].count); covered += b.spans[s].count; }
                CHECK(covered == b.src_samples);
                CHECK(b.src_samples <= budget || b.tiles == 1);
                // the tiles
                std::vector<CutTile> tiles;
                cuts_tiles(cuts.data(), b, direct_out, offs.data(), direct_src, hull0, &tiles);
                CHECK(tiles.size() == b.tiles);
                for (const CutTile &t : tiles) {
                    const qd_cut &c = cuts[t.job];
                    CHECK(t.count >= 1 && t.count <= cuts_tile_outputs(c.decimate, c.taps) && (uint64_t)t.first + t.count <= c.count);
                    uint64_t a, e;
                    cut_reads(c, t.first, t.count, &a, &e);
                    CHECK(e - a <= kCutsTileSamples);
                    CHECK((e - 1) / kCutsNcoRow - a / kCutsNcoRow + 1 <= kCutsTileRows);
                    CHECK(cuts_lds_index((uint32_t)(e - a - 1)) < kCutsLdsSamples);
                    const int64_t e0 = (int64_t)a + t.src_off, e1 = (int64_t)e + t.src_off;      // elements of the source buffer
                    if (direct_src) CHECK(e0 >= 0 && (uint64_t)e1 <= hulln && (uint64_t)e0 == a - hull0);
                    else {
                        CHECK(e0 >= 0 && (uint64_t)e1 <= b.src_samples);
                        bool inside = false;
                        for (const CutSpan &sp : b.spans) inside |= sp.first <= a && e <= sp.first + sp.count && (uint64_t)e0 == sp.at + (a - sp.first);
                        CHECK(inside);
                    }
                    for (uint32_t i = 0; i < t.count; ++i) {
                        CHECK(seen[t.job][t.first + i] == 0);
                        seen[t.job][t.first + i] = 1;
                        // the last tap of output i stays inside the tile's reads
                        const uint64_t D = c.decimate, T = c.taps, base = (uint64_t)(t.first + i) * D + (T - T / 2), valid = c.count * D + T;
                        const uint64_t jmax = std::min<uint64_t>(T, valid - base);
                        CHECK(jmax >= 1 && c.first * D + base >= a && c.first * D + base + jmax <= e);
                    }
                    if (direct_out) CHECK(t.out_at == offs[t.job] + t.first);
                    else CHECK(t.out_at + t.count <= b.out_samples);
                }
                if (!direct_out) {                                                   // the batch's own buffer: every element written once
                    std::vector<uint8_t> own(b.out_samples, 0);
                    for (const CutTile &t : tiles) for (uint32_t i = 0; i < t.count; ++i) { CHECK(own[t.out_at + i] == 0); own[t.out_at + i] = 1; }
                    for (uint8_t v : own) CHECK(v == 1);
                }
            }
            for (size_t k = 0; k < n_cuts; ++k) for (uint8_t v : seen[k]) CHECK(v == 1);
        }
}

static void refusals() {
    std::string err;
    qd_cut c{};
    c.decimate = 4; c.taps = 40; c.count = 10; c.first = 100; c.lowpass_hz = 1000;
    auto code = [&](const qd_cut &x) { return cuts_check(1000, 100000, &x, 1, false, 0, 0, nullptr, nullptr, nullptr, &err); };
    CHECK(code(c) == QD_OK);
    qd_cut x = c; x.decimate = 0; CHECK(code(x) == QD_ERR_PANIC);
    x = c; x.taps = 1; CHECK(code(x) == QD_ERR_PANIC);
    x = c; x.shift_hz = 500; CHECK(code(x) == QD_ERR_PANIC);
    x = c; x.shift_hz = -500; CHECK(code(x) == QD_ERR_PANIC);
    x = c; x.shift_hz = INT64_MIN; CHECK(code(x) == QD_ERR_PANIC);
    x = c; x.shift_hz = 499; CHECK(code(x) == QD_OK);
    x = c; x.decimate = QD_CUT_MAX_DECIMATE + 1; CHECK(code(x) == QD_ERR_UNSUPPORTED);
    x = c; x.taps = QD_CUT_MAX_TAPS + 1; CHECK(code(x) == QD_ERR_UNSUPPORTED);
    x = c; x.count = kCutsMaxCount + 1; CHECK(code(x) == QD_ERR_UNSUPPORTED);
    x = c; x.first = ~0ull; CHECK(code(x) == QD_ERR_SHORT);
    x = c; x.first = (100000 - 80) / 4 + 1; CHECK(code(x) == QD_ERR_SHORT);
    x = c; x.first = (100000 - 80) / 4; CHECK(code(x) == QD_OK);
    x = c; x.count = 0; x.first = ~0ull; CHECK(code(x) == QD_OK);
    CHECK(cuts_check(1000, 100000, nullptr, 1, false, 0, 0, nullptr, nullptr, nullptr, &err) == QD_ERR_INVALID);
    CHECK(cuts_check(1000, 100000, nullptr, 0, false, 0, 0, nullptr, nullptr, nullptr, &err) == QD_OK);
}

static void emission_edges() {
    typedef cuts_i128 I;
    for (int a = -40; a <= 40; ++a)
        for (int b = 1; b <= 9; ++b) {
            int f = -100, c = 100;
            while ((f + 1) * b <= a) ++f;                                             // the largest f with f b <= a
            while ((c - 1) * b >= a) --c;
            CHECK(cuts_fdiv(a, b) == f && cuts_cdiv(a, b) == c);
        }
    std::string err;
    for (int round = 0; round < 4000; ++round) {
        qd_chain_desc d{};
        d.struct_size = sizeof d;
        d.sample_rate = 2 + rnd(round % 2 ? 50 : 4000000);
        d.width = 1 + rnd(round % 3 ? 16 : 4096);
        d.stride = 1 + rnd(2 * d.width);
        d.n_samples = rnd(3) ? rnd(1 << 20) : rnd(64);
        if (rnd(2)) { d.has_shift = 1; d.shift_hz = (int64_t)rnd(d.sample_rate / 2 ? d.sample_rate / 2 : 1) * (rnd(2) ? 1 : -1); }
        if (rnd(2)) { d.has_lowpass = 1; d.decimate = 1 + rnd(40); d.taps = 2 + rnd(300); d.lowpass_hz = 1 + rnd(1000); }
        qd_emission e{};
        e.first = rnd(5000); e.last = e.first + rnd(200);
        e.lo = (uint32_t)rnd(d.width); e.hi = e.lo + (uint32_t)rnd(d.width - e.lo);
        qd_cut_rule r{};
        r.struct_size = sizeof r; r.guard_bins = (uint32_t)rnd(4); r.oversample = 1 + (uint32_t)rnd(4); r.pad = (uint32_t)rnd(6);
        r.taps = rnd(2) ? 0 : 2 + rnd(600); r.max_decimate = rnd(2) ? 0 : 1 + rnd(2000);
        qd_cut c{};
        const uint64_t fw = rnd(3) ? 0 : rnd(100000);
        CHECK(cut_of_emission(&d, fw, &e, &r, &c, &err) == QD_OK);
        const I sr = (I)d.sample_rate, D0 = d.has_lowpass ? (I)d.decimate : 1, R = sr / D0, W = (I)d.width;
        // the shift: inside Shift::new's range, and it moves the centre of the bins (in units of R / 2W) onto a multiple of sr
        CHECK((I)c.shift_hz > -(sr / 2) || sr / 2 == 0 || (I)c.shift_hz == 1 - sr / 2);
        if (sr >= 4) CHECK((I)c.shift_hz < sr / 2 && -(I)c.shift_hz < sr / 2);
        const I f0 = d.has_shift ? (I)d.shift_hz : 0, twice = ((I)e.lo + (I)e.hi - W) * R + W;      // 2W nu <= twice < 2W (nu + 1)
        I nu = -((I)1 << 60);
        { I l = -((I)1 << 60), h = (I)1 << 60; while (l < h) { const I m = l + (h - l + 1) / 2; if (m * 2 * W <= twice) l = m; else h = m - 1; } nu = l; }
        const I landed = ((f0 - nu - (I)c.shift_hz) % sr + sr) % sr;
        CHECK(landed == 0 || (I)c.shift_hz == 1 - sr / 2);
        CHECK(c.lowpass_hz >= 1 && (I)c.lowpass_hz * 2 * W >= ((I)e.hi - (I)e.lo + 1 + 2 * (I)r.guard_bins) * R);
        CHECK(c.decimate >= 1 && c.decimate <= (r.max_decimate ? r.max_decimate : QD_CUT_MAX_DECIMATE));
        CHECK(r.taps ? c.taps == r.taps : (c.taps >= 40 && c.taps <= QD_CUT_MAX_TAPS));
        // a cut with outputs is one full block of the stream
        if (c.count) CHECK((I)c.first * (I)c.decimate + (I)c.count * (I)c.decimate + (I)c.taps <= (I)d.n_samples);
    }
    qd_chain_desc d{};
    d.struct_size = sizeof d; d.sample_rate = 1000; d.width = 8; d.stride = 8; d.n_samples = 100000;
    qd_emission e{};
    e.last = 3; e.hi = 2;
    qd_cut_rule r{};
    r.struct_size = sizeof r; r.oversample = 1;
    qd_cut c{};
    CHECK(cut_of_emission(&d, 0, &e, &r, &c, &err) == QD_OK);
    CHECK(cut_of_emission(&d, ~0ull, &e, &r, &c, &err) == QD_ERR_UNSUPPORTED);
    d.stride = ~0ull; CHECK(cut_of_emission(&d, 5, &e, &r, &c, &err) == QD_ERR_UNSUPPORTED);
    d.stride = 8; d.sample_rate = 1ull << 48; CHECK(cut_of_emission(&d, 0, &e, &r, &c, &err) == QD_ERR_UNSUPPORTED);
    d.sample_rate = 1000; r.oversample = 0; CHECK(cut_of_emission(&d, 0, &e, &r, &c, &err) == QD_ERR_INVALID);
    r.oversample = 1; r.taps = 1; CHECK(cut_of_emission(&d, 0, &e, &r, &c, &err) == QD_ERR_INVALID);
    r.taps = 0; e.hi = 8; CHECK(cut_of_emission(&d, 0, &e, &r, &c, &err) == QD_ERR_INVALID);
    e.hi = 2; e.lo = 3; CHECK(cut_of_emission(&d, 0, &e, &r, &c, &err) == QD_ERR_INVALID);
    e.lo = 0; CHECK(cut_of_emission(&d, 0, &e, nullptr, &c, &err) == QD_ERR_INVALID);
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    refusals();
    emission_edges();
    for (g_round = 0; g_round < rounds; ++g_round) one_round();
    printf("cuts_host_check: ok (%d rounds)\n", rounds);
    return 0;
}
