// symbols_host_check.cpp — the symbol list's host planning (quadrs_amd/csrc/qd_symbols_plan.h: symbols_windows, symbols_check,
// symbols_tiles, symbols_groups) in a stand-alone program, for the sanitizers: random segment lists against brute force written here.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -Wextra -o symbols_host_check scripts/symbols_host_check.cpp
//   ./symbols_host_check [rounds = 200]
// Checked per round: the window counts against the reference's loops run as loops; the offsets are the prefix sums of the rule and the
// hull is that of the segments with a window; every window of every segment lies in exactly one tile, at the byte the layout gives it,
// whatever the size of the batches the table is asked for in; a tile fits its wave's LDS slice and every sample it reads lies inside
// its segment (and inside the uploaded hull at the element src_at says); the groups of qd_cuts_symbols cover every cut once, in order,
// within the cap, and a cut above the cap is refused.
#include "../quadrs_amd/csrc/qd_symbols_plan.h"

#include <cstdlib>
#include <cstring>

using namespace qd;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(uint64_t n) { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (g_rng >> 24) % n; }

static int g_round = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) { printf("symbols_host_check: FAILED %s (line %d, round %d)\n", #cond, __LINE__, g_round); exit(1); } \
    } while (0)

// the reference's loops, run (src/fft.rs:86: for i in 0..(len - W) / S; src/fft.rs:28,65: while i < len - W { i += S })
static uint64_t brute_windows(int epi, uint64_t count, uint64_t W, uint64_t S) {
    if (count <= W) return 0;                                                  // the stated departure: the reference underflows here
    uint64_t n = 0;
    if (epi == QD_EPI_BUCKET2_U8) { for (uint64_t i = 0; i < (count - W) / S; ++i) ++n; }
    else { for (uint64_t i = 0; i < count - W; i += S) ++n; }
    return n;
}

static void one_round() {
    static const uint64_t kW[] = {1, 2, 4, 8, 16, 64, 256, 1024, 2048, 4096};
    qd_symbols_desc d{};
    d.struct_size = sizeof d;
    d.epilogue = rnd(2) ? QD_EPI_BUCKET2_U8 : QD_EPI_MARK_U8;
    d.width = kW[rnd(10)];
    const uint64_t W = d.width;
    const uint64_t strides[] = {1, W / 2 ? W / 2 : 1, W, W + 3, 1 + rnd(3 * W), (1ull << 31) + rnd(5), ~0ull};
    d.stride = strides[rnd(7)];
    if (d.stride == 1 && W <= 4 && rnd(2)) d.stride = W;                       // (keep the brute force loops short)
    const uint64_t S = d.stride;
    const uint64_t n_in = 1 + rnd(300000);
    const size_t n = rnd(50);
    std::vector<qd_segment> segs(n);
    for (size_t k = 0; k < n; ++k) {
        const uint64_t kinds[] = {0, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 3 * W + 5, 1000, 4099, rnd(40000)};
        uint64_t c = kinds[rnd(11)];
        if (c > n_in || S > (1ull << 40)) c = std::min<uint64_t>(c > n_in ? rnd(n_in + 1) : c, n_in);
        segs[k].count = c;
        segs[k].first = rnd(n_in - c + 1);
    }
    std::vector<uint64_t> offs(n + 1);
    uint64_t hull0 = 0, hulln = 0;
    std::string err;
    CHECK(symbols_check(&d, segs.data(), n, true, n_in, offs.data(), &hull0, &hulln, &err) == QD_OK);
    CHECK(symbols_check(&d, segs.data(), n, false, 0, nullptr, nullptr, nullptr, &err) == QD_OK);
    uint64_t total = 0, lo = ~0ull, hi = 0;
    for (size_t k = 0; k < n; ++k) {
        CHECK(offs[k] == total);
        const uint64_t nw = brute_windows(d.epilogue, segs[k].count, W, S);
        CHECK(nw == symbols_windows(d.epilogue, segs[k].count, W, S));
        total += nw;
        if (nw) { lo = std::min(lo, segs[k].first); hi = std::max(hi, segs[k].first + segs[k].count); }
    }
    CHECK(offs[n] == total && hull0 == (hi ? lo : 0) && hulln == (hi ? hi - lo : 0));
    if (n) {                                                                    // a buffer one sample short of the farthest segment is refused
        uint64_t far = 0;
        for (const qd_segment &s : segs) far = std::max(far, s.first + s.count);
        if (far) CHECK(symbols_check(&d, segs.data(), n, true, far - 1, nullptr, nullptr, nullptr, &err) == QD_ERR_SHORT);
    }

    // the tile table, asked for in batches of a random size
    const size_t cap = 1 + rnd(rnd(2) ? 7 : 5000);
    const uint64_t base = hull0;
    std::vector<uint8_t> seen((size_t)total, 0);
    std::vector<SymTile> tiles;
    SymCursor cur;
    size_t seg_at = 0;                                                          // tiles come in list order
    uint64_t expect_out = 0;
    for (bool more = true; more;) {
        more = symbols_tiles(&d, segs.data(), n, offs.data(), base, &cur, cap, &tiles);
        CHECK(tiles.size() <= cap && (!more || tiles.size() == cap));
        for (const SymTile &t : tiles) {
            CHECK(t.count >= 1 && (uint64_t)t.count * W <= symbols_slice(W) && t.count <= symbols_tile_windows(W));
            CHECK(t.out_at == expect_out);
            while (seg_at < n && t.out_at >= offs[seg_at + 1]) ++seg_at;
            CHECK(seg_at < n && t.out_at >= offs[seg_at] && t.out_at + t.count <= offs[seg_at + 1]);      // windows of ONE segment
            const qd_segment &s = segs[seg_at];
            const uint64_t r0 = t.out_at - offs[seg_at];
            CHECK(t.src_at + base == s.first + r0 * S);
            const uint64_t Sk = std::min<uint64_t>(S, 1ull << 31);            // the kernel's clamped stride
            for (uint32_t r = 0; r < t.count; ++r) {
                CHECK(r == 0 || S == Sk);                                       // a clamped stride never reaches a second window
                const uint64_t a = t.src_at + base + (uint64_t)r * Sk, b = a + W;
                CHECK(a >= s.first && b <= s.first + s.count);                  // the reads stay inside the segment ...
                CHECK(a >= hull0 && b <= hull0 + hulln && b <= n_in);           // ... and the upload
                CHECK(seen[(size_t)(t.out_at + r)] == 0);
                seen[(size_t)(t.out_at + r)] = 1;
            }
            expect_out += t.count;
        }
    }
    CHECK(expect_out == total);
    for (uint8_t v : seen) CHECK(v == 1);
    CHECK(symbols_waves(W) * symbols_slice(W) * 8 == kSymLdsBytes && (W <= 2048 ? symbols_waves(W) == 4 : symbols_waves(W) == 2));

    // the groups of qd_cuts_symbols
    const size_t n_cuts = rnd(40);
    std::vector<qd_cut> cuts(n_cuts);
    uint64_t largest = 0;
    for (qd_cut &c : cuts) { c = qd_cut{}; c.count = rnd(4) ? rnd(5000) : 0; largest = std::max(largest, c.count); }
    const uint64_t iq_bytes = std::max<uint64_t>(8, 8 * (largest + rnd(20000)) + rnd(8)), cap_samples = iq_bytes / 8;
    std::vector<std::pair<size_t, size_t>> groups;
    CHECK(symbols_groups(cuts.data(), n_cuts, iq_bytes, &groups, &err) == QD_OK);
    size_t at = 0;
    for (const auto &g : groups) {
        CHECK(g.first == at && g.second > g.first && g.second <= n_cuts);
        uint64_t held = 0;
        for (size_t k = g.first; k < g.second; ++k) held += cuts[k].count;
        CHECK(held <= cap_samples);
        if (g.second < n_cuts) CHECK(held + cuts[g.second].count > cap_samples);                   // greedy: the next cut did not fit
        at = g.second;
    }
    CHECK(at == n_cuts);
    if (largest > 1) {
        CHECK(symbols_groups(cuts.data(), n_cuts, 8 * (largest - 1), &groups, &err) == QD_ERR_UNSUPPORTED);
        CHECK(err.find("iq_bytes") != std::string::npos);
    }
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    for (g_round = 0; g_round < rounds; ++g_round) one_round();

    // the validation, in the header's order
    std::string err;
    qd_symbols_desc d{};
    d.struct_size = sizeof d; d.epilogue = QD_EPI_MARK_U8; d.width = 64; d.stride = 16;
    qd_segment seg[3] = {{0, 100}, {5, (1ull << 31) + 1}, {~0ull - 3, 8}};
    CHECK(symbols_check(nullptr, seg, 3, false, 0, nullptr, nullptr, nullptr, &err) == QD_ERR_INVALID);
    CHECK(symbols_check(&d, nullptr, 3, false, 0, nullptr, nullptr, nullptr, &err) == QD_ERR_INVALID);
    CHECK(symbols_check(&d, nullptr, 0, false, 0, nullptr, nullptr, nullptr, &err) == QD_OK);
    CHECK(symbols_check(&d, seg, 3, false, 0, nullptr, nullptr, nullptr, &err) == QD_ERR_UNSUPPORTED && err.find("segment 1") != std::string::npos);
    seg[1].count = 1ull << 31;
    CHECK(symbols_check(&d, seg, 3, false, 0, nullptr, nullptr, nullptr, &err) == QD_OK);
    CHECK(symbols_check(&d, seg, 3, true, 1ull << 32, nullptr, nullptr, nullptr, &err) == QD_ERR_SHORT && err.find("segment 2") != std::string::npos);
    qd_symbols_desc b = d;
    b.width = 48;   CHECK(symbols_check_desc(&b, &err) == QD_ERR_PANIC);
    b.width = 0;    CHECK(symbols_check_desc(&b, &err) == QD_ERR_PANIC);
    b.width = 8192; CHECK(symbols_check_desc(&b, &err) == QD_ERR_UNSUPPORTED);
    b.stride = 0;   CHECK(symbols_check_desc(&b, &err) == QD_ERR_INVALID);
    b = d; b.windowing = 2;             CHECK(symbols_check_desc(&b, &err) == QD_ERR_INVALID);
    b = d; b.epilogue = QD_EPI_NORMS_F32; CHECK(symbols_check_desc(&b, &err) == QD_ERR_INVALID);
    b = d; b.struct_size = 40;          CHECK(symbols_check_desc(&b, &err) == QD_ERR_INVALID);
    printf("symbols_host_check: ok (%d rounds)\n", rounds);
    return 0;
}
