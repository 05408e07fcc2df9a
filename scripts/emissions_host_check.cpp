// emissions_host_check.cpp — the emission list's CPU twin (quadrs_amd/csrc/qd_emissions.h: emissions_twin_init / _row / _finish, what
// qd_emissions_fold and qd_emissions_finish run) in a stand-alone program, for scripts/sanitize_cpu.sh: random on/off matrices with tied
// peaks, NaN cells and masked bins, folded row by row into lists with and without room, against a flood fill written here.
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 -Wall -Wextra -o emissions_host_check scripts/emissions_host_check.cpp
//   ./emissions_host_check [rounds = 400]
#include "../quadrs_amd/csrc/qd_emissions.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

using namespace qd;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33) % n; }

static std::vector<Emission> flood(const std::vector<uint32_t> &bits, const std::vector<uint32_t> &thr, uint32_t n, uint32_t W, uint64_t min_len, uint64_t min_cells) {
    std::vector<uint8_t> on((size_t)n * W), seen((size_t)n * W, 0);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t b = 0; b < W; ++b) on[(size_t)i * W + b] = bursts_on(bursts_mag(bits[(size_t)i * W + b]), thr[b]);
    std::vector<Emission> out;
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    for (uint32_t i0 = 0; i0 < n; ++i0)
        for (uint32_t b0 = 0; b0 < W; ++b0) {
            if (!on[(size_t)i0 * W + b0] || seen[(size_t)i0 * W + b0]) continue;
            seen[(size_t)i0 * W + b0] = 1;
            stack.assign(1, {i0, b0});
            Emission e{};
            bool first = true;
            while (!stack.empty()) {
                const auto [i, b] = stack.back();
                stack.pop_back();
                const Emission c = emissions_cell(i, b, bursts_mag(bits[(size_t)i * W + b]));
                if (first) { e = c; first = false; } else emissions_join(e, c);
                const int di[4] = {-1, 1, 0, 0}, db[4] = {0, 0, -1, 1};
                for (int k = 0; k < 4; ++k) {
                    const int64_t j = (int64_t)i + di[k], c2 = (int64_t)b + db[k];
                    if (j < 0 || j >= n || c2 < 0 || c2 >= W) continue;
                    const size_t at = (size_t)j * W + (size_t)c2;
                    if (on[at] && !seen[at]) { seen[at] = 1; stack.push_back({(uint32_t)j, (uint32_t)c2}); }
                }
            }
            if (e.last == n - 1) e.flags |= kEmissionsCutLast;
            if (emissions_kept(e.first, e.last, e.cells, min_len, min_cells)) out.push_back(e);
        }
    std::sort(out.begin(), out.end(), [](const Emission &a, const Emission &b) { return a.last != b.last ? a.last < b.last : a.end_bin < b.end_bin; });
    return out;
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 400;
    const uint32_t levels[] = {0x3f800000u, 0x3fc00000u, 0x40000000u, 0x40000000u, 0x7f800000u, 0x7fc00000u, 0x3f000000u, 0u, 0xbfc00000u};
    uint64_t total = 0;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t W = 1 + rnd(round % 4 == 0 ? 3 : 40), n = rnd(60);
        const uint32_t density = 1 + rnd(9);
        std::vector<uint32_t> bits((size_t)n * W), thr(W);
        for (uint32_t &x : bits) x = rnd(10) < density ? levels[rnd(6)] : levels[6 + rnd(3)];
        for (uint32_t b = 0; b < W; ++b) {
            const uint32_t pick = rnd(10);
            if (!bursts_threshold(pick == 0 ? 0u : pick == 1 ? 0x7fc00000u : pick == 2 ? 0x7f800000u : 0x3f800000u, &thr[b])) return 2;
        }
        const uint64_t min_len = 1 + rnd(3), min_cells = 1 + rnd(4);
        const std::vector<Emission> ref = flood(bits, thr, n, W, min_len, min_cells);
        for (uint64_t cap : {(uint64_t)ref.size() + 1, (uint64_t)ref.size() / 2, (uint64_t)0}) {
            std::vector<uint64_t> state((size_t)kEmissionsWords * W + 2);
            std::vector<Emission> list(cap);                                  // exactly cap records: ASan guards the end
            uint64_t found = 0;
            const EmissionsSink sink{cap ? list.data() : nullptr, cap, &found, min_len, min_cells};
            emissions_twin_init(state.data(), W);
            for (uint32_t i = 0; i < n; ++i) emissions_twin_row(state.data(), W, thr.data(), i, bits.data() + (size_t)i * W, sink);
            emissions_twin_finish(state.data(), W, sink);
            if (found != ref.size()) { std::printf("FAILED round %d: found %llu, flood fill %zu\n", round, (unsigned long long)found, ref.size()); return 1; }
            const size_t k = (size_t)std::min<uint64_t>(found, cap);
            if (k && memcmp(list.data(), ref.data(), k * sizeof(Emission)) != 0) { std::printf("FAILED round %d: the lists differ (cap %llu)\n", round, (unsigned long long)cap); return 1; }
            if (state[0] != kEmissionsNone || state[(size_t)kEmissionsWords * W] != 0) { std::printf("FAILED round %d: _finish left a state\n", round); return 1; }
        }
        total += ref.size();
    }
    std::printf("ok: %d rounds, %llu emissions\n", rounds, (unsigned long long)total);
    return 0;
}
