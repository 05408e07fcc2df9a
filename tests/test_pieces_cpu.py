"""The piece geometry of the pooled folds (k_pool, k_mean, k_density; quadrs_amd/csrc/qd_pieces.h) on the CPU: the
header is host-clean, and a stand-alone program that includes nothing else walks every (workgroup, slot) of every launch of a range cut
into batches, for both kernels' column layouts, and checks what the kernels rely on.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrs_amd", "csrc")


def test_piece_rules_live_in_one_host_clean_header(tmp_path):
    tu = tmp_path / "only_pieces.cpp"
    tu.write_text('#include "qd_pieces.h"\nint main() { qd::PieceGeometry G; uint64_t grid; qd::piece_split(0, 1, 1, 1, 4, 4, 1, 256, 16, 4, 1, &G, &grid);\n'
                  '    return qd::piece_lane(G, 0, 0).whole(G) ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the derivations exist once: no fold header or host source carries its own copy
    for name in ("qd_pool.h", "qd_mean.h", "qd_density.h", "quadrs_hip.hip"):
        text = open(os.path.join(CSRC, name), encoding="utf-8").read()
        for phrase in ("wg_q0 + P.pieces_per_group", "wg_q0 + P->pieces_per_group", "* P.spr", "(want + rows - 1) / rows"):
            assert phrase not in text, (name, phrase)


WALKER = r"""
#include "qd_pieces.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace qd;

struct Layout { const char *name; uint32_t cols, lanes_per_win, pieces_per_group; uint64_t min_seg; };
// k_pool / k_mean: V 4 or 1, slabs of 1024 bins, 256 lanes, shortest piece 16
static Layout pool_layout(uint32_t W) {
    const uint32_t V = W >= 4 ? 4 : 1, cols = W < 1024 ? W : 1024, lpw = cols / V;
    return {"pool", cols, lpw, 256 / lpw, 16};
}
// k_density: ncol columns from the number of levels, one lane a bin, shortest piece 128
static Layout density_layout(uint32_t W, uint32_t L) {
    uint32_t ncol = 64;
    while (ncol * 2 * L <= 16384 && ncol * 2 <= 256) ncol *= 2;
    const uint32_t cols = W < ncol ? W : ncol;
    return {"density", cols, cols, ncol / cols, 128};
}

static const char *g_what = "";
static unsigned long long g_ctx[8];
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s: %s\n  %s W %llu n %llu pool %llu batch %llu n_cu %llu g0 %llu block %llu slot %llu\n", #c, g_what, g_what, \
    g_ctx[0], g_ctx[1], g_ctx[2], g_ctx[3], g_ctx[4], g_ctx[5], g_ctx[6], g_ctx[7]); std::exit(1); } } while (0)

static unsigned long long g_launches = 0;

static void walk(const Layout &lay, uint32_t W, uint64_t n, uint64_t pool, uint64_t bw, int n_cu) {
    g_what = lay.name;
    g_ctx[0] = W; g_ctx[1] = n; g_ctx[2] = pool; g_ctx[3] = bw; g_ctx[4] = (unsigned long long)n_cu;
    const uint32_t n_slabs = W / lay.cols;
    const uint64_t R = (n - 1) / pool + 1;
    std::vector<uint32_t> cover(n * n_slabs, 0), flushed(R * n_slabs, 0), whole(R * n_slabs, 0);
    std::vector<PieceLane> lanes(lay.pieces_per_group);
    for (uint64_t g0 = 0; g0 < n; g0 += bw) {
        const uint64_t nw = n - g0 < bw ? n - g0 : bw;
        g_ctx[5] = g0;
        PieceGeometry G;
        uint64_t grid = 0;
        piece_split(g0, nw, n, pool, W, lay.cols, lay.lanes_per_win, lay.pieces_per_group, lay.min_seg, 4, n_cu, &G, &grid);
        ++g_launches;
        CHECK(G.n_slabs == n_slabs && grid > 0 && grid % n_slabs == 0 && grid <= 0x7fffffffull);
        CHECK(G.seg >= 1 && G.seg <= pool && G.spr == (pool + G.seg - 1) / G.seg);
        for (uint64_t block = 0; block < grid; ++block) {
            g_ctx[6] = block;
            bool any = false;
            for (uint32_t slot = 0; slot < lay.pieces_per_group; ++slot) {
                g_ctx[7] = slot;
                const PieceLane l = lanes[slot] = piece_lane(G, (uint32_t)block, slot);
                CHECK(l.slab < n_slabs && l.end == g0 + nw);
                if (!l.active) { CHECK(l.wa == l.wb); continue; }
                any = true;
                CHECK(l.r < R && l.row_a == l.r * pool && l.row_b == (l.row_a + pool < n ? l.row_a + pool : n));
                CHECK(g0 <= l.wa && l.wa <= l.wb && l.wb <= g0 + nw);
                CHECK(l.row_a <= l.wa && l.wb <= l.row_b);
                for (uint64_t w = l.wa; w < l.wb; ++w) cover[w * n_slabs + l.slab] += 1;
                CHECK(l.lead <= slot && lanes[l.lead].active && lanes[l.lead].r == l.r && lanes[l.lead].slab == l.slab);
            }
            CHECK(any);
            for (uint32_t slot = 0; slot < lay.pieces_per_group; ++slot) {
                g_ctx[7] = slot;
                const PieceLane &l = lanes[slot];
                if (!l.active || l.lead != slot) continue;
                // the leader: slots lead ... lead + n_same - 1 are the row's pieces here, and no other slot is
                const uint32_t n_same = l.n_same(G);
                CHECK(n_same >= 1 && slot + n_same <= lay.pieces_per_group);
                for (uint32_t s = 0; s < lay.pieces_per_group; ++s)
                    CHECK((lanes[s].active && lanes[s].r == l.r) == (s >= slot && s < slot + n_same));
                flushed[l.r * n_slabs + l.slab] += 1;
                if (l.whole(G)) whole[l.r * n_slabs + l.slab] += 1;
            }
        }
    }
    g_ctx[5] = g_ctx[6] = g_ctx[7] = ~0ull;
    for (uint64_t i = 0; i < n * n_slabs; ++i) CHECK(cover[i] == 1);
    for (uint64_t i = 0; i < R * n_slabs; ++i) {
        CHECK(flushed[i] >= 1);
        CHECK(whole[i] == 0 || (whole[i] == 1 && flushed[i] == 1));
    }
}

int main() {
    const uint32_t Ws[] = {1, 2, 4, 64, 256, 1024, 4096}, Ls[] = {1, 64, 65, 256};
    const uint64_t ns[] = {1, 37, 1000}, pools[] = {1, 3, 16, 17, 500, 0}, bws[] = {0, 7, 48, 129};      // 0: n
    const int cus[] = {1, 256};
    for (uint32_t W : Ws)
        for (uint64_t n : ns)
            for (uint64_t pool_ : pools)
                for (uint64_t bw_ : bws)
                    for (int n_cu : cus) {
                        const uint64_t pool = pool_ && pool_ < n ? pool_ : n, bw = bw_ ? bw_ : n;       // the entry points clamp pool to one row
                        walk(pool_layout(W), W, n, pool, bw, n_cu);
                        for (uint32_t L : Ls) walk(density_layout(W, L), W, n, pool, bw, n_cu);
                    }
    std::printf("ok: %llu launches\n", g_launches);
    return 0;
}
"""


def test_every_slot_of_every_launch(tmp_path):
    """Over W in {1 ... 4096}, n in {1, 37, 1000}, pool in {1, 3, 16, 17, 500, n}, batches of {n, 7, 48, 129} windows and 1 or 256 compute
    units, with k_pool's / k_mean's layout and k_density's at L in {1, 64, 65, 256}: an inactive slot has an empty span; an active slot's
    span lies inside the batch and inside its row; lead <= slot is an active slot of the same row, and a leader's n_same names exactly
    the row's slots; every (window, slab) is covered exactly once over the partition; every workgroup has an active slot; the grid is a
    multiple of n_slabs; a (row, slab) flushed whole is flushed once and by nobody else; every (row, slab) is flushed."""
    src = tmp_path / "walk_pieces.cpp"
    src.write_text(WALKER)
    exe = tmp_path / "walk_pieces"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
