"""The planted-value streams of test_gpu_planted.py (tests/util.py: impulse_stream, cases_stream, planted_case_set) on the CPU: the
construction against the oracle — a window whose first sample is (a, 0) and whose others are +0 has the norm |a| in every bin, bit for
bit, for every pattern the GPU tests plant — and, by a stand-alone walker compiled from qd_pieces.h alone, which ending every output row of
those streams takes on a device of 256 compute units: stored whole by one lane group, stored whole after the LDS meeting of its pieces, or
cut and sent through the limb accumulator and the finish kernel.  No GPU, no HIP."""
import subprocess

import numpy as np
import pytest

import util
from test_pieces_cpu import CSRC
from test_power_cpu import VALUE_CLASSES

N_CU = 256
WORDS = {"pool": 10, "power": 28}                # the widest cell on each column layout: k_mean's 10 words, k_spread's 28


def planted_patterns():
    """every pattern that test_gpu_planted.py plants, ascending"""
    first, rest = util.planted_cells()
    pats = {b for c in first + rest for b in c} | {int(b) for b in util.bucket_sweep()} | {b for b in VALUE_CLASSES if util.plantable([b])}
    return np.array(sorted(pats | {util.PLANT_NAN}), dtype=np.uint32)


@pytest.mark.parametrize("W", [1, 2, 4, 128, 256, 2048])
def test_an_impulse_window_has_its_value_in_every_bin(oracle, W):
    pats = planted_patterns()
    assert pats.size > 20000 and pats[0] == 0 and 1 in pats and util.PLANT_INF in pats and util.PLANT_MAX in pats and pats[-1] == util.PLANT_NAN
    nan = pats == util.PLANT_NAN
    for at in range(0, pats.size, 4096):
        p, isnan = pats[at:at + 4096], nan[at:at + 4096]
        out = oracle.Chain.from_bytes(util.impulse_stream(p, W), 0, util.PLANTED_SR).spark_fft(W, want_codes=False)[0]
        out = np.asarray(out, dtype=np.float32).reshape(-1, W)
        assert out.shape == (p.size, W)
        assert np.isnan(out[isnan]).all()
        assert (out.view(np.uint32)[~isnan] == p[~isnan][:, None]).all(), (W, at)


def test_the_stream_builders():
    data, m = util.cases_stream([[1, 2, 3], [], [util.PLANT_INF]], 4, 2)
    x = np.frombuffer(data, dtype=np.uint32).reshape(13, 2, 2)
    assert m.shape == (3, 4) and m.dtype == np.uint32 and [int(v) for v in m[0]] == [1, 2, 3, util.PLANT_NAN] and (m[1] == util.PLANT_NAN).all()
    assert (x[:12, 0, 0] == m.reshape(-1)).all() and not x[:, 1].any() and not x[:, :, 1].any() and not x[12].any()
    for bad in (0x80000000, 0xBF800000, 0x7F800001, 0xFFC00000):
        assert not util.plantable([1, bad])
        with pytest.raises(AssertionError):
            util.impulse_stream([bad], 4)
    sweep = util.exponent_sweep()
    assert len(sweep) == 255 * 3 + 4 and all(util.plantable(c) and 1 <= len(c) <= 4 for c in sweep)
    assert {c[0] >> 23 for c in sweep if len(c) == 1} == set(range(255))
    b = util.bucket_sweep()
    assert b.size == 4081 and (np.diff(b.astype(np.int64)) > 0).all() and b[-1] == util.PLANT_INF and b[-2] == util.PLANT_MAX
    assert (np.bincount(b >> 20, minlength=2041) == [2] * 2040 + [1]).all()
    # every stream fits, holds the discriminating cells first, and every cell runs somewhere at its own smallest depth at the narrow widths
    first, rest = util.planted_cells()
    for W in util.PLANTED_WIDTHS:
        seen = set()
        for depth in util.planted_depths(W):
            cells = util.planted_case_set(W, depth)
            assert (len(cells) * depth + 1) * W * 8 < util.PLANTED_CAP and all(len(c) <= depth for c in cells)
            lead = [c for c in first if len(c) <= depth]
            assert cells[:len(lead)] == lead[:len(cells)]
            seen |= {tuple(c) for c in cells}
        if W <= 4:
            assert {tuple(c) for c in first + rest if len(c) <= 64} <= seen
    assert sum(len(c) <= 64 for c in util.planted_cells()[1]) >= 2000 + len(sweep)


WALKER = r"""
#include "qd_pieces.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace qd;

struct Layout { uint32_t cols, lanes_per_win, pieces_per_group; uint64_t min_seg; };
// k_pool / k_mean (qd_pool.h, pool_geometry): V 4 or 1, slabs of 1024 bins, 256 lanes, shortest piece 16
static Layout pool_layout(uint32_t W) {
    const uint32_t V = W >= 4 ? 4 : 1, cols = W < 1024 ? W : 1024, lpw = cols / V;
    return {cols, lpw, 256 / lpw, 16};
}
// k_power / k_spread as shipped (qd_power.h, power_geometry's V = 1 form): a lane a bin, 256 bins a workgroup, shortest piece 16
static Layout power_layout(uint32_t W) {
    const uint32_t cols = W < 256 ? W : 256;
    return {cols, cols, 256 / cols, 16};
}
// k_density (qd_density.h, density_geometry): ncol columns from the number of levels, one lane a bin, shortest piece 128
static Layout density_layout(uint32_t W, uint32_t L) {
    uint32_t ncol = 64;
    while (ncol * 2 * L <= 16384 && ncol * 2 <= 256) ncol *= 2;
    const uint32_t cols = W < ncol ? W : ncol;
    return {cols, cols, ncol / cols, 128};
}

// argv: layout (0 pool, 1 power, 2 density) W L n pool bw span_rows n_cu.  The range [0, n) goes in spans of span_rows rows (0: one span),
// each span in batches of bw windows from its start; prints how many (row, slab) are stored whole by one piece, stored whole after a
// meeting of several pieces, and cut (flushed with atomics, by anyone), and the largest number of pieces that met
int main(int argc, char **argv) {
    if (argc != 9) return 2;
    const int kind = std::atoi(argv[1]);
    const uint32_t W = (uint32_t)std::atoll(argv[2]), L = (uint32_t)std::atoll(argv[3]);
    const uint64_t n = std::atoll(argv[4]), pool = std::atoll(argv[5]), bw = std::atoll(argv[6]), span_rows = std::atoll(argv[7]);
    const int n_cu = std::atoi(argv[8]);
    const Layout lay = kind == 0 ? pool_layout(W) : kind == 1 ? power_layout(W) : density_layout(W, L);
    const uint32_t n_slabs = W / lay.cols;
    const uint64_t R = (n - 1) / pool + 1, span = span_rows ? span_rows * pool : n;
    std::vector<uint32_t> alone(R * n_slabs, 0), met(R * n_slabs, 0), cut(R * n_slabs, 0);
    uint32_t most = 0;
    for (uint64_t s0 = 0; s0 < n; s0 += span) {
        const uint64_t s1 = std::min(n, s0 + span);
        for (uint64_t g0 = s0; g0 < s1; g0 += bw) {
            const uint64_t nw = std::min(s1 - g0, bw);
            PieceGeometry G;
            uint64_t grid = 0;
            piece_split(g0, nw, n, pool, W, lay.cols, lay.lanes_per_win, lay.pieces_per_group, lay.min_seg, 4, n_cu, &G, &grid);
            for (uint64_t block = 0; block < grid; ++block)
                for (uint32_t slot = 0; slot < lay.pieces_per_group; ++slot) {
                    const PieceLane l = piece_lane(G, (uint32_t)block, slot);
                    if (!l.active || l.lead != slot) continue;
                    const uint64_t at = l.r * n_slabs + l.slab;
                    if (!l.whole(G)) { cut[at] += 1; continue; }
                    const uint32_t n_same = l.n_same(G);
                    if (n_same > 1) { met[at] += 1; most = std::max(most, n_same); } else alone[at] += 1;
                }
        }
    }
    unsigned long long a = 0, m = 0, c = 0;
    for (uint64_t i = 0; i < R * n_slabs; ++i) {
        if (alone[i] + met[i] + (cut[i] ? 1 : 0) != 1) { std::printf("row %llu ends more than once or never\n", (unsigned long long)i); return 1; }
        a += alone[i]; m += met[i]; c += cut[i] ? 1 : 0;
    }
    std::printf("%llu %llu %llu %u\n", a, m, c, most);
    return 0;
}
"""


@pytest.fixture(scope="module")
def endings(tmp_path_factory):
    """(layout, W, L, n, pool, bw, span_rows) -> (rows stored whole by one piece, stored whole after a meeting, cut, most pieces met)"""
    d = tmp_path_factory.mktemp("endings")
    (d / "endings.cpp").write_text(WALKER)
    exe = d / "endings"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(d / "endings.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(layout, W, L, n, pool, bw, span_rows):
        kind = {"pool": 0, "power": 1, "density": 2}[layout]
        r = subprocess.run([str(exe)] + [str(int(v)) for v in (kind, W, L, n, pool, bw, span_rows, N_CU)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return tuple(int(v) for v in r.stdout.split())
    return run


def device_batch(W, n, pool, chunk_bytes=64 << 20):
    """quadrs_hip.hip, Fold::carrier and walk_limbs: cw = chunk_windows(chunk_bytes / (W 4)), at most the range;
    bw = pool <= cw ? cw / pool * pool : cw"""
    cw = min(chunk_bytes // (W * 4), n)
    return cw // pool * pool if pool <= cw else cw


def limb_rows(W, words, R, chunk_bytes=64 << 20):
    """quadrs_hip.hip, walk_limbs: the accumulator holds max(1, min(2 chunk_bytes / row_bytes, R)) rows of W words u64"""
    return max(1, min(2 * chunk_bytes // (W * words * 8), R))


@pytest.mark.parametrize("W", util.PLANTED_WIDTHS)
def test_row_endings_of_the_limb_folds(endings, W):
    """What test_gpu_planted.py's labels rest on, for k_mean's / k_pool's column layout and k_power's / k_spread's: the default plan from a
    device source is one batch (bw = n), the plan of chunk_bytes = 64 KiB from a host source goes in spans of the accumulator's rows and in
    batches of 8192 / W windows."""
    for depth in util.planted_depths(W):
        n = len(util.planted_case_set(W, depth)) * depth
        R = n // depth
        for layout in ("pool", "power"):
            # walk_limbs uses the accumulator for a batch that cuts rows (spr > 1 here: the batch is the range), and never moves it
            assert depth <= 16 or limb_rows(W, WORDS[layout], R) == R
            bw = device_batch(W, n, depth)
            assert bw == n
            alone, met, cut, most = endings(layout, W, 0, n, depth, bw, 0)
            assert alone + met + cut == R * (W // min(W, 1024 if layout == "pool" else 256))
            if depth <= 16:
                assert alone > 0 and met == 0 and cut == 0, ("whole", layout, W, depth)
            elif depth == 64 and layout == "power" and W == 128:
                # two lane groups a workgroup: four pieces of 16 windows span two of them.  Pieces of 32 windows (a meeting of two) need
                # want / 2 = 1024 rows in the batch, a stream of 64 MiB: past the cap, so this shape is a cut one for k_power and
                # k_spread, and their meetings at depth 64 are the ones at W = 1 and 4
                assert R < 1024 and cut > 0 and alone == 0 and met == 0, ("cut", layout, W, depth)
            elif depth == 64 and W <= 128:
                assert met > 0 and alone == 0 and cut == 0 and most == 4, ("meet", layout, W, depth)
            elif depth == 64 and (W >= 1024 or (layout == "power" and W >= 256)):
                assert cut > 0 and alone == 0 and met == 0, ("cut", layout, W, depth)        # a workgroup holds one piece
            elif depth == 64:
                assert layout == "pool" and W == 256 and met > 0 and cut == 0, ("meet", layout, W, depth)
            elif layout == "power" and W == 4:
                # 16-window pieces make 256 a row; 256 / 4 = 64 lane groups a workgroup: the row spans four of them
                assert depth == 4096 and cut > 0 and alone == 0 and met == 0, ("cut", layout, W, depth)
            else:
                assert depth == 4096 and W <= 4 and met > 0 and most == 256 and alone == 0 and cut == 0, ("meet of 256", layout, W, depth)
            # chunk_bytes = 64 KiB, host source
            small = util.planted_small_batch(W)
            span = limb_rows(W, WORDS[layout], R, util.PLANTED_SMALL_CHUNK)
            alone, met, cut, most = endings(layout, W, 0, n, depth, small, span)
            if depth == 64 and W == 256:
                assert small == 32 and cut > 0 and alone == 0 and met == 0, ("seams inside rows", layout)
            if depth == 4096:
                assert small in (8192, 2048) and cut + met > 0 and alone == 0, ("deep rows", layout, W)
            if depth <= 16 and W <= 256:
                assert small % depth == 0 and alone > 0 and cut == 0, ("whole", layout, W, depth)


def test_all_three_endings_on_both_layouts(endings):
    """over the shapes of the GPU tests, either column layout has rows that are stored whole by one piece, rows stored after a meeting
    and rows that are cut"""
    for layout in ("pool", "power"):
        total = np.zeros(3, dtype=np.int64)
        for W in util.PLANTED_WIDTHS:
            for depth in util.planted_depths(W):
                n = len(util.planted_case_set(W, depth)) * depth
                total += endings(layout, W, 0, n, depth, n, 0)[:3]
        assert (total > 0).all(), (layout, total)


@pytest.mark.parametrize("W", util.PLANTED_WIDTHS)
def test_row_endings_of_the_density_fold(endings, W):
    """k_density's layout at the shapes of the GPU's density tests: the pairs of bucket ends under pool = 2 are rows stored whole from
    one piece; a part of the bucket sweep under pool = n is one row that is met in one workgroup or cut over several"""
    both = np.zeros(2, dtype=np.int64)
    for level0, L in util.PLANTED_GRIDS:
        n = 2 * len(util.density_pair_buckets(level0, L, W))
        assert 10 <= n <= 2 * (L + 4) and n // 2 * W * L * 4 <= max(16 << 20, 8 * W * L * 4)
        alone, met, cut, most = endings("density", W, L, n, 2, n, 0)
        assert alone > 0 and met == 0 and cut == 0, (W, L)
        for part in util.bucket_sweep_parts(W):
            n = part.size
            assert n > 128 and (n + 1) * W * 8 < util.PLANTED_CAP
            alone, met, cut, most = endings("density", W, L, n, n, n, 0)
            assert alone == 0 and met + cut > 0, (W, L)
            both += (met, cut)
    assert both.sum() > 0
    if W == 1:
        assert both[0] > 0                       # 64 lane groups and more a workgroup: the row's pieces meet
    if W >= 256:
        assert both[1] > 0                       # one lane group a workgroup: the row is cut
