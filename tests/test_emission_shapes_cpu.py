"""The designed shapes of util (serpentine, spiral, rings, comb, corners, checker) as the case table that test_gpu_emission_shapes runs on
the device, here with the design's levels as the norms (no transform): the CPU twin (engine.emissions_of) against the flood-fill referee of
test_emissions_cpu byte for byte, what each design states about itself asserted on the referee's list, and the teeth — a flood fill with
one rule broken must change the list of every case that is in the table for that rule.  No GPU."""
import collections

import numpy as np
import pytest

import util
from test_emissions_cpu import EMISSION, ref_emissions, same

F32 = np.float32
FILTERS = ((1, 1), (2, 3))
SMALL_CHUNKS = (1 << 16, 3 << 15)                # chunk_bytes of the two small plans: 8 and 12 windows of 2048 bins a batch
WIDE_CHUNKS = (1 << 17, 1 << 16)                 # ... and at 4096 bins: 8 and 4

# marked: the broken rules (VARIANTS) of which at least one must change the case's list.  A rule that only ADDS joins (a, b) cannot change
# a design that is one emission; it stands in a row for the design's companions in that row.  chunks: (one whose batches hold whole
# tile rows, one whose batches do not).
Case = collections.namedtuple("Case", "name shape args W n marked chunks")
CASES = [
    Case("serpentine0_w2048", "serpentine", (0,), 2048, 72, "bcd", SMALL_CHUNKS),
    Case("serpentine1_w2048", "serpentine", (1,), 2048, 72, "bcd", SMALL_CHUNKS),
    Case("spiral1_w2048", "spiral", (1,), 2048, 64, "acd", SMALL_CHUNKS),
    Case("comb_w2048", "comb", (31,), 2048, 100, "cd", SMALL_CHUNKS),
    Case("corners_w2048", "corners", (8,), 2048, 40, "ac", SMALL_CHUNKS),
    Case("checker_w2048", "checker", (), 2048, 24, "ab", SMALL_CHUNKS),
    Case("serpentine0_w4096", "serpentine", (0,), 4096, 40, "bc", WIDE_CHUNKS),
    Case("corners_w4096", "corners", (8,), 4096, 40, "bc", WIDE_CHUNKS),
    Case("rings_w128", "rings", (), 128, 128, "ac", SMALL_CHUNKS),
    Case("spiral2_w128", "spiral", (2,), 128, 96, "ac", SMALL_CHUNKS),
    Case("serpentine1_w256", "serpentine", (1,), 256, 40, "c", SMALL_CHUNKS),
    Case("serpentine0_w4", "serpentine", (0,), 4, 1100, "c", SMALL_CHUNKS),
    Case("serpentine1_w2", "serpentine", (1,), 2, 2100, "c", SMALL_CHUNKS),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
_DESIGNS = {}


def design(case):
    """(mask bool[n, W], levels f32[n, W]) of a case, made once and read-only"""
    if case.name not in _DESIGNS:
        mask = getattr(util, case.shape)(case.n, case.W, *case.args)
        assert mask.shape == (case.n, case.W) and mask.dtype == bool
        levels = util.shape_levels(mask, sum(case.name.encode()))
        mask.setflags(write=False)
        levels.setflags(write=False)
        _DESIGNS[case.name] = (mask, levels)
    return _DESIGNS[case.name]


def batch_windows(case, chunk, per_window=4, tile_windows=1):
    """the windows a batch of a chunk_bytes = chunk plan holds, as test_gpu_emissions.test_batch_seams_and_sources counts them for a device
    source (4 bytes of norms a bin); a host source's batches are cut by the 8 bytes of a cf32 sample; in whole tiles of the norms kernel"""
    cw = chunk // (case.W * per_window)
    return max(cw // tile_windows * tile_windows, tile_windows)


def seams_inside(mask, cw):
    """the batch seams k cw (between windows k cw - 1 and k cw) across which two on cells are neighbours"""
    return [k for k in range(cw, mask.shape[0], cw) if (mask[k - 1] & mask[k]).any()]


def filtered(ref, min_len, min_cells):
    """the referee's (list, found) under a filter, from its unfiltered list: the filter keeps the order"""
    lst = ref[0]
    keep = (lst["last"] - lst["first"] + 1 >= min_len) & (lst["cells"] >= min_cells)
    return lst[keep], int(keep.sum())


# ------------------------------------------------------------------ the broken flood fills

VARIANTS = {"a": "8 neighbours", "b": "bin W - 1 and bin 0 are neighbours, in a row and from a row to the next",
            "c": "no join across a tile border", "d": "no join across a batch seam of a small plan"}


def broken_fill(mask, variant=None, tr=0, cw=0):
    """[(last, end_bin, first, cells, lo, hi)] in the list's order of a flood fill over `mask` with one rule broken (None: none)"""
    n, W = mask.shape
    on = mask.tolist()
    seen = [[False] * W for _ in range(n)]
    TC = util.EMISSIONS_TILE_COLS
    out = []
    for at in np.flatnonzero(mask).tolist():
        i0, b0 = divmod(at, W)
        if seen[i0][b0]:
            continue
        seen[i0][b0] = True
        stack = [(i0, b0)]
        first, last, cells, lo, hi, end_bin = i0, i0, 0, b0, b0, b0
        while stack:
            i, b = stack.pop()
            cells += 1
            lo, hi = min(lo, b), max(hi, b)
            if i > last:
                last, end_bin = i, b
            elif i == last:
                end_bin = min(end_bin, b)
            near = [(i - 1, b), (i + 1, b), (i, b - 1), (i, b + 1)]
            if variant == "a":
                near += [(i - 1, b - 1), (i - 1, b + 1), (i + 1, b - 1), (i + 1, b + 1)]
            elif variant == "b" and b == W - 1:
                near += [(i, 0), (i + 1, 0)]
            elif variant == "b" and b == 0:
                near += [(i, W - 1), (i - 1, W - 1)]
            for j, c in near:
                if not (0 <= j < n and 0 <= c < W) or not on[j][c] or seen[j][c]:
                    continue
                if variant == "c" and ((j != i and max(i, j) % tr == 0) or (c != b and max(b, c) % TC == 0)):
                    continue
                if variant == "d" and j != i and max(i, j) % cw == 0:
                    continue
                seen[j][c] = True
                stack.append((j, c))
        out.append((last, end_bin, first, cells, lo, hi))
    return sorted(out)


def fields(lst):
    return [tuple(int(r[k]) for k in ("last", "end_bin", "first", "cells", "lo", "hi")) for r in lst]


@pytest.fixture(scope="module")
def referee():
    """name -> the referee's (list, found, components) on the design's levels at threshold 0.5, made once"""
    cache = {}

    def get(name):
        if name not in cache:
            mask, levels = design(BY_NAME[name])
            cache[name] = ref_emissions(levels.view(np.uint32), np.full(mask.shape[1], 0.5, F32))
            on = levels >= 0.5
            assert (on == mask).all() and set(np.unique(levels[mask]).tolist()) == {1.0, 2.0, 3.0}
        return cache[name]
    return get


def test_every_row_of_the_table_is_a_case():
    rows = {(c.shape, c.W, c.n) for c in CASES}
    assert rows == {("serpentine", 2048, 72), ("spiral", 2048, 64), ("comb", 2048, 100), ("corners", 2048, 40), ("checker", 2048, 24),
                    ("serpentine", 4096, 40), ("corners", 4096, 40), ("rings", 128, 128), ("spiral", 128, 96), ("serpentine", 256, 40),
                    ("serpentine", 4, 1100), ("serpentine", 2, 2100)}
    assert {c.args for c in CASES if (c.shape, c.W) == ("serpentine", 2048)} == {(0,), (1,)}
    assert BY_NAME["spiral1_w2048"].args == (1,) and BY_NAME["spiral2_w128"].args == (2,)
    assert [util.emissions_tile_rows(W) for W in (1, 2, 4, 128, 256, 2048, 4096)] == [1024, 1024, 512, 16, 8, 8, 8]
    for c in CASES:                                                         # the batches of the two small plans: whole tile rows, and not
        tr = util.emissions_tile_rows(c.W)
        assert c.chunks[0] >= 1 << 16 and c.chunks[1] >= 1 << 16           # the smallest chunk_bytes a plan takes
        if c.W >= 2048:                                                     # below that, 64 KiB of norms hold the whole design: no seam
            assert batch_windows(c, c.chunks[0]) % tr == 0 and batch_windows(c, c.chunks[1]) % tr != 0
        else:
            assert batch_windows(c, c.chunks[0]) >= c.n - c.n // 4
    assert [batch_windows(BY_NAME["comb_w2048"], ch) for ch in SMALL_CHUNKS] == [8, 12]
    assert [batch_windows(BY_NAME["corners_w4096"], ch) for ch in WIDE_CHUNKS] == [8, 4]


@pytest.mark.parametrize("name", NAMES)
def test_tone_stream_plants_the_design_in_the_oracles_norms(oracle, name):
    """The oracle's transform of util.tone_stream: every on norm is its level and every off norm the transform's rounding — at most 12 f32
    stages on levels up to 3, about 2e-6, so on and off lie 2^16 apart at least — with the trailing window of zeros behind them"""
    case = BY_NAME[name]
    mask, levels = design(case)
    data = util.tone_stream(levels)
    assert len(data) == (case.n + 1) * case.W * 8 and not any(data[-case.W * 8:])
    norms = oracle.Chain.from_bytes(data, 0, util.PLANTED_SR).spark_fft(case.W, None, max_windows=case.n, want_codes=False)[0]
    assert norms.shape == mask.shape
    on_min, off_max = float(norms[mask].min()), float(norms[~mask].max())
    assert on_min >= 65536 * off_max and np.abs(norms[mask] - levels[mask]).max() <= 1e-5
    assert ((norms >= (np.sqrt(on_min * off_max) if off_max else 0.5)) == mask).all()


@pytest.mark.parametrize("name", NAMES)
def test_twin_matches_the_flood_fill_on_the_design(engine, referee, name):
    case = BY_NAME[name]
    mask, levels = design(case)
    ref = referee(name)
    assert int(ref[0]["cells"].sum()) == int(mask.sum()) and ref[1] == ref[2]
    for min_len, min_cells in FILTERS:
        want = ref[:2] if (min_len, min_cells) == (1, 1) else ref_emissions(levels.view(np.uint32), np.full(case.W, 0.5, F32), min_len, min_cells)[:2]
        assert same(filtered(ref, min_len, min_cells), want)               # filtered(), which the GPU file uses: the referee's own filter
        assert same(engine.emissions_of(levels, 0.5, min_len, min_cells, cap=case.n * case.W), want), (min_len, min_cells)


def test_filtering_the_referees_list_is_the_referees_filter(referee):
    """filtered(), which the large streams of the GPU file use, against ref_emissions' own filter where both are cheap and drop something"""
    for name in ("corners_w2048", "rings_w128"):
        mask, levels = design(BY_NAME[name])
        ref = referee(name)
        for min_len, min_cells in ((2, 3), (3, 5), (7, 400)):
            want = ref_emissions(levels.view(np.uint32), np.full(mask.shape[1], 0.5, F32), min_len, min_cells)
            assert same(filtered(ref, min_len, min_cells), want[:2])
        drops = (2, 3) if name == "corners_w2048" else (7, 400)
        assert 0 < filtered(ref, *drops)[1] < ref[1]


@pytest.mark.parametrize("name", [c.name for c in CASES if c.shape == "serpentine"])
def test_serpentine_is_one_emission_over_everything(referee, name):
    case = BY_NAME[name]
    mask, _ = design(case)
    n, W, phase = case.n, case.W, case.args[0]
    tr = util.emissions_tile_rows(W)
    lst, found, comps = referee(name)
    assert found == comps == 1
    full = [i for i in range(n) if mask[i].all()]
    single = [i for i in range(n) if mask[i].sum() == 1]
    assert full == list(range(1 - phase, n, 2)) and single == list(range(phase, n, 2))
    ends = [int(np.flatnonzero(mask[i])[0]) for i in single]
    assert ends == [0 if k % 2 == 0 else W - 1 for k in range(len(single))]      # alternating ends
    # the row above every tile-row border: a full one (phase 0) or a connector (phase 1); there is at least one border
    above = [k * tr - 1 for k in range(1, (n - 1) // tr + 1)]
    assert above and all((i in full) == (phase == 0) for i in above)
    r = lst[0]
    assert (int(r["first"]), int(r["last"]), int(r["lo"]), int(r["hi"]), int(r["flags"])) == (0, n - 1, 0, W - 1, 3)
    assert int(r["cells"]) == len(full) * W + len(single)
    assert int(r["end_bin"]) == (0 if n - 1 in full else ends[-1])


def test_spirals_are_one_arm_one_cell_thick(referee):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, gap in (("spiral1_w2048", 1), ("spiral2_w128", 2)):
        mask, _ = design(BY_NAME[name])
        lst, found, comps = referee(name)
        assert found == comps == 1 and ndimage.label(mask)[1] == 1
        assert not (mask[:-1, :-1] & mask[1:, :-1] & mask[:-1, 1:] & mask[1:, 1:]).any()       # no 2 x 2 block: one cell thick
        assert ndimage.label(~mask)[1] == 1                                                   # the gap is one region: a single arm
        # `gap` off cells between two turns: along the middle window and the middle bin the on cells come at gap + 1, the centre apart
        for line in (mask[mask.shape[0] // 2], mask[:, mask.shape[1] // 2]):
            steps = np.diff(np.flatnonzero(line))
            assert (steps >= gap + 1).all() and (steps == gap + 1).sum() >= steps.size - 1
        r = lst[0]
        assert (int(r["first"]), int(r["last"]), int(r["lo"]), int(r["hi"]), int(r["end_bin"]), int(r["flags"])) == (0, mask.shape[0] - 1, 0, mask.shape[1] - 1, 0, 3)
    big = util.spiral(1436, 2048, 1)                                        # the stream of the GPU file's span test
    assert ndimage.label(big)[1] == 1 and ndimage.label(~big)[1] == 1


def test_rings_end_innermost_first(referee):
    n = W = 128
    lst, found, comps = referee("rings_w128")
    depth = list(range(0, 63, 2))
    assert found == comps == len(depth) == 32
    assert lst["last"].tolist() == sorted(lst["last"].tolist()) == [n - 1 - d for d in reversed(depth)]
    for r, d in zip(lst, reversed(depth)):
        h, w = n - 2 * d, W - 2 * d
        assert (int(r["first"]), int(r["lo"]), int(r["hi"]), int(r["end_bin"]), int(r["cells"])) == (d, d, W - 1 - d, d, 2 * (h + w) - 4)
        assert int(r["flags"]) == (3 if d == 0 else 0)
    # each ring lies around the next
    assert (np.diff(lst["first"].astype(np.int64)) < 0).all() and (np.diff(lst["hi"].astype(np.int64)) > 0).all()


def test_comb_ends_at_its_longest_tooth(referee):
    case = BY_NAME["comb_w2048"]
    n, W = case.n, case.W
    mask, _ = design(case)
    ln = util.comb_lengths(n, W, *case.args)
    lst, found, comps = referee(case.name)
    assert found == comps == 1 and ln.size == W // 2 and ln.min() >= 1 and ln.max() == n - 3 and (ln == ln.max()).sum() == 1
    assert len(set(ln.tolist())) > 20 and not mask[0].any() and mask[1].all() and not mask[:, 1::2][2:].any()
    r = lst[0]
    assert (int(r["first"]), int(r["last"]), int(r["lo"]), int(r["hi"]), int(r["flags"])) == (1, n - 2, 0, W - 1, 0)
    assert int(r["cells"]) == W + int(ln.sum()) and int(r["end_bin"]) == 2 * int(np.argmax(ln)) > 0
    # through a seam it is open as many cells that are no neighbours of each other
    for k in (8, 12, 48):
        assert (mask[k - 1] & mask[k]).sum() > 256 and not (mask[k, :-1] & mask[k, 1:]).any()


@pytest.mark.parametrize("name", ["corners_w2048", "corners_w4096"])
def test_corners_figures(referee, name):
    case = BY_NAME[name]
    mask, _ = design(case)
    figs = util.corner_figures(case.n, case.W, *case.args)
    assert len(figs) == ((case.n - 1) // 8) * (case.W // 256 - 1) and {f for _, _, f, _ in figs} == {0, 1, 2} and {m for _, _, _, m in figs} == {0, 1}
    lst, found, comps = referee(name)
    assert found == comps == sum(2 if f == 0 else 1 for _, _, f, _ in figs)
    assert int(mask.sum()) == sum((2, 3, 4)[f] for _, _, f, _ in figs)
    assert sorted(set(lst["cells"].tolist())) == [1, 3, 4]
    for i, b, f, mirrored in figs:                                          # every figure has a cell in each tile it is meant to touch
        quad = mask[i - 1:i + 1, b - 1:b + 1]
        assert int(quad.sum()) == (2, 3, 4)[f] and (f != 0 or (quad[0, 0] == quad[1, 1] != quad[0, 1] == quad[1, 0]))


def test_checker_is_all_singletons(referee):
    case = BY_NAME["checker_w2048"]
    lst, found, comps = referee(case.name)
    assert found == comps == case.n * case.W // 2 == 24576 and (lst["cells"] == 1).all()
    # a root in every slot (pair of bins) of every row, 1024 to each emit piece of 2048 cells
    assert (lst["lo"] // 2 + (case.W // 2) * lst["last"] == np.arange(found)).all()


@pytest.mark.parametrize("name", NAMES)
def test_teeth_a_broken_rule_changes_the_list(referee, name):
    case = BY_NAME[name]
    mask, _ = design(case)
    tr = util.emissions_tile_rows(case.W)
    whole = broken_fill(mask)
    assert whole == fields(referee(name)[0])                                # the local fill with no rule broken is the referee
    bites = set()
    for v in case.marked:
        cws = [batch_windows(case, ch) for ch in case.chunks] if v == "d" else [0]
        if all(broken_fill(mask, v, tr, cw) != whole for cw in cws):       # d: at the seams of either small plan
            bites.add(v)
    assert bites, "no rule marked for %s changes its list" % name
    # what the design makes certain beyond that: borders and seams cut every design that crosses them, and a rule that adds joins bites
    # wherever two emissions lie that close
    certain = {"serpentine": "cd", "spiral": "cd", "comb": "cd", "corners": "ac", "checker": "ab", "rings": "c"}[case.shape]
    assert set(certain) & set(case.marked) <= bites, (name, bites)
    if "d" in case.marked:
        for ch in case.chunks:
            for per_window in (4, 8):                                       # a device source's batches and a host source's
                assert len(seams_inside(mask, batch_windows(case, ch, per_window))) >= 2
