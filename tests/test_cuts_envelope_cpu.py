"""The conditions of the cut list's envelope tests (test_gpu_cuts_envelope.py) on the planning header's text and
the reference alone, without a GPU:
  * the longest tile of all admissible (D, T), where it occurs, and that the planted cut's first tile is one and touches every NCO row
    slot but one;
  * the tables hold what they claim: five counts a shape, shift 0 and at least two others a shape, every reachable pair of 16-byte load
    residues, no ambiguous NCO multiplier component in any shifted span, so the GPU comparison is byte for byte;
  * the value streams show every sample code in both components at every load position inside the cuts' reads, and the per-sample path
    sees the edge codes;
  * a numpy twin of the header's definition equals the oracle byte for byte on every envelope case, and each of its three broken rules
    (no tail truncation, descending taps, a fused multiply-add) changes every case marked for it;
  * at the sensitive samples the first-order multiplier changes the reference of the cut that reads it."""
import numpy as np
import pytest

import cuts_util as U
from test_cuts_cpu import span_of, tile_outputs
from util import CS16_COMB, ambiguous_components, bits_equal, code_coverage, normal_or_zero, stream_codes


def test_header_constants_and_dtype(engine):
    k = U.header_constants()
    assert {"kCutsThreads", "kCutsTileSamples", "kCutsNcoRow", "kCutsTileRows", "kCutsLdsRow", "kCutsBatchTiles"} <= set(k), k
    assert U.CUT_DTYPE == engine.CUT_DTYPE
    assert k["kCutsLdsRow"] == 32 and k["kCutsNcoRow"] == 512                 # what the table's (33, 64) and the planted row residue are chosen against


def test_the_longest_tile_and_its_rows():
    k = U.header_constants()
    threads, samples, row, slots = k["kCutsThreads"], k["kCutsTileSamples"], k["kCutsNcoRow"], k["kCutsTileRows"]
    D = np.arange(1, 1025, dtype=np.int64)[:, None]
    T = np.arange(2, 4097, dtype=np.int64)[None, :]
    outs = np.minimum(threads, (samples - T) // D)
    assert outs.min() >= 1
    span = (outs - 1) * D + T
    longest = int(span.max())
    where = {(int(D[i, 0]), int(T[0, j])) for i, j in np.argwhere(span == longest)}
    assert where == {U.ROW_SHAPE}, (longest, sorted(where))                  # retuned geometry: move ROW_SHAPE (and the table's shape) here
    assert U.ROW_SHAPE in U.ENV_SHAPES and tile_outputs(*U.ROW_SHAPE) == threads and longest <= samples
    # rows a tile of that span touches from residue r of its first read: never more than the slots, and one less than the slots from the
    # planted residue - the most any tile touches
    rows_at = lambda r, n: (r + n - 1) // row + 1      # noqa: E731
    most = max(int(rows_at(r, longest)) for r in range(row))
    assert most == slots - 1
    assert int(((row - 1 + span - 1) // row + 1).max()) <= slots                # any shape at any residue
    cut = U.envelope_cuts()[-1]
    assert (int(cut["decimate"]), int(cut["taps"])) == U.ROW_SHAPE and int(cut["shift_hz"]) != 0
    lo, hi = U.tiles_of(cut)[0]
    assert hi - lo == longest
    reach = {(f * U.ROW_SHAPE[0] + U.ROW_SHAPE[1] - U.ROW_SHAPE[1] // 2) % row for f in range(row)}
    assert lo % row == max(reach) == row - 4 and row - 1 not in reach           # D = 20 and T - T/2 = 2048 are multiples of 4: 508 is the last residue there is
    assert (hi - 1) // row - lo // row + 1 == slots - 1 == rows_at(row - 1, longest)      # the rows residue 511 would touch


def test_the_shapes_reach_their_corners():
    k = U.header_constants()
    t = {s: tile_outputs(*s) for s in U.ENV_SHAPES}
    assert t[(36, 36)] == k["kCutsThreads"] - 1                                 # a tile of 255 lanes
    assert t[(1024, 2)] == 8 and t[(1023, 4096)] == 5 and t[(255, 4096)] == 20  # D >> T; a handful of outputs on a long filter
    assert np.gcd(33, k["kCutsLdsRow"]) == 1
    # (1, 4096): whole tiles in which every output is tail-truncated
    cut = next(c for c in U.envelope_cuts() if (int(c["decimate"]), int(c["taps"])) == (1, 4096) and int(c["count"]) == 2 * t[(1, 4096)] + 3)
    valid = int(cut["count"]) + 4096
    all_cut = [o for o in range(0, int(cut["count"]), t[(1, 4096)]) if o + 2048 + 4096 > valid]
    assert len(all_cut) >= 2
    assert tile_outputs(2, 4094) == k["kCutsThreads"] and (k["kCutsTileSamples"] - 4094) // 2 > k["kCutsThreads"]


def test_envelope_coverage(oracle):
    cuts = U.envelope_cuts()
    for D, T in U.ENV_SHAPES:
        mine = [c for c in cuts[:-1] if (int(c["decimate"]), int(c["taps"])) == (D, T)]
        assert sorted(int(c["count"]) for c in mine) == sorted(U.env_counts(D, T)), (D, T)
        shifts = {int(c["shift_hz"]) for c in mine}
        assert 0 in shifts and len(shifts - {0}) >= 2, (D, T, shifts)
    assert {int(c["shift_hz"]) for c in cuts} == set(U.ENV_SHIFTS)
    assert U.ENV_SHIFTS[5] == U.SR // 2 - 1 == -U.ENV_SHIFTS[6]
    for c in cuts:
        a, b = span_of(c)
        assert b <= U.N_STREAM and int(c["taps"]) % 2 == 0
        if int(c["shift_hz"]):
            assert a >= U.FLOOR and U.clean(oracle, c), c


def test_alignment_coverage(oracle):
    cuts = U.align_cuts()
    for fmt, spv in U.SPV.items():
        for shifted in (False, True):
            mine = [c for c in cuts if bool(int(c["shift_hz"])) == shifted]
            pairs = {(int(c["decimate"]), U.first_read(c) % spv, span_of(c)[1] % spv) for c in mine}
            assert {(1, h, e) for h in range(spv) for e in range(spv)} <= pairs, (fmt, shifted)
            reach4 = {(4, h, e) for h in range(0, spv, 4) for e in range(0, spv, 4)}
            assert reach4 <= pairs, (fmt, shifted, reach4 - pairs)
            ones = {U.first_read(c) % spv for c in mine if int(c["count"]) == 1}
            assert ones == set(range(spv)), (fmt, shifted)
            assert {int(c["decimate"]) for c in mine if span_of(c)[1] == U.N_STREAM} == {1, 4}, (fmt, shifted)
        # the two-sample tiles of the 8-bit formats lie behind every ragged head 0 ... 7: `head > len` wherever it is above 2
        if spv == 8:
            heads = {(-U.first_read(c)) % spv for c in cuts if int(c["count"]) == 1}
            assert heads == set(range(8)) and all(len(U.ragged_samples(c, fmt)) == 2 for c in cuts if int(c["count"]) == 1)
    assert {int(c["decimate"]) for c in cuts if int(c["first"]) == 0 and not int(c["shift_hz"])} == {1, 4}
    for c in cuts:
        a, b = span_of(c)
        assert b <= U.N_STREAM
        if int(c["shift_hz"]):
            assert a >= U.FLOOR and U.clean(oracle, c), c


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_value_cuts_read_every_code_at_every_position(oracle, fmt):
    data, cuts, spv = U.value_stream(fmt), U.value_cuts(fmt), U.SPV[fmt]
    n = data.size // U.FMT_BYTES[fmt]
    codes = stream_codes(fmt, data)
    for shifted in (False, True):
        mine = [c for c in cuts if bool(int(c["shift_hz"])) == shifted]
        read = np.zeros(n, dtype=bool)
        for c in mine:
            for lo, hi in U.tiles_of(c):
                read[lo:hi] = True
        assert read[spv:].all()                                                  # every sample of the code stream itself
        cov = code_coverage(fmt, data, spv, n - spv)
        assert cov.min() >= 1, np.argwhere(cov == 0)[:5]
        if fmt == 3:                                                             # the comb rule (util.CS16_COMB): a one-ulp error on one cs16 sample shows only as a
            tail = (U.VALUE_N[3] - 4 * 65536) // 4 // len(CS16_COMB)             # flipped rounding, so the comb's codes come again and again behind the first pass
            assert tail >= 18 and cov[:, :, CS16_COMB].min() >= 1 + tail, (tail, int(cov[:, :, CS16_COMB].min()))
        assert {U.first_read(c) % spv for c in mine if int(c["count"]) > 1} == set(range(spv))
        ragged = np.array(sorted({s for c in mine for s in U.ragged_samples(c, fmt)}), dtype=np.int64)
        for comp in range(2):
            assert set(U.EDGE_CODES[fmt]) <= set(codes[ragged, comp].tolist()), (fmt, shifted, comp)
        for c in mine:
            if shifted:
                assert U.clean(oracle, c), c


def test_special_streams(oracle):
    data, mask = U.zero_stream()
    x = data.view(np.float32).reshape(-1, 2)
    assert normal_or_zero(x)
    neg = np.signbit(x) & (x == 0)
    quarters = set()
    for c in U.zero_cuts():
        a, b = span_of(c)
        assert mask[a:b].any() and not mask[a:b].all()
        quarters |= {(bool(i), bool(q)) for i, q in neg[a:b][(x[a:b] == 0).all(axis=1)]}
        assert U.clean(oracle, c), c
    assert quarters == {(False, False), (True, False), (False, True), (True, True)}
    y = U.special_stream().view(np.float32).reshape(-1, 2)
    assert int(np.isnan(y).sum()) == 1 and int(np.isinf(y).sum()) == 1 and abs(U.NAN_AT - U.INF_AT) > 20_000
    for c in U.special_cuts():
        hit = U.reaches(c, U.NAN_AT) | U.reaches(c, U.INF_AT)
        assert hit.any() and not hit[:8].any() and not hit[-8:].any()
        assert U.clean(oracle, c), c


# ------------------------------------------------------------------ the twin

def _marked_truncated(c):
    D, T, count = int(c["decimate"]), int(c["taps"]), int(c["count"])
    return (count - 1) * D + (T - T // 2) + T > count * D + T                     # the last output's reach ends past the block


@pytest.mark.parametrize("shape", U.ENV_SHAPES, ids=lambda s: "%dx%d" % s)
def test_twin_equals_the_oracle_and_its_broken_rules_show(oracle, shape):
    cuts = [c for c in U.envelope_cuts() if (int(c["decimate"]), int(c["taps"])) == shape]
    refs = U.oracle_refs(oracle, "env", U.signal_stream(0), 0, U.envelope_cuts())
    refs = [r for r, c in zip(refs, U.envelope_cuts()) if (int(c["decimate"]), int(c["taps"])) == shape]
    assert len(cuts) >= 5
    seen = 0
    for c, ref in zip(cuts, refs):
        x = U.shifted_stream(oracle, int(c["shift_hz"]))
        assert bits_equal(ref, U.twin_cut(oracle, x, c)), c
        if _marked_truncated(c):
            assert not bits_equal(ref, U.twin_cut(oracle, x, c, truncate=False)), ("truncation", c)
            seen += 1
        else:
            assert bits_equal(ref, U.twin_cut(oracle, x, c, truncate=False)), c      # nothing to truncate there: the mark is exact
        if shape[1] >= 40:
            assert not bits_equal(ref, U.twin_cut(oracle, x, c, ascending=False)), ("tap order", c)
            assert not bits_equal(ref, U.twin_cut(oracle, x, c, fused=True)), ("fma", c)
    assert seen == (len(cuts) if shape[1] - shape[1] // 2 > shape[0] else 0)     # every cut of a shape with T - T/2 > D has truncated outputs


# ------------------------------------------------------------------ both NCO orders in one list

@pytest.mark.parametrize("k", range(len(U.SENSITIVE_CASES)))
def test_sensitive_slabs(oracle, k):
    from test_gpu_parity import SENSITIVE
    shift, sr, n, companion = U.SENSITIVE_CASES[k]
    assert n in SENSITIVE[(shift, sr)]
    _, n_samples, base, slab, cuts = U.sensitive_case(k)
    assert slab.size <= 1 << 20 and base % U.SENS_D == 0
    assert ambiguous_components(oracle.shift_ratio(shift, sr), n - U.SENS_HALF, n + U.SENS_HALF) == []
    for c, second in zip(cuts[1:], (False, True)):
        a, b = span_of(c)
        assert base <= a and b <= base + slab.size // 8 and b <= n_samples and a < n < b
        ratio = oracle.shift_ratio(int(c["shift_hz"]), sr)
        assert ambiguous_components(ratio, a, b) == [], c
        assert (abs(ratio) * float(b) > U.SECOND_ORDER_ABOVE) == second, c            # one cut of either order, and a shift-free one, in the same list
    # the first-order multiplier at n changes the sensitive cut's reference: the GPU comparison can fail
    c, s, moved = U.sensitive_mults(oracle, k, shift, first_order_at=n)
    assert moved >= 1
    wrong = U.oracle_cut(oracle, slab, 0, sr, cuts[2], first=int(cuts[2]["first"]) - base // U.SENS_D, mults=(c, s))
    right = U.sensitive_refs(oracle, k)[2]
    assert not bits_equal(right, wrong)
    assert U.reaches(cuts[2], n).sum() >= U.SENS_T // U.SENS_D - 1
    assert ((right.view(np.uint32) != wrong.view(np.uint32)).any(axis=1) <= U.reaches(cuts[2], n)).all()      # and only outputs that read n


def test_many_and_cap_tables(oracle):
    cuts = U.many_cuts()
    assert cuts.size == U.MANY_N
    shifts = set(cuts["shift_hz"].tolist())
    assert len(shifts) == 600 and all(-s in shifts for s in shifts) and {1, -1, U.SR // 2 - 1, 1 - U.SR // 2} <= shifts
    pairs = {(int(c["lowpass_hz"]), int(c["taps"])) for c in cuts}
    assert len(pairs) == 150 and {2, 4096} <= {t for _, t in pairs}
    assert all(U.FLOOR <= span_of(c)[0] and span_of(c)[1] <= U.N_STREAM for c in cuts)
    assert U.many_clean(oracle).sum() >= 0.9 * U.MANY_N                              # almost every span is free of ambiguity: the oracle referees those
    k = U.header_constants()
    ones = U.cap_ones()
    assert ones.size > k["kCutsBatchTiles"] and (ones["count"] == 1).all()
    a, b = span_of(ones[0])[0], span_of(ones[-1])[1]
    assert U.FLOOR <= a and b <= U.N_STREAM and ambiguous_components(oracle.shift_ratio(U.CAP_SHAPE[0], U.SR), a, b) == []
    data, long = U.cap_long()
    tiles = -(-int(long[0]["count"]) // tile_outputs(1, 2))
    assert tiles == k["kCutsBatchTiles"] + 2 and span_of(long[0])[1] <= data.size // 2
