"""The inputs of test_gpu_bucket_order.py, judged with the oracle alone (no GPU).

QD_EPI_BUCKET2_U8 reduces a window to first < second ? 0 : 1, two sequential f32 sums of |X| over the natural bins 0 ... W/2-1 and
W/2 ... W-1 (src/fft.rs:95-97).  On the tie-balanced real streams of util.balanced_real_stream / balanced_cs8_stream the digit of
every balanced window hinges on the order of those sums and on the tie rule.  This file holds the conditions that make the GPU test
mean something — they are conditions on the INPUTS, computed from oracle norms, never tolerances on a result:

  * util.digits_from_norms(..., "sequential") is freq_levels, on every window of every stream;
  * both digits occur among the balanced windows, and at least one of them is an exact tie (which must read 1);
  * from W = 8 up at least 0.10 of the balanced windows change their digit when the half sums are formed pairwise, and at least
    0.10 when they are formed in f64 (W = 4 and W = 2: a sum of two terms has no order, every balanced window is an exact tie, and
    only the tie rule is pinned);
  * the negative control: util.bucket_digits_ok — the 8-ulp excuse every other bucket check of the suite uses — accepts the
    pairwise digits on these very streams, so none of those checks could tell a pairwise kernel from the reference's order.

A seed that misses a condition is replaced by another seed; the shares are not lowered.
"""
import numpy as np
import pytest

from util import (BUCKET_ORDER_CASES, SUM_ORDERS, _oracle_chain, balanced_cs8_stream, balanced_geometry, bucket_digits_ok,
                  bucket_order_stream, digits_from_norms, exact_ties)

MIN_SHARE = 0.10


def _streams():
    seen, out = set(), []
    for c in BUCKET_ORDER_CASES:
        if c.stream_key() not in seen:
            seen.add(c.stream_key())
            out.append(c)
    return out


STREAMS = _streams()


def _oracle_view(oracle, case):
    """(freq_levels digits, sparkfft norms of the same windows, balanced windows) of the case's own chain"""
    raw, bal = bucket_order_stream(oracle, case)
    ch = _oracle_chain(oracle, raw, case.fmt, case.sr, case.chain_stages())
    levels = ch.freq_levels(case.W, case.S)
    norms, _ = ch.spark_fft(case.W, case.S, max_windows=levels.size, want_codes=False)
    assert norms.shape == (levels.size, case.W) and bal[-1] < levels.size, (norms.shape, levels.size, int(bal[-1]))
    return levels, norms, bal


def test_every_family_of_the_issue_has_a_case():
    """the table names each place that forms the digit; the GPU file asserts the plans come out as them"""
    names = {c.name for c in BUCKET_ORDER_CASES}
    assert len(names) == len(BUCKET_ORDER_CASES)
    assert sum(c.paths for c in BUCKET_ORDER_CASES) == 2
    for c in BUCKET_ORDER_CASES:
        span = balanced_geometry(c.stages, c.W, c.S)[0]
        assert (c.n_balanced == 40 and span > 8192) or (100 <= c.n_balanced <= 300 and span <= 8192), (c.name, span, c.n_balanced)
        assert c.shift in (None, 0)                 # never a shift that turns: the chain stays exact and the stream real


def test_cs8_builder_is_balanced_exactly(oracle):
    x = balanced_cs8_stream(4096, 7)
    assert x.dtype == np.int8 and not x[:, 1].any()
    assert np.array_equal(x[1::4, 0], -x[3::4, 0]) and x[1::4, 0].min() >= -127
    v = oracle.unpack(1, x.tobytes())
    assert not v[:, 1].any() and np.array_equal(v[1::4, 0], -v[3::4, 0])                # code / 127 is odd-symmetric: exact in f32
    assert len(np.unique(x[0::2, 0])) > 200 and len(np.unique(x[1::4, 0])) > 200


def test_balanced_windows_are_balanced(oracle):
    """the builder's claim itself, on a lowpass chain, a cascade and a bare window: the odd outputs of every balanced window sum
    to zero up to the chain's own f32 rounding (the FIR's accumulations are not exactly linear), and the other windows' are
    thousands of times larger"""
    for name in ("cfg3-streaming", "cascade-w16-s8", "spark-w64"):
        case = next(c for c in BUCKET_ORDER_CASES if c.name == name)
        raw, bal = bucket_order_stream(oracle, case)
        ch = _oracle_chain(oracle, raw, case.fmt, case.sr, case.chain_stages())
        levels, norms, _ = _oracle_view(oracle, case)
        odd = np.array([abs(float(ch.read_at(int(w) * case.S, case.W)[1][1::2, 0].astype(np.float64).sum())) for w in range(levels.size)])
        mask = np.zeros(levels.size, dtype=bool)
        mask[bal] = True
        print(f"{name}: worst balanced odd sum {odd[mask].max():.3g}, median elsewhere {np.median(odd[~mask]):.3g}")
        assert np.median(odd[~mask]) > 1000 * odd[mask].max()
        assert not np.frombuffer(raw, dtype=np.float32)[1::2].any()           # imaginary parts exactly zero


def test_a_shift_of_zero_changes_nothing(oracle):
    """the cases that reach a built-in kernel through `shift 0`: the oracle's chain with that stage gives the norms and digits of
    the chain without it, bit for bit (the multiplier is exactly (1, 0))"""
    shifted = [c for c in BUCKET_ORDER_CASES if c.shift is not None]
    assert len(shifted) == 3
    for case in shifted:
        raw, _ = bucket_order_stream(oracle, case)
        a = _oracle_chain(oracle, raw, case.fmt, case.sr, case.chain_stages())
        b = _oracle_chain(oracle, raw, case.fmt, case.sr, [("lowpass", lp) for lp in case.stages])
        assert np.array_equal(a.freq_levels(case.W, case.S), b.freq_levels(case.W, case.S))
        na, nb = a.spark_fft(case.W, case.S, want_codes=False)[0], b.spark_fft(case.W, case.S, want_codes=False)[0]
        assert np.array_equal(na.view(np.uint32), nb.view(np.uint32))


@pytest.mark.parametrize("case", STREAMS, ids=lambda c: c.name)
def test_streams_discriminate_between_summation_orders(oracle, case):
    levels, norms, bal = _oracle_view(oracle, case)
    W = case.W
    # the helper against the oracle, on every window
    assert np.array_equal(digits_from_norms(norms, "sequential"), levels)
    ties = exact_ties(norms)
    shares = {o: float((digits_from_norms(norms, o) != levels)[bal].mean()) for o in SUM_ORDERS[1:]}
    print(f"{case.name}: W={W} S={case.S} windows={levels.size} balanced={bal.size} digit-1 share {levels[bal].mean():.2f} "
          f"exact ties {ties[bal].mean():.2f} " + " ".join(f"{o} {v:.2f}" for o, v in shares.items()))
    # an exact tie reads 1 (`<`), and there is one among the balanced windows
    assert (levels[ties] == 1).all()
    assert (ties[bal] & (levels[bal] == 1)).any()
    # the two sums change places: every window that is no tie inverts, every tie stays
    assert np.array_equal(digits_from_norms(norms, "shifted_halves") != levels, ~ties)
    pair = digits_from_norms(norms, "pairwise")
    if W >= 8:
        assert 0 < levels[bal].sum() < bal.size                         # both digits occur
        assert shares["pairwise"] >= MIN_SHARE and shares["f64"] >= MIN_SHARE, shares
        # outside the balanced windows the halves lie far apart: no order changes a digit there (what today's streams are like)
        rest = np.ones(levels.size, dtype=bool)
        rest[bal] = False
        if case.fmt == 0:
            assert not (pair != levels)[rest].any()
    else:
        assert ties[bal].all()                                          # two terms per half: nothing but the tie rule
    # The negative control.  bucket_digits_ok excuses a digit where the sequential half sums lie within 8 ulp of each other, so a
    # kernel that summed pairwise would pass it on these streams.  Up to W = 256 it accepts EVERY pairwise digit; at W = 1024 the
    # halves of a balanced window drift further apart than 8 ulp in some windows, so there the excused flips are counted instead.
    nat = np.roll(norms, W // 2, axis=1)
    first = np.cumsum(nat[:, : W // 2], axis=1, dtype=np.float32)[:, -1]
    second = np.cumsum(nat[:, W // 2:], axis=1, dtype=np.float32)[:, -1]
    excused = np.abs(first.astype(np.float64) - second) <= 8 * np.spacing(np.maximum(first, second)).astype(np.float64)
    flips = pair != levels
    assert bucket_digits_ok(norms, levels)
    if W <= 256:
        assert bucket_digits_ok(norms, pair)
    if W >= 8:
        print(f"{case.name}: pairwise flips {int(flips.sum())}, of them excused by the 8-ulp rule {int((flips & excused).sum())}")
        assert (flips & excused)[bal].mean() >= MIN_SHARE
