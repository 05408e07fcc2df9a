"""The NCO rule's own machinery, on the CPU (no GPU): nco_candidates against exact arithmetic, the oracle's f64 multipliers and
override hook, the soundness of shift_spans, and unexplained_windows / replay_window on flips made through the hook."""
import math
from fractions import Fraction

import numpy as np
import pytest

from util import (NCO_ABS_ERR, ambiguous_components, nco_candidates, replay_window, shift_ratios, shift_spans,
                  unexplained_windows)


def _f32_exact(x):
    """round-to-nearest-even of the rational x to f32, by exact comparison with the f32 neighbours"""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    best = None
    for c in cands:
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - x)
        if best is None or d < best[0] or (d == best[0] and int(np.float32(c).view(np.int32)) % 2 == 0):
            best = (d, c)
    return best[1]


def _brute(v):
    e = Fraction(NCO_ABS_ERR)
    return _f32_exact(Fraction(float(v)) - e), _f32_exact(Fraction(float(v)) + e)


def _check_candidates(vals):
    vals = np.asarray(vals, dtype=np.float64)
    lo, hi = nco_candidates(vals)
    for v, a, b in zip(vals, lo, hi):
        wa, wb = _brute(v)
        assert a.view(np.uint32) == np.float32(wa).view(np.uint32) and b.view(np.uint32) == np.float32(wb).view(np.uint32), \
            (repr(v), a, b, wa, wb)


def test_candidates_at_midpoints():
    rng = np.random.default_rng(1)
    f = np.concatenate([rng.uniform(-1, 1, 60).astype(np.float32), np.float32([0.5, -0.5, 1.0, -1.0, 2.0 ** -20, 0.7071068])])
    up = np.nextafter(f, np.float32(np.inf))
    mids = (f.astype(np.float64) + up.astype(np.float64)) / 2
    vals = []
    for m in mids:
        u = np.spacing(m)
        k = np.arange(-40, 41)
        vals += list(m + k * u)
        # the midpoints the interval's own ends fall on: v = mid +- eps, +- 1 f64 ulp
        for s in (-1, 1):
            c = m + s * NCO_ABS_ERR
            vals += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    _check_candidates(vals)
    lo, hi = nco_candidates(mids)
    assert (lo != hi).all()                                 # a midpoint is always ambiguous


def test_candidates_at_one_zero_and_subnormal():
    specials = [1.0, -1.0, 0.0, -0.0, 1e-45, -1e-45, 1.4e-45, 1e-39, -1e-39, 5e-324, 1e-300, 2e-15, -2e-15, 1 - 1e-16, -1 + 1e-16]
    _check_candidates(specials)
    lo, hi = nco_candidates(np.array([1.0, -1.0, 0.0, -0.0]))
    assert lo[0] == hi[0] == 1 and lo[1] == hi[1] == -1     # +-1 are never ambiguous
    assert lo[2] < 0 < hi[2] and lo[3] < 0 < hi[3]          # a zero crossing holds many values


def test_candidates_random():
    rng = np.random.default_rng(2)
    vals = np.concatenate([np.cos(rng.uniform(0, 2 * np.pi, 60_000)), rng.uniform(-1, 1, 30_000),
                           rng.uniform(-1, 1, 10_000) * 10.0 ** rng.integers(-12, 0, 10_000)])
    lo, hi = nco_candidates(vals)
    # the rule itself: the f32 of v is a candidate, every candidate is within eps of some x that rounds to it
    f = vals.astype(np.float32)
    assert ((lo <= f) & (f <= hi)).all()
    # exact comparison for every ambiguous value and a sample of the rest
    amb = np.nonzero(lo != hi)[0]
    pick = np.concatenate([amb, rng.choice(vals.size, 3000, replace=False)])
    _check_candidates(vals[pick])
    # elsewhere lo == hi == f32(v) and both ends of the interval round to it: vectorised exact check in f64 pairs
    one = lo == hi
    assert (lo[one] == f[one]).all()


def test_f64_multipliers_round_to_the_reference(oracle):
    rng = np.random.default_rng(3)
    one = np.zeros((1, 2), np.float32)
    one[0, 0] = 1
    total = 0
    for freq, sr in ((280000, 21_000_000), (-10_499_999, 21_000_000), (3, 400), (49_999_999, 100_000_000)):
        ratio = oracle.shift_ratio(freq, sr)
        for n0 in (0, 2**28 - 50_000, 2**34 + 12_345, 2**35 + 7):
            n = 125_000
            c, s = oracle.shift_multipliers_f64(ratio, n0, n)
            ref = oracle.shift_apply(np.repeat(one, n, axis=0), n0, ratio)            # 1 + 0i: the multiplier itself ...
            zero = (ref == 0).any(axis=1)                                           # ... up to the sign of a zero
            ref[zero] = oracle.shift_multipliers(ratio, n0 + np.nonzero(zero)[0])
            assert bits_equal_pair(c.astype(np.float32), ref[:, 0]) and bits_equal_pair(s.astype(np.float32), ref[:, 1])
            total += n
            for i in rng.integers(0, n, 20):
                m = oracle.shift_multipliers(ratio, [n0 + int(i)])[0]
                assert np.float32(c[i]) == m[0] and np.float32(s[i]) == m[1]
    assert total >= 1_000_000


def bits_equal_pair(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_shift_ratios_equal_the_oracle(oracle):
    stages = [("shift", 1234), ("lowpass", (100_000, 7, 40)), ("shift", -98_765), ("lowpass", (10_000, 3, 10)), ("shift", 77)]
    ch = oracle.Chain.gen([1000], 3_000_000, 0.01)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    assert shift_ratios((stages, 16, 16, 3_000_000)) == ch.shift_ratios


def test_override_hook(oracle):
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((3000, 2)) * 0.1).astype(np.float32)
    ch = oracle.Chain.from_bytes(x.tobytes(), oracle.FMT_CF32, 1000).shift(123)
    _, base = ch.read_at(0, 3000)
    ch.override_shift(0, [5, 2999, 17], [0.5, 0.25, 1.0], [0.0, 0.0, 0.0])
    _, got = ch.read_at(0, 3000)
    _, part = ch.read_at(10, 20)                           # reads that start inside the overridden range
    ch.override_shift(0, [], [], [])
    _, back = ch.read_at(0, 3000)
    assert bits_equal_pair(back, base)
    ne = np.nonzero((got != base).any(axis=1))[0]
    assert set(ne) <= {5, 17, 2999}
    assert (got[5] == x[5] * np.float32(0.5)).all() and (got[2999] == x[2999] * np.float32(0.25)).all() and (got[17] == x[17]).all()
    assert bits_equal_pair(part, got[10:30])
    with pytest.raises(ValueError):
        ch.override_shift(0, [3, 3], [1, 1], [0, 0])


# ------------------------------------------------------------------ span soundness

def _draw_shape(rng, kind):
    if kind == "single":
        D, T = int(rng.choice([1, 2, 3, 4, 8, 16])), int(rng.choice([2, 5, 8, 16, 40]))
        W = 1 << int(rng.integers(0, 6))
        S = int(rng.choice([W, max(1, W // 2), int(rng.integers(1, 2 * W + 1))]))
        return [("shift", int(rng.integers(-400, 400))), ("lowpass", (200, D, T))], W, S
    if kind == "nofir":
        W = 1 << int(rng.integers(0, 6))
        S = int(rng.choice([max(1, W // 4), max(1, W // 2), int(rng.integers(1, W + 1))]))
        return [("shift", int(rng.integers(-400, 400)))], W, S
    # cascade [S] L [S] [L [S]]
    l2 = rng.random() < 0.6
    s0, s1 = rng.random() < 0.5, rng.random() < 0.5 or not l2
    s2 = l2 and (rng.random() < 0.5 or not (s0 or s1))
    st = []
    if s0:
        st.append(("shift", int(rng.integers(-400, 400))))
    st.append(("lowpass", (150, int(rng.choice([1, 2, 3, 4])), int(rng.choice([2, 5, 8, 12])))))
    if s1:
        st.append(("shift", int(rng.integers(-50, 50))))
    if l2:
        st.append(("lowpass", (40, int(rng.choice([1, 2, 3])), int(rng.choice([2, 4, 7])))))
        if s2:
            st.append(("shift", int(rng.integers(-10, 10))))
    W = 1 << int(rng.integers(0, 4))
    return st, W, int(rng.choice([W, max(1, W // 2), int(rng.integers(1, 2 * W + 1))]))


def test_shift_spans_are_sound(oracle):
    """Flip one multiplier to its f32 neighbour through the hook: the windows that change are among those whose span holds the
    index, and the spans are at most one FIR length (per stage below, at the flipped stage's rate) wider than needed."""
    rng = np.random.default_rng(5)
    sr = 1000
    n_shapes = changed_any = changed_ulp = tight = 0
    for i in range(240):
        kind = ("single", "nofir", "cascade")[i % 3]
        stages, W, S = _draw_shape(rng, kind)
        N = int(rng.integers(600, 1500))
        x = (rng.standard_normal((N, 2)) * 0.1).astype(np.float32)
        ch = oracle.Chain.from_bytes(x.tobytes(), oracle.FMT_CF32, sr)
        for k, a in stages:
            ch = ch.shift(a) if k == "shift" else ch.lowpass(*a)
        try:
            ref, _ = ch.spark_fft(W, S, want_codes=False)
        except RuntimeError:
            continue
        if ref.shape[0] == 0:
            continue
        nw = ref.shape[0]
        shifts = [j for j, (k, _) in enumerate(stages) if k == "shift"]
        pick = int(rng.integers(0, len(shifts)))
        # the flipped stage's stream length and its index range the windows read
        rate_len = N
        for k, a in stages[:shifts[pick]]:
            rate_len = 1 + (rate_len - a[2]) // a[1] if k == "lowpass" else rate_len
        spans = shift_spans((stages, W, S, sr), np.arange(nw))[pick]
        n = int(rng.integers(int(spans[0].min()), min(int(spans[1].max()), rate_len)))
        ratio = ch.shift_ratios[pick]
        c, s = oracle.shift_multipliers_f64(ratio, n, 1)
        m = [np.float32(c[0]), np.float32(s[0])]
        comp = int(rng.integers(0, 2))
        m[comp] = np.nextafter(m[comp], np.float32(np.inf if rng.random() < 0.5 else -np.inf))
        changed = {}
        for how, mult in (("ulp", m), ("big", [np.float32(4), np.float32(3)])):      # the f32 neighbour; a value far off
            ch.override_shift(pick, [n], [mult[0]], [mult[1]])
            got, _ = ch.spark_fft(W, S, want_codes=False)
            ch.override_shift(pick, [], [], [])
            changed[how] = set(int(w) for w in np.nonzero(((ref != got) & ~(np.isnan(ref) & np.isnan(got))).any(axis=1))[0])
        predicted = set(int(w) for w in np.nonzero((spans[0] <= n) & (n < spans[1]))[0])
        assert changed["ulp"] <= predicted and changed["big"] <= predicted, (stages, W, S, n, changed, predicted)
        changed_ulp += bool(changed["ulp"])
        changed_any += bool(changed["big"])
        # tightness: within one FIR length (of the stages below, at this stage's rate) of either end of a window's span there is
        # a sample the window reads, i.e. one whose multiplier set to 4 + 3i changes the window
        fir, mult = 0, 1
        for k, a in stages[shifts[pick] + 1:]:
            if k == "lowpass":
                fir += a[2] * mult
                mult *= a[1]
        w = int(rng.integers(0, nw))
        lo, hi = int(spans[0][w]), min(int(spans[1][w]), rate_len)
        if not np.isnan(ref[w]).any():
            for probe in (range(lo, min(hi, lo + fir + 1)), range(hi - 1, max(lo, hi - 1 - fir) - 1, -1)):
                for idx in probe:
                    ch.override_shift(pick, [idx], [4.0], [3.0])
                    one, _ = ch.spark_fft(W, S, first_window=w, max_windows=1, want_codes=False)
                    ch.override_shift(pick, [], [], [])
                    if not bits_equal_pair(one, ref[w:w + 1]):
                        break
                else:
                    raise AssertionError(("span wider than one FIR length", stages, W, S, w, lo, hi, fir))
                tight += 1
        n_shapes += 1
    assert n_shapes >= 200 and changed_any >= 0.6 * n_shapes and changed_ulp >= 50 and tight >= n_shapes, (n_shapes, changed_any, changed_ulp, tight)


def _exhaustive_shapes(rng):
    """two-lowpass cascades where the second FIR is shorter than two decimations (c2 < D2) and the first is longer than two
    (c1 > D1) -- a span capped by the dependency end instead of the block end falls short there -- plus a seeded draw of every
    kind"""
    fixed = [([("shift", 100), ("lowpass", (150, 1, 12)), ("lowpass", (40, 3, 2))], 4, 4),
             ([("shift", 100), ("lowpass", (150, 1, 40)), ("lowpass", (40, 4, 2))], 4, 4),
             ([("shift", -77), ("lowpass", (150, 2, 16)), ("shift", 9), ("lowpass", (40, 5, 4)), ("shift", 3)], 2, 1),
             ([("lowpass", (150, 1, 10)), ("shift", 31), ("lowpass", (40, 6, 2)), ("shift", -5)], 4, 8)]
    drawn = []
    for i in range(45):
        if i % 3 == 2:
            D1, D2 = int(rng.choice([1, 2])), int(rng.choice([3, 4, 6]))
            T1, T2 = int(rng.choice([8, 12, 16, 40])), int(rng.choice([2, 4]))
            st = [("shift", int(rng.integers(-400, 400))), ("lowpass", (150, D1, T1))]
            if rng.random() < 0.5:
                st.append(("shift", int(rng.integers(-50, 50))))
            st.append(("lowpass", (40, D2, T2)))
            if rng.random() < 0.5:
                st.append(("shift", int(rng.integers(-10, 10))))
            W = 1 << int(rng.integers(0, 3))
            drawn.append((st, W, int(rng.choice([W, max(1, W // 2), 2 * W]))))
        else:
            drawn.append(_draw_shape(rng, ("single", "cascade")[i % 3]))
    return fixed + drawn


def test_shift_spans_hold_every_index_a_window_reads(oracle):
    """Deterministic: for a window of each shape and each of its shift stages, set the multiplier of EVERY index in
    [lo - margin, hi + margin) to 4 + 3i in turn; each index that changes the window lies in its span [lo, hi), and within one
    FIR length (of the stages below, at that stage's rate) of either end of the span there is one that does."""
    rng = np.random.default_rng(8)
    sr = 1000
    probed = 0
    for stages, W, S in _exhaustive_shapes(rng):
        N = 900
        x = (np.random.default_rng(len(stages) + W).standard_normal((N, 2)) * 0.1).astype(np.float32)
        ch = oracle.Chain.from_bytes(x.tobytes(), oracle.FMT_CF32, sr)
        for k, a in stages:
            ch = ch.shift(a) if k == "shift" else ch.lowpass(*a)
        try:
            ref, _ = ch.spark_fft(W, S, want_codes=False)
        except RuntimeError:
            continue
        nw = ref.shape[0]
        if nw == 0:
            continue
        shifts = [j for j, (k, _) in enumerate(stages) if k == "shift"]
        for w in sorted({nw // 2, nw - 1}):
            if np.isnan(ref[w]).any():
                continue
            spans = shift_spans((stages, W, S, sr), w)
            for pick, (lo, hi) in enumerate(spans):
                rate_len = N
                for k, a in stages[:shifts[pick]]:
                    rate_len = 1 + (rate_len - a[2]) // a[1] if k == "lowpass" else rate_len
                fir, mult = 0, 1
                for k, a in stages[shifts[pick] + 1:]:
                    if k == "lowpass":
                        fir += a[2] * mult
                        mult *= a[1]
                margin = fir + S * mult
                reads = []
                for idx in range(max(0, lo - margin), min(rate_len, hi + margin)):
                    ch.override_shift(pick, [idx], [4.0], [3.0])
                    one, _ = ch.spark_fft(W, S, first_window=w, max_windows=1, want_codes=False)
                    ch.override_shift(pick, [], [], [])
                    if not bits_equal_pair(one, ref[w:w + 1]):
                        reads.append(idx)
                outside = [i for i in reads if not lo <= i < hi]
                assert not outside, ("span rounds inward", stages, W, S, w, pick, (lo, hi), outside)
                if reads:
                    assert reads[0] - lo <= fir and min(hi, rate_len) - 1 - reads[-1] <= fir, \
                        ("span wider than one FIR length", stages, W, S, w, pick, (lo, hi), reads[0], reads[-1], fir)
                    probed += 1
    assert probed >= 60, probed


# ------------------------------------------------------------------ the check and the replay on flips made through the hook

def _find_ambiguous(ratio, lo, hi):
    amb = ambiguous_components(ratio, lo, hi)
    return [a for a in amb if a[2] is not None and len(a[2]) == 2]


def _blocks(ch, w0, cnt, B):
    return np.stack([ch.read_at((w0 + i) * B, B)[1].reshape(-1) for i in range(cnt)])


def test_check_accepts_ambiguous_flips_and_rejects_others(oracle):
    """Windows here are blocks of B shifted samples of 1 + 0i (the write sink without a lowpass): a flipped multiplier always
    shows.  An ambiguous flip is explained and replays to exactly that flip; a flip of a non-ambiguous component is not."""
    sr, freq = 21_000_000, 1_234_567
    ratio = oracle.shift_ratio(freq, sr)
    amb = _find_ambiguous(ratio, 0, 3_000_000)
    assert amb, "no ambiguous component in the first 3 M samples"
    n_a, comp, cand = amb[0]
    B, cnt = 4, 5
    desc = ([("shift", freq)], B, B, sr)
    N = n_a + 4 * B * cnt
    x = np.zeros((N, 2), np.float32)
    x[:, 0] = 1
    ch = oracle.Chain.from_bytes(x.tobytes(), oracle.FMT_CF32, sr).shift(freq)
    w0 = n_a // B - 2
    ref = _blocks(ch, w0, cnt, B)
    c, s = oracle.shift_multipliers_f64(ratio, n_a, 1)
    default = [np.float32(c[0]), np.float32(s[0])]
    other = [v for v in cand if v != default[comp]][0]
    flipped = list(default)
    flipped[comp] = other
    ch.override_shift(0, [n_a], [flipped[0]], [flipped[1]])
    got = _blocks(ch, w0, cnt, B)
    ch.override_shift(0, [], [], [])
    diff_rows = np.nonzero((ref != got).any(axis=1))[0]
    assert diff_rows.tolist() == [2]
    detail = {}
    assert unexplained_windows(ref, got, lambda w: shift_spans(desc, w), shift_ratios(desc), w0, detail) == []
    w = w0 + 2
    combo = replay_window(ch, w, detail[w], got[2], B, sink="blocks")
    assert combo is not None
    assert [(k, n, cp, v) for k, n, cp, v in combo if v != default[cp] or n != n_a] == [(0, n_a, comp, float(other))], combo
    assert bits_equal_pair(_blocks(ch, w0, cnt, B), ref)                     # replay leaves no override behind
    # a non-ambiguous component flipped to its f32 neighbour: reported, in its own window only
    n_b = n_a + B
    assert not ambiguous_components(ratio, n_b, n_b + 1)
    c, s = oracle.shift_multipliers_f64(ratio, n_b, 1)
    ch.override_shift(0, [n_b], [np.float32(c[0])], [np.nextafter(np.float32(s[0]), np.float32(2))])
    got2 = _blocks(ch, w0, cnt, B)
    ch.override_shift(0, [], [], [])
    assert unexplained_windows(ref, got2, lambda w: shift_spans(desc, w), shift_ratios(desc), w0) == [w0 + 3]
    # both flips at once: the first window explained, the second not
    assert unexplained_windows(ref, np.where(np.arange(cnt)[:, None] == 2, got, got2), lambda w: shift_spans(desc, w),
                               shift_ratios(desc), w0) == [w0 + 3]


def test_ratio_matches_tau_formula(oracle):
    for f, sr in ((280000, 21_000_000), (-3, 400), (49_999_999, 100_000_000)):
        assert oracle.shift_ratio(f, sr) == math.tau * f / sr
