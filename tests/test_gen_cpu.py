"""The referee of tests/test_gpu_gen.py on the CPU: oracle.gen_terms_f64 (NOT reference behaviour: the f64 terms of src/gen.rs:41 before
the f32 casts) and the rule built on it (util.gen_reference, util.gen_rule_violations).

A generated sample must equal the reference's bytes unless one of its terms is ambiguous, i.e. lies within NCO_ABS_ERR of an f32 rounding
boundary; then it must lie between the sums of the low and of the high candidates.  How many samples that excuses is a property of the
tone list and printed here per run.  Per term the chance is 5.8e-7 (util.GEN_TERM_P, derived there; 17 samples of 65 536 with 255 tones),
so the lists of up to three tones stay below one sample in 10^5 over their six blocks, while 64 tones cannot (7e-5 expected); every block is
held to 3 x its list's expected count + 5 (util.gen_ambiguous_bound).  cfg4's own list is worse for a reason of its own: its tones
are odd multiples of 390 625 Hz = 100 MHz / 256, every tone's sine crosses zero at every 128th sample and its cosine at the 64th between,
so one sample in 64 is ambiguous (the phases are rounded: a crossing is a value of ~1e-9, where the f32 grid is finer than the bound)."""
import os

import numpy as np
import pytest

from util import (GEN_BLOCK, GEN_FIRSTS, GEN_LONG, GEN_RUNS, gen_ambiguous_bound, gen_long_stretches, gen_reference, gen_rule_violations,
                  gen_tone_lists)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lists():
    return gen_tone_lists(np.load(os.path.join(GOLDEN, "oracle_vectors.npz"))["gen_tones"])


def test_the_runs_cover_the_issue(lists):
    assert sorted(len(t) for t, _ in lists.values()) == [1, 2, 3, 64, 64, 255]
    assert {f for _, f in GEN_RUNS} == set(GEN_FIRSTS) and {n for n, _ in GEN_RUNS} == set(lists)
    t64 = lists["t64"][0]
    assert 0 in t64 and min(t64) < 0 and len(set(t64)) < len(t64)                        # zero, negative and repeated frequencies
    assert sorted(abs(t).bit_length() for t in lists["huge"][0])[1:] == [41, 63]          # 2^40 and 2^62 Hz
    first, n = GEN_LONG["first"], GEN_LONG["n"]
    assert n == (1 << 24) + 4097 and n > 65536 * 256 and first < 1 << 32 < first + n
    assert all(0 <= a and a + (1 << 14) <= n for a in gen_long_stretches(n))
    # the blocks cross 2^32 and the point past which (double)(first + i) rounds
    assert GEN_FIRSTS["2^32-2^15"] < 1 << 32 < GEN_FIRSTS["2^32-2^15"] + GEN_BLOCK
    assert GEN_FIRSTS["2^53-2^15"] < 1 << 53 < GEN_FIRSTS["2^53-2^15"] + GEN_BLOCK


@pytest.mark.parametrize("name,first", GEN_RUNS, ids=[f"{n}@{f}" for n, f in GEN_RUNS])
def test_hook_reproduces_the_reference_and_counts_ambiguity(oracle, lists, name, first):
    tones, sr = lists[name]
    ref, amb, lo, hi = gen_reference(oracle, tones, sr, GEN_FIRSTS[first], GEN_BLOCK)
    print(f"gen {name} at {first}: {int(amb.sum())} of {GEN_BLOCK} samples hold an ambiguous term")
    # the hook is the reference's expression: its terms cast to f32 and summed in order from +0 are Gen::read_at, byte for byte
    c, s = oracle.gen_terms_f64(tones, sr, GEN_FIRSTS[first], 4096)
    for comp, v in enumerate((c, s)):
        acc = np.zeros(4096, dtype=np.float32)
        for k in range(len(tones)):
            acc = acc + v[:, k].astype(np.float32)
        assert acc.tobytes() == ref[:4096, comp].tobytes(), (name, first, comp)
    # the candidates bracket the reference, and coincide with it wherever nothing is ambiguous
    assert (lo <= ref).all() and (ref <= hi).all() and (lo[~amb] == ref[~amb]).all() and (hi[~amb] == ref[~amb]).all()
    assert all(v.size == 0 for v in gen_rule_violations(ref, amb, lo, hi, ref))
    # what the list's size (and, for cfg4, its structure) lets expect, with a margin: everything else is held to the reference's bytes
    assert amb.sum() <= gen_ambiguous_bound(name, tones, GEN_BLOCK), (name, first, int(amb.sum()), gen_ambiguous_bound(name, tones, GEN_BLOCK))


def test_short_lists_stay_below_one_ambiguous_sample_in_100000(oracle, lists):
    """the issue's bound, over all six blocks of each list of up to three tones; 64 tones and more cannot meet it (2 K GEN_TERM_P = 7e-5
    per sample at K = 64), nor can cfg4's own list (one sample in 64)"""
    for name in ("one", "two", "huge"):
        tones, sr = lists[name]
        count = sum(int(gen_reference(oracle, tones, sr, at, GEN_BLOCK)[1].sum()) for at in GEN_FIRSTS.values())
        print(f"gen {name}: {count} ambiguous samples in {len(GEN_FIRSTS) * GEN_BLOCK}")
        assert count * 100_000 <= len(GEN_FIRSTS) * GEN_BLOCK, (name, count)


def test_rule_catches_a_32_bit_sample_index(oracle, lists):
    """the mutation (double)(uint32_t)(first + i) of the generator, applied to the reference: a block across 2^32 then continues with
    samples 0, 1, ... — the rule must refuse it, for every list, and must refuse one ulp on one component of one sample"""
    first = GEN_FIRSTS["2^32-2^15"]
    half = GEN_BLOCK // 2
    for name in ("one", "two", "cfg4", "huge"):
        tones, sr = lists[name]
        ref, amb, lo, hi = gen_reference(oracle, tones, sr, first, GEN_BLOCK)
        ch = oracle.Chain.gen(tones, sr, 1.0)
        wrapped = np.concatenate([ch.read_at(first, half)[1], ch.read_at(0, half)[1]])
        differ, outside = gen_rule_violations(ref, amb, lo, hi, wrapped)
        assert differ.size > half // 2 and differ.min() >= half, (name, differ.size)
        one = ref.copy()
        k = int(np.flatnonzero(~amb)[777])
        one[k, 1] = np.nextafter(one[k, 1], np.float32(4))
        differ, outside = gen_rule_violations(ref, amb, lo, hi, one)
        assert differ.tolist() == [k] and outside.size == 0
    # an ambiguous sample is held to its candidates' sums: past them by one ulp is refused
    tones, sr = lists["cfg4"]
    ref, amb, lo, hi = gen_reference(oracle, tones, sr, first, GEN_BLOCK)
    k = int(np.flatnonzero(amb)[5])
    far = ref.copy()
    far[k, 0] = np.nextafter(hi[k, 0], np.float32(1e9))
    differ, outside = gen_rule_violations(ref, amb, lo, hi, far)
    assert differ.size == 0 and outside.tolist() == [k]
