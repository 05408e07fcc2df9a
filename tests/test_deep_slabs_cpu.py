"""The conditions the deep-slab GPU tests (tests/test_gpu_deep_slabs.py) rest on, held on the reference alone (no GPU):

  * no ambiguity — util.ambiguous_components is empty over every shift stage's span of every slab, so the byte-for-byte comparison
    needs no NCO-rule excuse.  Shift 280 000 Hz at 21 MHz, which the older deep tests use, repeats its phase every 75 samples: sin(place)
    is a zero crossing once per period — at the head of the stream every period holds an ambiguous component, next to 2^32 93 of 100,
    next to 2^34 37 of 100 (asserted below as the observation it is) — so most windows of 75 samples or more read one; the shifts of util.DEEP_CASES cross zero once in 10.5 million samples;
  * depth — every case has a run with source sample 2^32 strictly inside, one with 2^33, and one that ends with the stream's last
    window; lowpass-free cases of stride 2 have window indices past 2^32;
  * geometry — the source range of every run (and of the run that starts one window later) lies inside its slab, the slab inside the
    stream, window 0 of the slab is window w0 of the stream, and the last run's window count is the slab chain's own;
  * size — runs of 3 tiles + 5 windows (a ragged last tile), at most 64 (a tile + 5 where the tile is 64); slabs below 1 MiB; at most eight plan-time builds;
  * the referee — the planted slab chain equals the window-by-window construction from the oracle's primitives at absolute indices."""
import numpy as np
import pytest

from util import (DEEP_CASES, DEEP_MAX_WINDOWS, DEEP_SLAB_CAP, FMT_BYTES, ambiguous_components, deep_ambiguous, deep_geometry, deep_reference,
                  deep_run_windows, deep_shift_bases, deep_slab_range, shift_ratios)


def test_table_is_bounded():
    names = [c.name for c in DEEP_CASES]
    assert len(set(names)) == len(names)
    assert sum(c.policy == "specialise" for c in DEEP_CASES) <= 8
    assert all(c.policy in ("builtin", "generic", "specialise") for c in DEEP_CASES)
    assert sum(c.paths for c in DEEP_CASES) == 3
    # the eight plan-time builds sit on distinct kernels or sinks: no shape is built twice
    built = [(c.fmt, tuple(map(str, c.stages)), c.W, c.S, c.sink) for c in DEEP_CASES if c.policy == "specialise"]
    assert len(set(built)) == len(built)
    for c in DEEP_CASES:
        assert c.n == deep_run_windows(c.tile) <= max(DEEP_MAX_WINDOWS, c.tile + 5) and (c.tile == 1 or c.n % c.tile), c.name
        assert not any(k == "shift" and abs(a) == 280_000 and c.sr == 21_000_000 for k, a in c.stages), c.name


def test_period_75_shift_is_ambiguous_every_few_periods_at_any_depth(oracle):
    """why the table avoids it: 280 000 / 21 000 000 = 1 / 75, sin(place) crosses zero at every 75th sample, at any depth"""
    ratio = oracle.shift_ratio(280_000, 21_000_000)
    for base in (0, (1 << 32) + 28_672, (1 << 34) - (1 << 20)):
        at = sorted({n for n, _, _ in ambiguous_components(ratio, base, base + 7_500)})
        print(f"shift 280 000 Hz at 21 MHz, samples {base} + 7 500: {len(at)} of 100 periods hold an ambiguous component")
        # at the head of the stream every period; deep in it n * ratio is rounded and a crossing may land a few 1e-9 off zero
        assert (len(at) == 100 if base == 0 else len(at) >= 25) and all(d % 75 == 0 for d in np.diff(at)), (base, len(at))
    assert not ambiguous_components(oracle.shift_ratio(999_983, 21_000_000), (1 << 32) + 28_672, (1 << 32) + 28_672 + 7_500)


@pytest.mark.parametrize("case", DEEP_CASES, ids=lambda c: c.name)
def test_slab_conditions(engine, oracle, case):
    total, complete, raw_step, raw_per_window = deep_geometry(engine, case)
    assert complete == total and raw_step == case.step() and raw_per_window == case.span(1)
    runs = case.runs(total)
    bps = FMT_BYTES[case.fmt]
    for depth, w0, n in runs:
        base, count = deep_slab_range(case, depth, w0, n)
        amb = deep_ambiguous(case, base, count)
        print(f"{case.name} {depth}: windows {w0} + {n}, slab of {count * bps} bytes at sample {base}, ambiguous components {len(amb)}")
        assert not amb, (case.name, depth, amb[:4])
        assert w0 % case.tile == 0 and 2 <= n <= case.n and count * bps < DEEP_SLAB_CAP and base + count <= case.N
        assert all(base % dec == 0 for _, _, dec in deep_shift_bases(case, base))
        # the run, and the run that starts one window inside the tile, read inside the slab
        for a, m in ((w0, n), (w0 + 1, n - 1)):
            first, cnt = a * raw_step, (m - 1) * raw_step + raw_per_window
            assert base <= first and first + cnt <= base + count, (case.name, depth, a, m)
        lo, hi = w0 * raw_step, (w0 + n - 1) * raw_step + raw_per_window
        if depth in ("x32", "x33"):
            mark = 1 << (32 if depth == "x32" else 33)
            assert n == case.n and lo < mark < hi - 1, (case.name, depth, lo, hi)
        else:
            # the stream's last windows: the slab runs to the end of the stream and its own chain counts exactly the run's windows
            assert w0 + n == total and base + count == case.N
            ch = oracle.Chain.from_bytes(bytes(count * bps), case.fmt, case.sr)
            for kind, arg in case.stages:
                ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
            if case.sink == "blocks":
                own = min(b for b in range(n + 2) if case.span(b + 1) > count)
            elif case.sink == "bucket":
                own = (ch.len() - case.W) // case.S
            else:
                own = oracle.lib().qo_spark_window_count(ch.len(), case.W, case.S)
            assert own == n, (case.name, own, n)
            if (len(case.lowpasses) > 1 and case.sink != "bucket") or case.sink == "blocks":      # (freq_levels stops at (len - W) / S: no failing read)
                # a cascade's complete windows and the write sink's full blocks, asked of the ORACLE chain: the run's last window
                # (block) reads exactly, the next one comes back short (or panics: fewer samples than taps)
                stride = case.W if case.sink == "blocks" else case.S
                got, _ = ch.read_at((n - 1) * stride, case.W)
                assert got == case.W, (case.name, got)
                got, _ = ch.read_at(n * stride, case.W)
                assert got != case.W, (case.name, got)
    assert {d for d, _, _ in runs} == {"x32", "x33", "end"}
    if not case.lowpasses and total > 1 << 32:
        assert any(w0 > 1 << 32 for _, w0, _ in runs), case.name       # window indices past 2^32


def test_lowpass_free_stride_2_cases_reach_window_2_to_the_32():
    deep = [c.name for c in DEEP_CASES if not c.lowpasses and c.S == 2]
    assert len(deep) >= 1, deep


@pytest.mark.parametrize("name,depth", [("builtin-pipe3s-cs8", "x33"), ("generic-cs16", "x32"), ("cascade-slsls", "end")])
def test_planted_slab_chain_equals_the_window_by_window_construction(engine, oracle, name, depth):
    """the referee against the oracle's primitives at ABSOLUTE indices: unpack, shift_apply(abs), lowpass_block, ... fft, norm"""
    case = next(c for c in DEEP_CASES if c.name == name)
    total = deep_geometry(engine, case)[0]
    w0, n = next((w, m) for d, w, m in case.runs(total) if d == depth)
    raw, base, ref, _ = deep_reference(oracle, case, depth, w0, n)
    x = oracle.unpack(case.fmt, raw.tobytes())
    ratios = shift_ratios(case.chain)
    W, S = case.W, case.S
    for j in range(n):
        # the block reads of window j, sink to source, then the stages source to sink
        reads = [(j * S, W)]
        for kind, arg in reversed(case.stages):
            if kind == "lowpass":
                off, ln = reads[-1]
                reads.append((off * arg[1], ln * arg[1] + arg[2]))
        off, ln = reads.pop()
        y = x[off:off + ln]
        absolute, k = base + off, 0
        for kind, arg in case.stages:
            if kind == "shift":
                y = oracle.shift_apply(y, absolute, ratios[k])
                k += 1
            else:
                off, ln = reads.pop()
                got, y = oracle.lowpass_block(oracle.taps(arg[0], _rate(case, arg), arg[2]), arg[1], y, out_cap=ln)
                assert got == ln
                absolute //= arg[1]
        row = oracle.norm(oracle.fft(y))[np.r_[W // 2:W, 0:W // 2]]
        assert row.tobytes() == ref[j].tobytes(), (name, depth, j)


def _rate(case, arg):
    """the input rate of lowpass stage `arg` of the case"""
    sr = case.sr
    for k, a in case.stages:
        if k == "lowpass":
            if a is arg:
                return sr
            sr //= a[1]
    raise AssertionError(arg)


@pytest.mark.parametrize("name", ["generic-cs8", "generic-cs16", "specialise-pipe3", "specialise-long-filter-512", "spark-cs8-w128", "spark-cf32-w8",
                                  "cascade-slsls", "write-b64"])
def test_a_32_bit_nco_index_changes_every_window_past_2_to_the_32(engine, oracle, name):
    """The mutation "the NCO's absolute index narrowed to 32 bits", applied to the referee instead of a kernel: a slab chain planted with the
    multipliers of (base_k + i) mod 2^32 is what such a kernel computes.  Its output differs from the referee's in every window that reads
    a source sample past 2^32 and in none before — so the byte-for-byte comparison refuses such a kernel in each of these families."""
    case = next(c for c in DEEP_CASES if c.name == name)
    total, _, raw_step, raw_per_window = deep_geometry(engine, case)
    for depth, w0, n in case.runs(total):
        ref = deep_reference(oracle, case, depth, w0, n)[2]
        cut = deep_reference(oracle, case, depth, w0, n, index_bits=32)[2]
        differs = (np.ascontiguousarray(ref).view(np.uint8).reshape(n, -1) != np.ascontiguousarray(cut).view(np.uint8).reshape(n, -1)).any(axis=1)
        # stage 0 runs at the source rate: window j reads past 2^32 iff its last source sample does
        past = np.array([(w0 + j) * raw_step + raw_per_window > 1 << 32 for j in range(n)])
        before = np.array([(w0 + j) * raw_step + raw_per_window <= 1 << 32 for j in range(n)])
        print(f"{name} {depth}: {int(differs.sum())} of {n} windows differ under a 32-bit index, {int(past.sum())} read past 2^32")
        assert not differs[before].any(), (name, depth)
        assert past.any() and differs[past].all(), (name, depth, differs, past)


def test_ambiguous_windows_counts_by_the_per_window_definition(oracle):
    """util.ambiguous_windows, the figure the older deep tests now record next to their NCO-rule verdict, against the rule's own per-window
    form; on their shift of 280 000 Hz every one of the 24 windows is excusable"""
    from util import ambiguous_windows, shift_spans
    w0 = (1 << 33) // 2048 + 12345
    for desc, ws, want in [(([("shift", 280000), ("lowpass", (2_000_000, 16, 40))], 128, 128, 21_000_000), np.arange(w0, w0 + 24), 24),
                           (([("shift", -1234567)], 64, 1, 21_000_000), np.array([17178820608 + 300 + 250 * i for i in range(24)]), 0),
                           (([("shift", 321334)], 64, 16, 21_000_000), np.arange(190, 230), 4)]:
        slow = sum(any(ambiguous_components(r, lo, hi) for (lo, hi), r in zip(shift_spans(desc, int(w)), shift_ratios(desc))) for w in ws)
        assert ambiguous_windows(desc, ws) == slow == want, (desc, slow)
