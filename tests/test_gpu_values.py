"""Value-domain tests (-m gpu): the fused kernel families of tests/test_gpu_footprint.py on streams chosen for their VALUES.
The other GPU tests feed one signal (cf32 components of 0.02-0.05, integer codes of a part of the range); here every family gets

  A. every sample code of cs8 / cu8 / cs16, in I and in Q, at every byte offset modulo 16 of the stream (util.code_stream; the
     coverage is counted inside p.src_range of the complete windows).  This is what runs the two-operation unpack of
     qd_device.h (div_small, unpack_cs8_at / unpack_cu8_at / unpack_cs16) through every fused load path for every input;
     tests/test_value_streams_cpu.py shows on the oracle that a one-ulp error on any single code changes such a stream's result.
  B. cf32 streams scaled by 2^k.  The scaling is exact while nothing leaves the normal range, so out(x 2^k) == out(x) 2^k bit
     for bit: for the oracle (asserted on the CPU) and for the engine's own two runs, shifted chains included (the multipliers
     do not depend on the data).  k = -50 and k = 64 send EVERY bin of |X| to the IEEE form (norm_fast's range switch,
     x^2 + y^2 outside [2^-96, 2^96)); a k chosen per case from the reference's norms puts slow and fast bins inside the same
     window, which is what a wrong per-bin select in a four-at-a-time epilogue would get wrong.
  C. runs of exact zeros (util.zero_runs): whole tiles of zeros, runs that start and end inside a window, both signs, in I and
     in Q; cs8 code 0.  A bin with x^2 + y^2 == 0 must take the IEEE form (rsq(0) = inf, 0 * inf = NaN).

Every expectation is the oracle's bytes or a relation the oracle satisfies itself: bit for bit without a shift, the NCO rule
with one (util.footprint_reference states both).  Finite normal-range values and exact zeros only: no NaN, infinity, subnormal
or overflow goes through a fused kernel here, and near-boundary |X| ties stay with test_gpu_parity.py::test_norm_equals_hypotf.
Every case asserts its kernel family like the footprint tests and runs on the device path; each part has one host-path run.

Which integer formats a family can be had at (part A asserts the family for each):
  * k_chain plan-time builds (kernel_policy=2) and the generic DynGeo kernels (kernel_policy=1): all four formats;
  * k_spark2 / k_spark / k_spark0 plan-time builds (kernel_policy=2): all four; the built-in k_spark through kernel_policy=3;
  * k_chain_pipe3s: cs8 is the built-in of the fsk shape, cu8 comes through a tile hint with the cs8 built-in's tiling;
  * k_cascade<fmt> / k_cascade_write<fmt>: run here at cs8, the format the footprint table has them at;
  * two-stage plans: cf32 only here (one cs8 window spans 33 168 samples, more than a graded segment of a 3e5-sample stream)."""
import numpy as np
import pytest

from test_gpu_footprint import FSK, ROW1, ROW2, ROW3, ROW4, ROW5, ROW7, ROW8, Case, _usable_windows, plan_time
from test_gpu_parity import _signal, _to_format, record_observed
from util import (bits_equal, code_coverage, code_stream, footprint_reference, mixed_scale, normal_or_zero, slow_bins, source_block,
                  zero_runs)

pytestmark = pytest.mark.gpu


def _as(case, fmt=None, n=None, name=None, **plan_kw):
    """the case at another sample format / stream length (same chain, same family)"""
    kw = dict(case.plan_kw, **plan_kw)
    fmt = case.fmt if fmt is None else fmt
    return Case(name or f"{case.name}-as-{('cf32', 'cs8', 'cu8', 'cs16')[fmt]}", fmt, case.n if n is None else n, case.W, case.S, case.shift, case.lp,
                case.stages_arg, case.sr, case.epi, case.rng, case.family, case.follows_env, **kw)


PIPE3S_HINT = [14, 512, 1, 8, 4, 2, 1 | (164128 << 8), 0]
PIPE3S_HINT_8BIT = [14, 256, 1, 8, 4, 2, 1 | (164128 << 8), 0]      # the cs8 built-in's tiling: 256 threads
PIPE3S_CF32 = Case("pipe3s-cf32-short", 0, 300_000, family=plan_time("k_chain_pipe3s", 32768 | 131072), follows_env=True, tile_hint=PIPE3S_HINT, **FSK)

# the cf32 families of the table (parts B and C)
CF32_NORMS = ROW1 + [ROW2[4], PIPE3S_CF32, ROW3[0], ROW3[4], ROW3[5], ROW4[0], ROW5[0], ROW5[3], ROW5[4], ROW5[5], ROW7[0], ROW8[0], ROW8[2]]
CF32_WRITE = [ROW4[2], ROW4[3], ROW8[4]]
assert [c.name for c in CF32_WRITE] == ["write-sink-streaming", "write-sink-generic", "cascade-write-LL"] and all(c.fmt == 0 for c in CF32_NORMS)

# part A: the integer cases of the table, and its shapes at the other integer formats where the family can be had
N16 = 300_000                                                # cs16: 4 * 65536 samples hold every code at every offset once
CODE_CASES = (
    [ROW2[2], _as(PIPE3S_CF32, 2, name="pipe3s-cu8-short", tile_hint=PIPE3S_HINT_8BIT)] +
    [ROW3[1], ROW3[2], _as(ROW3[3], n=N16)] +
    [_as(ROW4[0], f, n=N16 if f == 3 else None) for f in (1, 2, 3)] + [_as(ROW4[1], n=N16)] +
    [_as(ROW5[0], f, n=N16 + 384 if f == 3 else None) for f in (1, 2, 3)] +
    [ROW5[1], _as(ROW5[1], 2), _as(ROW5[1], 3, n=N16 + 192)] +
    [_as(ROW5[2], n=N16 + 96)] +
    [_as(ROW5[3], f, n=N16 + 12 if f == 3 else None) for f in (1, 2, 3)] +
    [_as(ROW5[6], n=N16 + 48), ROW5[7]] +
    [ROW8[3], ROW8[7]]
)
ZERO_CS8 = [ROW2[2], ROW5[1], ROW8[3]]
assert [c.name for c in ZERO_CS8] == ["pipe3s-cs8-short", "spark-cs8", "cascade-LL-cs8"]


# ------------------------------------------------------------------ running and comparing

def _run(p, data, nw, path="device"):
    """windows [0, nw) of the stream `data` (bytes / uint8); returns the output as a numpy array"""
    data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1))
    if path == "host":
        return p.run_host(data, 0, nw)
    import torch
    shape, dt = p._out_shape_dtype(nw)
    src = torch.from_numpy(data.copy()).cuda()
    out = torch.full((int(np.prod(shape)) * np.dtype(dt).itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    p.run_device(src, out, 0, nw)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(dt).reshape(shape)


def _hold_to_oracle(case, oracle, p, data, got, nw, what):
    """the chain's rule against the oracle on the same stream (bit for bit without a shift, the NCO rule with one; util.
    footprint_reference); records what was observed.  Returns the oracle's output."""
    ref, rule, _ = footprint_reference(case.oracle_chain(oracle, data), case.stages, case.sr, case.W, case.S, case.epi, case.rng, nw)(0, nw)
    payload = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    ref_b = np.ascontiguousarray(ref).view(np.uint8).reshape(-1)
    assert payload.size == ref_b.size, (case.name, what, payload.size, ref_b.size)
    unit = ref.dtype.itemsize
    differing = int((payload.reshape(-1, unit) != ref_b.reshape(-1, unit)).any(axis=1).sum())
    bad = ([] if differing == 0 else ["differs from the oracle, and the chain has no shift stage"]) if rule is None else rule(payload)
    record_observed(f"values {what} {case.name}", kernel=p.kernel_name(), windows=int(nw), elements=int(ref.size), elements_differing=differing,
                    rule="bit for bit" if rule is None else "NCO rule", complaints=bad[:3])
    assert not bad, (case.name, what, p.kernel_name(), bad)
    return ref


# ------------------------------------------------------------------ A: every code at every load position

def _codes(engine, oracle, case, path="device"):
    p = case.plan(engine)
    nw = _usable_windows(p)
    data = code_stream(case.fmt, case.n, 7 + case.fmt)
    first, count = p.src_range(0, nw)
    cov = code_coverage(case.fmt, data, first, count)
    assert cov.min() >= 1, (case.name, "codes missing inside the consumed samples", np.argwhere(cov == 0)[:5])
    if case.fmt == 1:                                        # a graded segment outlasts the case's window span
        assert case.n // 8 > source_block(case.stages, case.W, case.S, 0)[1], case.name
    _hold_to_oracle(case, oracle, p, data, _run(p, data, nw, path), nw, f"codes[{path}]")
    p.close()


@pytest.mark.parametrize("case", CODE_CASES, ids=repr)
def test_every_sample_code_at_every_load_position(engine, oracle, case):
    _codes(engine, oracle, case)


def test_every_sample_code_host_path(engine, oracle):
    _codes(engine, oracle, ROW3[2], path="host")


# ------------------------------------------------------------------ B: power-of-two scaled cf32 streams

def _x(case):
    return _signal(np.random.default_rng(case.n + case.W), case.n)


def _scaled_run(case, oracle, p, x, k, nw, base_got, path="device"):
    """x 2^k through the plan: held to the oracle on the scaled stream, and to the engine's own run on x, scaled"""
    xs = x * np.float32(2.0 ** k)
    assert normal_or_zero(xs) and (xs != 0).all()
    got = _run(p, xs, nw, path)
    ref = _hold_to_oracle(case, oracle, p, xs.tobytes(), got, nw, f"x 2^{k}" + ("" if path == "device" else f"[{path}]"))
    if ref.dtype == np.float32:
        assert normal_or_zero(ref), (case.name, k)
        assert bits_equal(got, base_got * np.float32(2.0 ** k)), (case.name, k, "the engine's scaled run is not its base run, scaled")
    else:
        assert np.array_equal(got, base_got), (case.name, k, "codes / digits changed under an exact scaling")
    return ref


@pytest.mark.parametrize("case", CF32_NORMS, ids=repr)
def test_scaled_streams_reach_the_ieee_norm_in_every_epilogue(engine, oracle, case):
    if case is ROW7[0]:
        case = case.longer(2)                                # 14 windows: the mixed run needs 10
    p = case.plan(engine)
    nw = _usable_windows(p)
    x = _x(case)
    assert normal_or_zero(x)
    base_got = _run(p, x, nw)
    base = _hold_to_oracle(case, oracle, p, x.tobytes(), base_got, nw, "x")
    assert normal_or_zero(base) and (base > 0).all() and normal_or_zero(base_got)
    k_mixed, both = mixed_scale(base)
    assert both >= 10, (case.name, k_mixed, both)
    # every bin below 2^-48 / at or above 2^48: -50 and 64 unless the case's own norms reach further (one binade of margin)
    k_small = min(-50, int(np.floor(-48 - np.log2(float(base.max())))) - 1)
    k_large = max(64, int(np.ceil(48 - np.log2(float(base.min())))) + 1)
    for k in (k_small, k_large, k_mixed):
        ref = _scaled_run(case, oracle, p, x, k, nw, base_got)
        slow, edge = slow_bins(ref)
        s = ref.astype(np.float64) ** 2
        if k == k_small:
            assert slow.all() and (s < 2.0 ** -96).all(), (case.name, k, float(s.max()))
        elif k == k_large:
            assert slow.all() and (s >= 2.0 ** 96).all(), (case.name, k, float(s.min()))
        else:
            mixed = int((slow.any(axis=1) & (~slow & ~edge).any(axis=1)).sum())
            assert mixed >= 10, (case.name, k, mixed)
            record_observed(f"values mixed {case.name}", k=int(k), windows_with_both=mixed, slow_share=float(slow.mean()))
    p.close()


@pytest.mark.parametrize("case", CF32_WRITE, ids=repr)
def test_scaled_streams_through_the_write_sinks(engine, oracle, case):
    """no |X| behind a write sink: one k, the FIR on scaled data"""
    p = case.plan(engine)
    nw = _usable_windows(p)
    x = _x(case)
    base_got = _run(p, x, nw)
    base = _hold_to_oracle(case, oracle, p, x.tobytes(), base_got, nw, "x")
    assert normal_or_zero(base) and normal_or_zero(base_got)
    _scaled_run(case, oracle, p, x, 50, nw, base_got)
    p.close()


@pytest.mark.parametrize("case,epi", [(ROW1[0], 1), (ROW1[0], 2), (ROW5[4], 1), (ROW8[0], 2)], ids=repr)
def test_scaled_streams_keep_glyph_codes_and_bucket_digits(engine, oracle, case, epi):
    """the range of the glyph sink scaled by the same 2^k: equal codes; the bucket sink: equal digits"""
    x = _x(case)
    norms = case.oracle_chain(oracle, x.tobytes()).spark_fft(case.W, case.S, max_windows=400, want_codes=False)[0]
    k = mixed_scale(norms)[0]
    rng = (np.float32(np.percentile(norms, 20)), np.float32(np.percentile(norms, 99)))
    runs = []
    for kk in (0, k):
        c = case.with_sink(epi, (float(rng[0] * np.float32(2.0 ** kk)), float(rng[1] * np.float32(2.0 ** kk))) if epi == 1 else None)
        p = c.plan(engine)
        nw = _usable_windows(p)
        if kk == 0:
            got = _run(p, x, nw)
            _hold_to_oracle(c, oracle, p, x.tobytes(), got, nw, "x")
            if epi == 1:
                assert len(np.unique(got)) >= 5              # the range really walks the glyph ladder
            runs.append(got)
        else:
            _scaled_run(c, oracle, p, x, kk, nw, runs[0])
        p.close()


def test_scaled_streams_host_path(engine, oracle):
    case = ROW5[5]
    p = case.plan(engine)
    nw = _usable_windows(p)
    x = _x(case)
    base_got = _run(p, x, nw, "host")
    base = _hold_to_oracle(case, oracle, p, x.tobytes(), base_got, nw, "x[host]")
    _scaled_run(case, oracle, p, x, mixed_scale(base)[0], nw, base_got, "host")
    p.close()


# ------------------------------------------------------------------ C: exact zeros

def _zero_case(engine, case):
    """(case, plan, long run, window span): the case lengthened until a run of zeros longer than two tiles AND seven window steps
    fits into its middle third"""
    span, step = source_block(case.stages, case.W, case.S, 0)[1], source_block(case.stages, case.W, case.S, 1)[0]
    for _ in range(2):
        p = case.plan(engine)
        tile_span = (max(int(p.info.tile_windows), 1) - 1) * int(p.info.raw_step) + int(p.info.raw_per_window)
        long_run = max(2 * tile_span, 7 * step) + span
        grow = -(-(long_run + 4 * span) * 8 // (5 * case.n))
        if grow <= 1:
            return case, p, long_run, span
        p.close()
        case = case.longer(grow)
    raise AssertionError((case.name, "the tile grows with the stream"))


def _zeros(engine, oracle, case, path="device"):
    case, p, long_run, span = _zero_case(engine, case)
    nw = _usable_windows(p)
    x, zero = zero_runs(_x(case), long_run, span, 11)
    data = np.frombuffer(_to_format(x, case.fmt), dtype=np.uint8)
    if case.fmt == 1:                                        # the zeros are code 0 (and so is whatever else rounds to it)
        assert (data.reshape(-1, 2) == 0).any(axis=1)[zero].all()
        zero = (data.reshape(-1, 2) == 0).any(axis=1)
    got = _run(p, data, nw, path)
    ref = _hold_to_oracle(case, oracle, p, data, got, nw, f"zeros[{path}]")
    # conditions on the reference alone
    rows = ref.reshape(nw, -1)
    if case.epi == 3:
        all_zero = (rows == 0).all(axis=1)
    else:
        norms = ref if case.epi == 0 else case.oracle_chain(oracle, data).spark_fft(case.W, case.S, max_windows=nw, want_codes=False)[0]
        all_zero = (norms.view(np.uint32) == 0).all(axis=1)  # exactly +0.0
    csum = np.concatenate([[0], np.cumsum(zero)])
    blocks = np.array([source_block(case.stages, case.W, case.S, w) for w in range(nw)])
    nz = csum[blocks[:, 1]] - csum[blocks[:, 0]]
    mixed = (nz > 0) & (nz < blocks[:, 1] - blocks[:, 0])
    assert all_zero.sum() >= 5 and mixed.sum() >= 5, (case.name, int(all_zero.sum()), int(mixed.sum()))
    if ref.dtype == np.float32:
        assert normal_or_zero(ref)
        assert not np.isnan(got).any(), (case.name, "NaN", np.argwhere(np.isnan(got))[:5])
    g = got.reshape(nw, -1)
    if case.epi == 0:
        assert (g[all_zero].view(np.uint32) == 0).all(), (case.name, "an all-zero window is not exactly +0.0")
    elif case.epi == 3:
        assert np.array_equal(g[all_zero].view(np.uint32), rows[all_zero].view(np.uint32))      # signed zeros included
    else:
        assert case.rng[0] > 0 and not g[all_zero].any(), (case.name, "an all-zero window must render as code 0")
    record_observed(f"values zeros {case.name}", windows_all_zero=int(all_zero.sum()), windows_mixed=int(mixed.sum()))
    p.close()


@pytest.mark.parametrize("case", CF32_NORMS + CF32_WRITE + ZERO_CS8 + [ROW1[0].with_sink(1, (0.01, 0.3))], ids=repr)
def test_exact_zero_runs(engine, oracle, case):
    _zeros(engine, oracle, case)


def test_exact_zero_runs_host_path(engine, oracle):
    _zeros(engine, oracle, ROW1[0], path="host")
