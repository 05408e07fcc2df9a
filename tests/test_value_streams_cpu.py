"""The value-domain streams of tests/test_gpu_values.py, held to their conditions on the ORACLE alone (no GPU):
  * code_stream really places every code of cs8 / cu8 / cs16 in I and in Q at every byte offset modulo 16 inside the samples
    that complete windows consume (counted, not left to chance);
  * the sensitivity control: a one-ulp error of the unpacked value of ANY single code in either component changes the result
    of a chain with a lowpass (T = 40, W = 32) and of one without (W = 8).  No code may go unseen: a stream that fails this
    could not see a wrong unpack on the GPU either;
  * scaling a cf32 stream by 2^k scales the reference's output by 2^k bit for bit while nothing leaves the normal range, and
    the scaled norms land where the |X| range switch (qd_device.h norm_fast: x^2 + y^2 outside [2^-96, 2^96)) needs them:
    all small, all large, and both kinds inside one window;
  * zero_runs gives windows that are all +0.0 and windows that mix zero and non-zero samples, and nothing is NaN."""
import numpy as np
import pytest

from test_gpu_parity import _signal, _to_format
from util import (CS16_COMB, bits_equal, code_count, code_coverage, code_stream, contiguous_runs, cs8_grades, mixed_scale, normal_or_zero, perturb_code,
                  slow_bins, source_block, windows_reading, zero_runs)

SR = 21_000_000
LP_CHAIN = ([("lowpass", (2_000_000, 4, 40))], 32, 32)
LP_CHAIN_CS16 = ([("lowpass", (2_000_000, 1, 40))], 32, 32)   # an absorbed error shows per FIR output that reads the sample (util.CS16_COMB): /1 reads each four times as often
NOLP_CHAIN = ([], 8, 8)
# the four chains the scaling relation was first checked on
SCALE_CHAINS = [
    ([("lowpass", (200_000, 32, 200))], 128, 128, 400_000),
    ([("shift", 280000), ("lowpass", (200_000, 32, 400))], 64, 16, 200_000),
    ([], 64, 64, 30_000),
    ([("shift", 280000)], 4, 2, 30_000),
]
N_CODES = {1: 100_000, 2: 100_000, 3: 300_000}


def _chain(oracle, data, fmt, stages):
    ch = oracle.Chain.from_bytes(data, fmt, SR)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch


def _norms(oracle, data, fmt, stages, W, S, **kw):
    return _chain(oracle, data, fmt, stages).spark_fft(W, S, want_codes=False, **kw)[0]


@pytest.fixture(scope="module")
def streams():
    return {fmt: code_stream(fmt, n, 1000 + fmt) for fmt, n in N_CODES.items()}


@pytest.mark.parametrize("fmt", [1, 2, 3])
@pytest.mark.parametrize("chain", [LP_CHAIN, NOLP_CHAIN], ids=["lowpass", "no-lowpass"])
def test_every_code_at_every_load_position(oracle, streams, fmt, chain):
    stages, W, S = chain
    data = streams[fmt]
    n = N_CODES[fmt]
    nw = _norms(oracle, data, fmt, stages, W, S).shape[0]
    lo, hi = source_block(stages, W, S, 0, nw)
    assert lo == 0 and hi <= n
    cov = code_coverage(fmt, data, lo, hi - lo)
    assert cov.shape == (2, 16 // (2 if fmt != 3 else 4), code_count(fmt))
    assert cov.min() >= 1, np.argwhere(cov == 0)[:5]
    if fmt == 1:                                             # graded: a segment holds its grade only and outlasts every window span
        seg = n // 8
        assert seg > 2 * source_block(stages, W, S, 0)[1]
        v = data.view(np.int8).astype(np.int64).reshape(-1, 2)
        for g, gc in enumerate(cs8_grades()):
            assert np.isin(v[g * seg:(g + 1) * seg], gc.view(np.int8)).all()


def _unseen(oracle, fmt, data, chain, codes):
    """the (code, component, sign) whose one-ulp error leaves every window that reads it bit-identical"""
    stages, W, S = chain
    x0 = oracle.unpack(fmt, data)
    ref = _norms(oracle, x0.tobytes(), 0, stages, W, S)
    assert bits_equal(ref, _norms(oracle, data, fmt, stages, W, S))
    unseen = []
    for code in codes:
        for comp in (0, 1):
            for sign in ((1, -1) if (fmt == 1 and code == 0) else (1,)):
                xp, at = perturb_code(fmt, data, x0, code, comp, sign)
                ws = windows_reading(stages, W, S, at, ref.shape[0])
                assert ws, (fmt, code, comp)
                ch = _chain(oracle, xp.tobytes(), 0, stages)
                seen = False
                for first, count in contiguous_runs(ws):
                    for a in range(first, first + count, 64):
                        c = min(64, first + count - a)
                        got = ch.spark_fft(W, S, first_window=a, max_windows=c, want_codes=False)[0]
                        if not bits_equal(got, ref[a:a + c]):
                            seen = True
                            break
                    if seen:
                        break
                if not seen:
                    unseen.append((int(code), comp, sign))
    return unseen


@pytest.mark.parametrize("fmt,codes", [(1, range(256)), (2, range(256)), (3, CS16_COMB)], ids=["cs8", "cu8", "cs16"])
@pytest.mark.parametrize("chain", [LP_CHAIN, NOLP_CHAIN], ids=["lowpass", "no-lowpass"])
def test_no_code_goes_unseen(oracle, streams, fmt, codes, chain):
    assert len(codes) >= 256 and (fmt != 3 or len(codes) >= 512)
    if fmt == 3 and chain is LP_CHAIN:
        chain = LP_CHAIN_CS16
    unseen = _unseen(oracle, fmt, streams[fmt], chain, codes)
    assert not unseen, (len(unseen), unseen[:20])


@pytest.fixture(scope="module")
def base_runs(oracle):
    out = []
    for stages, W, S, n in SCALE_CHAINS:
        x = _signal(np.random.default_rng(n + W), n)
        out.append((x, _norms(oracle, x.tobytes(), 0, stages, W, S, max_windows=400)))
    return out


@pytest.mark.parametrize("i", range(len(SCALE_CHAINS)))
def test_reference_scales_exactly_and_lands_in_the_slow_ranges(oracle, base_runs, i):
    stages, W, S, n = SCALE_CHAINS[i]
    x, base = base_runs[i]
    assert normal_or_zero(x) and normal_or_zero(base) and (base > 0).all()
    k_mixed, both = mixed_scale(base)
    assert both >= 10, (k_mixed, both)
    for k in (-50, -49, -47, 47, 49, 50, 64, k_mixed):
        xs = x * np.float32(2.0 ** k)
        assert normal_or_zero(xs)
        ref = _norms(oracle, xs.tobytes(), 0, stages, W, S, max_windows=400)
        assert normal_or_zero(ref)
        assert bits_equal(ref, base * np.float32(2.0 ** k)), k
        slow, edge = slow_bins(ref)
        if k == -50:
            assert slow.all() and (ref.astype(np.float64) ** 2 < 2.0 ** -96).all()
        if k == 64:
            assert slow.all() and (ref.astype(np.float64) ** 2 >= 2.0 ** 96).all()
        if k == k_mixed:
            fast = ~slow & ~edge
            assert int((slow.any(axis=1) & fast.any(axis=1)).sum()) == both


@pytest.mark.parametrize("i", range(len(SCALE_CHAINS)))
@pytest.mark.parametrize("fmt", [0, 1])
def test_zero_runs_give_zero_windows_and_mixed_windows(oracle, i, fmt):
    stages, W, S, n = SCALE_CHAINS[i]
    span, step = source_block(stages, W, S, 0)[1], source_block(stages, W, S, 1)[0]
    x, zero = zero_runs(_signal(np.random.default_rng(n + W), n), 7 * step + span, span, 5)
    assert normal_or_zero(x)
    for comp in (0, 1):                                      # zeros of both signs in I and in Q
        z = x[:, comp] == 0
        assert (z & np.signbit(x[:, comp])).any() and (z & ~np.signbit(x[:, comp])).any()
    data = np.frombuffer(_to_format(x, fmt), dtype=np.uint8)
    if fmt == 1:
        assert (data.reshape(-1, 2) == 0).any(axis=1)[zero].all()
        zero = (data.reshape(-1, 2) == 0).any(axis=1)
    ref = _norms(oracle, data, fmt, stages, W, S)
    assert not np.isnan(ref).any() and normal_or_zero(ref)
    all_zero = (ref.view(np.uint32) == 0).all(axis=1)        # exactly +0.0
    assert all_zero.sum() >= 5
    csum = np.concatenate([[0], np.cumsum(zero)])
    blocks = np.array([source_block(stages, W, S, w) for w in range(ref.shape[0])])
    nz = csum[blocks[:, 1]] - csum[blocks[:, 0]]
    mixed = (nz > 0) & (nz < blocks[:, 1] - blocks[:, 0])
    assert mixed.sum() >= 5
    # a run that starts and ends inside one window
    edges = np.flatnonzero(np.diff(zero.astype(np.int8)))
    starts, ends = edges[::2] + 1, edges[1::2] + 1
    assert any(((blocks[:, 0] < a) & (b < blocks[:, 1])).any() for a, b in zip(starts, ends))
