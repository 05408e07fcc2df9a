"""qd_gen (k_gen, Gen::read_at of src/gen.rs:35-47) against the oracle (-m gpu), by the rule of util.gen_reference: a sample equals the
reference's bytes unless one of its f64 terms lies within NCO_ABS_ERR of an f32 rounding boundary — the project's bound for a device sincos
(<= 2 ulp) plus glibc's ulp —, and lies between the sums of the low and the high candidates where one does.  tests/test_gen_cpu.py holds
the referee and prints how many samples of each run that excuses.

Runs: blocks of 2^16 samples of cfg4's own tone list and of lists of 1, 2, 3, 64 and 255 tones (negative, zero and repeated frequencies,
tones of 2^40 and 2^62 Hz: the huge-argument reduction of the device sincos) at first = 0, 2^24 - 100, 2^32 - 2^15 (across 2^32), 2^40,
2^53 - 2^15 (across the point past which (double)(first + i) rounds) and 2^63, into host and into device memory; one call of
2^24 + 4097 samples, past the 65536 blocks of 256 lanes the launch is capped at, so k_gen's grid-stride loop takes a second pass; and a
caller's stream."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_parity import record_observed
from util import GEN_BLOCK, GEN_FIRSTS, GEN_LONG, GEN_RUNS, gen_long_stretches, gen_reference, gen_rule_violations, gen_tone_lists

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lists():
    return gen_tone_lists(np.load(os.path.join(GOLDEN, "oracle_vectors.npz"))["gen_tones"])


def _hold(what, refs, got):
    ref, amb, lo, hi = refs
    differ, outside = gen_rule_violations(ref, amb, lo, hi, got)
    exact = int((np.asarray(got).view(np.uint32) == ref.view(np.uint32)).all(axis=1).sum())
    record_observed(what, samples=int(ref.shape[0]), ambiguous=int(amb.sum()), bit_exact=exact, differing_unexcused=int(differ.size),
                    outside_candidates=int(outside.size))
    assert differ.size == 0 and outside.size == 0, (what, differ[:8].tolist(), outside[:8].tolist())


@pytest.mark.parametrize("name,first", GEN_RUNS, ids=[f"{n}@{f}" for n, f in GEN_RUNS])
def test_gen_blocks_equal_the_oracle(engine, oracle, lists, name, first):
    import torch
    tones, sr = lists[name]
    at = GEN_FIRSTS[first]
    refs = gen_reference(oracle, tones, sr, at, GEN_BLOCK)
    host = engine.gen(tones, sr, at, GEN_BLOCK)
    _hold(f"gen {name} at {first}", refs, host)
    dev = torch.full((GEN_BLOCK, 2), float("nan"), dtype=torch.float32, device="cuda")
    engine.gen_device(tones, sr, at, dev)
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == host.tobytes()            # host and device destinations: the same kernel, the same bytes


def test_gen_grid_stride_call(engine, oracle, lists):
    """n = 2^24 + 4097 > 65536 * 256: lanes 0 ... 4096 of the grid generate a second sample each"""
    import torch
    tones, sr = lists[GEN_LONG["tones"]]
    first, n = GEN_LONG["first"], GEN_LONG["n"]
    whole = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda")
    engine.gen_device(tones, sr, first, whole)
    torch.cuda.synchronize()
    stretch = 1 << 14
    for a in gen_long_stretches(n, stretch):
        _hold(f"gen long call, samples {a} + {stretch}", gen_reference(oracle, tones, sr, first + a, stretch), whole[a:a + stretch].cpu().numpy())
    # the whole of it against the same range generated in four pieces, none of which reaches the grid-stride branch
    pieces = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda")
    cuts = [0, n // 4, n // 2, 3 * (n // 4) + 1, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert b - a <= 65536 * 256
        engine.gen_device(tones, sr, first + a, pieces[a:b])
    torch.cuda.synchronize()
    assert torch.equal(whole.view(torch.int32), pieces.view(torch.int32))


def test_gen_on_a_callers_stream(engine, oracle, lists):
    import torch
    L = engine._ffi.lib()
    tones, sr = lists["t64"]
    at = GEN_FIRSTS["2^53-2^15"]
    refs = gen_reference(oracle, tones, sr, at, GEN_BLOCK)
    st = torch.cuda.Stream()
    dev = torch.full((GEN_BLOCK, 2), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    engine._ffi.check(L.qd_set_stream(C.c_void_p(st.cuda_stream)))
    try:
        engine.gen_device(tones, sr, at, dev)
        host = engine.gen(tones, sr, at, GEN_BLOCK)                 # a host destination returns after the copy back
    finally:
        engine._ffi.check(L.qd_set_stream(None))
    st.synchronize()
    _hold("gen t64 at 2^53-2^15 on a caller's stream", refs, host)
    assert dev.cpu().numpy().tobytes() == host.tobytes()
