"""The bucket sink's half-sum order (-m gpu): QD_EPI_BUCKET2_U8 against the oracle's freq_levels on tie-balanced real streams.

The digit is first < second ? 0 : 1 with two SEQUENTIAL f32 sums of |X| over the natural bins 0 ... W/2-1 and W/2 ... W-1
(src/fft.rs:95-97).  Every other bucket check of the suite excuses a differing digit where the two sums lie within a few ulp of
each other, and runs on streams whose halves lie percents apart: a kernel that summed pairwise, in f64, back to front or with the
halves exchanged at a tie would pass them all.  Here the streams are real-valued with balanced windows (util.balanced_real_stream,
util.balanced_cs8_stream): |X[k]| = |X[W-k]| and X[0] ~ X[W/2], so `second` is `first`'s multiset summed the other way round, and
only the order of the sums and the tie rule decide the digit.  tests/test_bucket_order_cpu.py shows with the oracle alone that on
these very streams 0.18 ... 0.62 of the balanced windows change their digit under another order, and that exact ties occur.

There is no shift stage that turns, so the chain is exact (unpack, FIR, Radix4, hypot) and the engine must equal the oracle on
EVERY window: np.array_equal, no excuse list, no ulp margin.  Expected digits come from the oracle only.

One case per place that forms the digit (util.BUCKET_ORDER_CASES), each asserted to run on its intended kernel:
wave_bucket_epilogue_fn (deferred FFT, three-stage, built-in wave-local and k_spark2 kernels), phase 4 of k_chain (generic, built-in
and plan-time geometry), the streaming three-stage kernel's swizzled epilogue, the lean path of the plan-time k_spark, the register
path of k_spark0, lane 0 of k_cascade, and the two-stage plan's second stage.  Plans are created with explicit options, so the
cases do not follow the QD_* names of the test matrix.  The built-in kernels of cfg2, cfg3' and the 64 / 16 FSK chain exist only
with a shift stage; `shift 0` (a multiplier of exactly (1, 0)) reaches them and leaves the stream real and the chain exact.  The
interleaved launches of overlapping lowpass-free windows serve the norms and glyph sinks only: W = 64 / S = 16 is pinned on the
kernels the bucket sink really runs there.
"""
import numpy as np
import pytest

from util import BUCKET_ORDER_CASES, FMT_BYTES, _oracle_chain, bucket_order_stream

pytestmark = pytest.mark.gpu


def _plan(engine, case, n, **opt_kw):
    policy = {"auto": engine.KERNEL_AUTO, "generic": engine.KERNEL_GENERIC, "specialise": engine.KERNEL_SPECIALISE,
              "builtin": engine.KERNEL_NO_PLAN_TIME}[case.policy]
    opts = engine.plan_options(kernel_policy=policy, tile_hint=case.tile_hint, **opt_kw)
    kw = dict(width=case.W, stride=case.S, epilogue=engine.EPI_BUCKET2_U8, options=opts)
    if len(case.stages) > 1:
        assert case.shift is None
        kw["stages"] = [("lowpass", lp) for lp in case.stages]
    else:
        kw.update(shift_hz=case.shift, lowpass=case.stages[0] if case.stages else None)
    p = engine.Plan(case.fmt, case.sr, n, **kw)
    name = p.kernel_name()
    print(f"{case.name}: {name} | kind {int(p.info.kernel_kind)} flags {int(p.info.kernel_flags)} tile_windows {int(p.info.tile_windows)} "
          f"threads {int(p.info.threads)} windows {int(p.n_windows)}")
    assert case.family(p.info, name), (case.name, name, int(p.info.kernel_kind), int(p.info.kernel_flags))
    return p


def _reference(oracle, case):
    raw, bal = bucket_order_stream(oracle, case)
    ref = _oracle_chain(oracle, raw, case.fmt, case.sr, case.chain_stages()).freq_levels(case.W, case.S)
    assert ref.size > int(bal[-1])
    return raw, bal, ref


def _assert_digits(case, got, ref, bal, first_window=0, what="whole stream"):
    assert got.shape == ref.shape and got.dtype == np.uint8, (case.name, what, got.shape, ref.shape)
    bad = np.flatnonzero(got != ref) + first_window
    print(f"{case.name} [{what}]: {ref.size} windows, {bad.size} differing digits, {int(np.isin(bad, bal).sum())} of them in balanced windows")
    assert np.array_equal(got, ref), (case.name, what, bad[:20].tolist())


@pytest.mark.parametrize("case", BUCKET_ORDER_CASES, ids=lambda c: c.name)
def test_bucket_digits_equal_the_oracle_on_balanced_streams(engine, oracle, case):
    raw, bal, ref = _reference(oracle, case)
    p = _plan(engine, case, raw.size // FMT_BYTES[case.fmt])
    assert p.n_windows == ref.size
    _assert_digits(case, p.run_host(raw), ref, bal)
    p.close()


@pytest.mark.parametrize("case", [c for c in BUCKET_ORDER_CASES if c.paths], ids=lambda c: c.name)
def test_bucket_digits_on_the_device_path_and_in_chunks(engine, oracle, case):
    """the same bytes from a window sub-range of a device-resident slab (it starts off a tile boundary) and from a host run in at
    least three chunks"""
    import torch
    raw, bal, ref = _reference(oracle, case)
    bps = FMT_BYTES[case.fmt]
    p = _plan(engine, case, raw.size // bps)
    whole = p.run_host(raw)
    _assert_digits(case, whole, ref, bal)
    G = max(int(p.info.tile_windows), 1)
    w0 = G + 1 if G > 1 else 3
    cnt = p.n_windows - w0 - 2
    assert cnt > 3 * G and (G == 1 or w0 % G != 0)
    first, count = p.src_range(w0, cnt)
    src = torch.from_numpy(raw[first * bps:(first + count) * bps].copy()).cuda()
    out = torch.full((cnt,), 0xA5, dtype=torch.uint8, device="cuda")
    p.run_device(src, out, w0, cnt, src_first=first, src_count=count)
    torch.cuda.synchronize()
    sub = out.cpu().numpy()
    _assert_digits(case, sub, ref[w0:w0 + cnt], bal, w0, f"device slab, windows {w0} ... {w0 + cnt - 1}")
    assert sub.tobytes() == whole[w0:w0 + cnt].tobytes()
    p.close()
    chunk = 1 << 16
    while raw.size // chunk > 8:
        chunk <<= 1
    small = _plan(engine, case, raw.size // bps, chunk_bytes=chunk)
    got = small.run_host(raw)
    st = small.stats()
    print(f"{case.name}: {int(st.chunks)} chunks of {chunk} bytes")
    assert st.chunks >= 3, (int(st.chunks), chunk, raw.size)
    _assert_digits(case, got, ref, bal, 0, f"{int(st.chunks)} host chunks")
    assert got.tobytes() == whole.tobytes()
    small.close()
