"""The symbol list on the device (include/quadrs_hip.h, "symbol list").
  * byte for byte against the oracle: about 44 segments at odd elements of one 2^16-sample buffer (FSK, on / off keying around the mark
    threshold, noise, blank rows, a NaN sample, tie-balanced real windows), W = 2 ... 4096, S in {1, W/2, W, W + 3}, both sinks;
  * byte for byte against one plan per segment, Blackman-Harris windows included;
  * independence: alone, doubled and shuffled, from pageable, pinned and device memory with guards and poison, the source unchanged;
  * degenerate lists;
  * qd_cuts_symbols = qd_cuts_run then qd_symbols_run = the oracle, in four formats, through batches and IQ groups;
  * end to end: emissions -> cuts -> digits -> bits_scan returns the planted bits of every packet.
The streams' conditions are held in test_symbols_cpu.py on the oracle alone."""
import numpy as np
import pytest

import symbols_util as U
from test_cuts_cpu import N_STREAM, SR as CUT_SR, strict_cuts
from test_gpu_cuts import strict_refs, stream
from util import FMT_BYTES, GUARD_BYTE, POISON_WORDS, framed, framed_out

pytestmark = pytest.mark.gpu

CASES = [(W, S) for W in U.WIDTHS for S in U.strides(W)]


def desc_of(engine, epi, W, S, windowing=0, iq_bytes=0, rmin=None):
    rng = None if epi == U.BUCKET else ((U.mark_min(W) if rmin is None else rmin), 1.0)
    return engine.symbols_desc(epi, W, S, rng=rng, windowing=windowing, iq_bytes=iq_bytes)


def assert_same(refs, got, what):
    assert len(refs) == len(got), what
    for k, (r, g) in enumerate(zip(refs, got)):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert r.shape == g.shape and np.array_equal(r, g), (what, k, r.shape, g.shape, int((r != g).sum()) if r.shape == g.shape else None)


# ------------------------------------------------------------------ 1. the oracle, byte for byte

@pytest.mark.parametrize("epi", [U.BUCKET, U.MARK])
@pytest.mark.parametrize("W,S", CASES)
def test_segments_equal_the_oracle(engine, oracle, W, S, epi):
    x = U.buffer(oracle)
    got = engine.symbols_run(desc_of(engine, epi, W, S), x, U.segments(W, S))
    assert_same(U.references(oracle, epi, W, S), got, (W, S, epi))


def test_the_default_mark_threshold_is_the_reference_s(engine, oracle):
    """has_range == 0: min is 0.08f (src/fft.rs:22-23)"""
    x = U.buffer(oracle)
    W, S = 2, 1                                     # (|X| of the blank rows and of the 0.03 ... 0.07 tones lies about 0.08 at this width)
    segs = U.segments(W, S)
    refs = [U.oracle_bytes(oracle, x[int(f):int(f) + int(c)], U.MARK, W, S, rmin=np.float32(0.08)) for f, c in segs]
    every = np.concatenate(refs)
    assert 0.1 <= every.mean() <= 0.9, every.mean()
    assert_same(refs, engine.symbols_run(engine.symbols_desc(U.MARK, W, S), x, segs), "default min")


# ------------------------------------------------------------------ 2. one plan per segment

@pytest.mark.parametrize("windowing", [0, 1])
@pytest.mark.parametrize("W,S", [(8, 4), (64, 64), (64, 67), (1024, 512)])
def test_segments_equal_one_plan_each(engine, oracle, W, S, windowing):
    x = U.buffer(oracle)
    segs = U.segments(W, S)
    for epi in (U.BUCKET, U.MARK):
        got = engine.symbols_run(desc_of(engine, epi, W, S, windowing=windowing), x, segs)
        plans = {}
        ran = 0
        for (f, c), g in zip(segs, got):
            f, c = int(f), int(c)
            if c <= W:
                assert g.size == 0
                continue
            if c not in plans:
                plans[c] = engine.Plan(engine.FMT_CF32, U.SR, c, width=W, stride=S, epilogue=epi, rng=None if epi == U.BUCKET else (U.mark_min(W), 1.0),
                                       windowing=windowing, kernel_policy=engine.KERNEL_NO_PLAN_TIME)
            want = plans[c].run_host(x[f:f + c].tobytes()).reshape(-1)
            assert want.size == g.size and np.array_equal(want, g), (W, S, epi, windowing, f, c, int((want != g).sum()) if want.size == g.size else None)
            ran += want.size
        for p in plans.values():
            p.close()
        assert ran > 0
    if windowing == 0:
        return
    # the window is not a no-op on these streams: some byte of the case differs from the rectangular run
    plain = np.concatenate(engine.symbols_run(desc_of(engine, U.BUCKET, W, S), x, segs))
    assert (plain != np.concatenate(engine.symbols_run(desc_of(engine, U.BUCKET, W, S, windowing=1), x, segs))).any()


# ------------------------------------------------------------------ 3. a segment depends on nothing but itself

def poisoned_gaps(x, segs, which):
    """the buffer with every sample that no segment covers replaced by the NaN-pattern / huge-value poison word"""
    covered = np.zeros(x.shape[0], dtype=bool)
    for f, c in segs:
        covered[int(f):int(f) + int(c)] = True
    y = x.copy().view(np.uint32)
    y[~covered] = POISON_WORDS[which]
    return y.view(np.float32), int((~covered).sum())


@pytest.mark.parametrize("epi", [U.BUCKET, U.MARK])
@pytest.mark.parametrize("W,S", [(64, 32), (256, 256), (4096, 4099)])
def test_a_segment_depends_on_nothing_but_itself(engine, oracle, W, S, epi):
    import torch
    x = U.buffer(oracle)
    segs = U.segments(W, S)
    refs = U.references(oracle, epi, W, S)
    d = desc_of(engine, epi, W, S)
    n = segs.size
    # alone
    for k in range(n):
        assert_same([refs[k]], engine.symbols_run(d, x, segs[k:k + 1]), f"alone {k}")
    # every segment twice, shuffled: overlapping and repeated by construction
    order = np.random.default_rng(7).permutation(np.concatenate([np.arange(n), np.arange(n)]))
    assert_same([refs[k] for k in order], engine.symbols_run(d, x, segs[order]), "shuffled")
    # framed sources and outputs of every memory kind, poison in the gaps between the segments and around the buffer
    total = sum(r.size for r in refs)
    for which, kind in ((0, "host"), (1, "pinned"), (0, "device"), (1, "device")):
        y, gaps = poisoned_gaps(x, segs, which)
        assert gaps >= 256
        src = framed(kind, 0, which, 1 << 16, y.view(np.uint8).reshape(-1), 1 << 16, engine)
        out = framed_out(kind, 1 << 12, total, engine)
        got = engine.symbols_run(d, src.body, segs, pinned=kind == "pinned", out=out.body)
        if kind == "device":
            torch.cuda.synchronize()
        assert_same(refs, got, (kind, which))
        snap = out.snapshot()
        assert (snap[:out.lo] == GUARD_BYTE).all() and (snap[out.hi:] == GUARD_BYTE).all(), kind
        assert snap[out.lo:out.hi].tobytes() == b"".join(r.tobytes() for r in refs), kind
        assert (src.snapshot() == src.uploaded).all(), kind
        del got
        src.close()
        out.close()


# ------------------------------------------------------------------ 4. degenerate lists

N_SHORT_AT = U.N_BUF - 16


def test_degenerate_lists(engine, oracle):
    x = U.buffer(oracle)
    W = S = 16
    for epi in (U.BUCKET, U.MARK):
        d = desc_of(engine, epi, W, S)
        assert engine.symbols_run(d, x, np.zeros(0, dtype=engine.SEGMENT_DTYPE)) == []
        short = np.array([(1, 0), (3, W - 1), (5, W), (101, 1), (N_SHORT_AT, W)], dtype=engine.SEGMENT_DTYPE)
        out = np.full(64, 0x5A, dtype=np.uint8)
        got = engine.symbols_run(d, x, short, out=out)
        assert [g.size for g in got] == [0] * 5 and (out == 0x5A).all()
        import torch
        dev, out_dev = torch.from_numpy(np.array(x)).cuda(), torch.full((64,), 0x5A, dtype=torch.uint8, device="cuda")
        engine.symbols_run(d, dev, short, out=out_dev)
        torch.cuda.synchronize()
        assert (out_dev.cpu().numpy() == 0x5A).all()
        # 4096 segments of exactly one window each
        ones = np.zeros(4096, dtype=engine.SEGMENT_DTYPE)
        ones["first"], ones["count"] = 1 + 13 * np.arange(4096), W + S
        offs = engine.symbols_geometry(d, ones)
        assert offs.tolist() == list(range(4097))
        got = np.concatenate(engine.symbols_run(d, x, ones))
        assert got.size == 4096
        for k in range(0, 4096, 41):
            f = int(ones["first"][k])
            assert U.oracle_bytes(oracle, x[f:f + W + S], epi, W, S).tolist() == [int(got[k])], (epi, k)
        assert 0.05 < got.mean() < 0.95
    # width 1, the smallest power of two: X[0] is the sample, first = 0 and second = |x|, so the digit is 0 unless |x| is 0 or NaN;
    # a row is blank when |x| < min
    seg = np.array([(U.NAN_AT - 301, 700)], dtype=engine.SEGMENT_DTYPE)
    y = x[U.NAN_AT - 301:U.NAN_AT + 399][:699].astype(np.float64)
    mag = np.hypot(y[:, 0], y[:, 1]).astype(np.float32)
    assert engine.symbols_run(engine.symbols_desc(U.BUCKET, 1, 1), x, seg)[0].tolist() == np.where(np.float32(0) < mag, 0, 1).tolist()
    assert engine.symbols_run(engine.symbols_desc(U.MARK, 1, 1, rng=(0.4, 1.0)), x, seg)[0].tolist() == np.where(mag < np.float32(0.4), 0, 1).tolist()


# ------------------------------------------------------------------ 5. cuts and symbols in one call

CUT_W = 16
_CUT_REFS = {}


def cut_case(engine, oracle, fmt, epi):
    """(desc arguments, [oracle bytes of cut k]) of the strict cuts in a format: the oracle's  from -> [shift] -> lowpass  read_at of each
    cut re-viewed as a stream of its own, then freq_levels or marks.  The mark threshold is the median, over all windows, of the window's
    largest |X| on the oracle: both marks occur."""
    key = (fmt, epi)
    if key not in _CUT_REFS:
        iq = strict_refs(engine, oracle, fmt)
        S = CUT_W if epi == U.BUCKET else CUT_W // 2
        rmin = None
        if epi == U.MARK:
            peaks = []
            for y in iq:
                if y.shape[0] > CUT_W:
                    norms, _ = oracle.Chain.from_bytes(y.tobytes(), 0, CUT_SR).spark_fft(CUT_W, S, want_codes=False)
                    peaks.append(norms.max(axis=1))
            rmin = float(np.float32(np.median(np.concatenate(peaks))))
        refs = [U.oracle_bytes(oracle, y, epi, CUT_W, S, sr=CUT_SR, rmin=rmin) for y in iq]
        every = np.concatenate(refs)
        assert every.size > 300 and 0.05 <= every.mean() <= 0.95, (fmt, epi, every.size, every.mean())
        _CUT_REFS[key] = (S, rmin, refs)
    return _CUT_REFS[key]


@pytest.mark.parametrize("epi", [U.BUCKET, U.MARK])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_cuts_symbols_equals_the_two_calls_and_the_oracle(engine, oracle, fmt, epi):
    import torch
    cuts = strict_cuts(engine)
    S, rmin, refs = cut_case(engine, oracle, fmt, epi)
    data = np.frombuffer(stream(fmt), dtype=np.uint8)
    # the two calls
    iq = engine.cuts_run(fmt, CUT_SR, N_STREAM, data, cuts)
    segs = np.zeros(cuts.size, dtype=engine.SEGMENT_DTYPE)
    segs["count"] = cuts["count"]
    segs["first"] = np.concatenate([[0], np.cumsum(cuts["count"])[:-1]])
    two = engine.symbols_run(desc_of(engine, epi, CUT_W, S, rmin=rmin), np.concatenate(iq), segs)
    assert_same(refs, two, "cuts_run then symbols_run")
    # one call: every memory kind, batches of 64 KiB of source, IQ groups of 16 KiB (at least three of them)
    iq_bytes = 8 * 2048
    assert int(cuts["count"].max()) * 8 <= iq_bytes and int(cuts["count"].sum()) * 8 > 3 * iq_bytes
    total = sum(r.size for r in refs)
    _, lo, count = engine.cuts_geometry(CUT_SR, N_STREAM, cuts)
    bps = FMT_BYTES[fmt]
    for kind, chunk, cap in (("host", 0, 0), ("host", 65536, iq_bytes), ("pinned", 65536, iq_bytes), ("device", 0, iq_bytes), ("device", 65536, 0)):
        src = framed(kind, fmt, 0, 1 << 16, data[lo * bps:(lo + count) * bps], 1 << 16, engine)
        out = framed_out(kind, 1 << 12, total, engine)
        got = engine.cuts_symbols(fmt, CUT_SR, N_STREAM, src.body, cuts, desc_of(engine, epi, CUT_W, S, iq_bytes=cap, rmin=rmin), src_first=lo, src_count=count,
                                  pinned=kind == "pinned", out=out.body, chunk_bytes=chunk)
        if kind == "device":
            torch.cuda.synchronize()
        assert_same(refs, got, (kind, chunk, cap))
        snap = out.snapshot()
        assert (snap[:out.lo] == GUARD_BYTE).all() and (snap[out.hi:] == GUARD_BYTE).all(), kind
        assert snap[out.lo:out.hi].tobytes() == b"".join(r.tobytes() for r in refs), kind
        assert (src.snapshot() == src.uploaded).all(), kind
        del got
        src.close()
        out.close()
    # a cut larger than the workspace: refused, out untouched
    out = np.full(total, 0x5A, dtype=np.uint8)
    with pytest.raises(engine.QuadrsError) as err:
        engine.cuts_symbols(fmt, CUT_SR, N_STREAM, data, cuts, desc_of(engine, epi, CUT_W, S, iq_bytes=8 * int(cuts["count"].max()) - 8, rmin=rmin), out=out)
    assert err.value.code == engine._ffi.ERR_UNSUPPORTED and "iq_bytes" in str(err.value) and (out == 0x5A).all()


# ------------------------------------------------------------------ 6. end to end

def test_planted_bits_come_back(engine):
    x = U.e2e_stream()
    n = x.shape[0]
    data = x.tobytes()
    plan = engine.Plan(engine.FMT_CF32, U.E2E_SR, n, width=U.E2E_W, stride=U.E2E_W)
    records, found = plan.emissions(data, np.full(U.E2E_W, U.E2E_LEVEL, dtype=np.float32), min_cells=8)
    assert found == len(records) == len(U.E2E_BINS)
    cuts = np.array([engine.cut_of_emission(plan.desc, 0, r, engine.cut_rule(*U.E2E_RULE)) for r in records], dtype=engine.CUT_DTYPE)
    digits = engine.cuts_symbols(engine.FMT_CF32, U.E2E_SR, n, data, cuts, engine.symbols_desc(U.BUCKET, U.E2E_SINK_W, U.E2E_SINK_W))
    for cut, dg, bits in zip(cuts, digits, U.e2e_bits()):
        err, got = engine.bits_scan(dg, U.e2e_scale(cut))
        assert got.tolist() == bits.tolist(), (cut, err, got.tolist(), bits.tolist())
