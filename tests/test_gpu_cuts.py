"""The cut list on the device (include/quadrs_hip.h, "cut list").
  * STRICT_CUTS (test_cuts_cpu.strict_cuts: no ambiguous NCO multiplier in any span, held there on the reference alone) byte for byte
    against the oracle's  from -> [shift] -> lowpass  read_at, in all four formats, and two cuts of a described stream of 2^34 + 12 345
    samples against the oracle over the slab with the reference's own multipliers of the absolute indices planted;
  * independence: alone, doubled and shuffled, from pageable, pinned and device memory, through 64 KiB batches: the same bytes every time,
    guards untouched, poison around the slab never read into a result;
  * any shift: the cuts of a burst stream's emissions equal qd_unpack -> qd_shift -> qd_lowpass_block byte for byte, and meet section 5's
    older bounds against the oracle;
  * a shift-free cut of one write block equals that block of the QD_EPI_CF32_BLOCKS plan;
  * lists with empty cuts, the empty list, 4096 one-sample cuts."""
import numpy as np
import pytest

from test_cuts_cpu import BURST_SR, DEEP_N, N_STREAM, SR, burst_stream, deep_cuts, span_of, strict_cuts
from test_gpu_parity import _signal, _to_format
from util import FMT_BYTES, GUARD_BYTE, bits_equal, complex_ulp_err, framed, framed_out

pytestmark = pytest.mark.gpu

_STREAMS, _REFS = {}, {}


def stream(fmt):
    """the 2^17-sample stream of a format: test_gpu_parity's signal in that format's codes (read-only bytes)"""
    if fmt not in _STREAMS:
        _STREAMS[fmt] = _to_format(_signal(np.random.default_rng(20261021), N_STREAM), fmt)
    return _STREAMS[fmt]


def oracle_cut(oracle, data, fmt, sr, cut, first=None, plant=None):
    """the reference's read_at(first, count) of  from -> [shift] -> lowpass  over `data`; plant = (ratio, base): the multipliers of absolute
    indices base ... planted through override_shift (data is then a slab from sample base on and `first` is relative to it)"""
    ch = oracle.Chain.from_bytes(data, fmt, sr)
    if int(cut["shift_hz"]):
        ch = ch.shift(int(cut["shift_hz"]))
        if plant is not None:
            m = len(data) // FMT_BYTES[fmt]
            c, s = oracle.shift_multipliers_f64(plant[0], plant[1], m)
            ch.override_shift(0, np.arange(m, dtype=np.uint64), c.astype(np.float32), s.astype(np.float32))
    ch = ch.lowpass(int(cut["lowpass_hz"]), int(cut["decimate"]), int(cut["taps"]))
    got, y = ch.read_at(int(cut["first"]) if first is None else first, int(cut["count"]))
    assert got == int(cut["count"]), (got, cut)
    return y


def strict_refs(engine, oracle, fmt):
    if fmt not in _REFS:
        refs = [oracle_cut(oracle, stream(fmt), fmt, SR, c) for c in strict_cuts(engine)]
        for r in refs:
            r.setflags(write=False)
        _REFS[fmt] = refs
    return _REFS[fmt]


def assert_same(refs, got, what):
    assert len(refs) == len(got), what
    for k, (r, g) in enumerate(zip(refs, got)):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert r.shape == g.shape and bits_equal(r, g), (what, k, int((r.view(np.uint32) != g.view(np.uint32)).sum()), r.shape)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_strict_cuts_equal_the_oracle(engine, oracle, fmt):
    cuts = strict_cuts(engine)
    got = engine.cuts_run(fmt, SR, N_STREAM, stream(fmt), cuts)
    assert_same(strict_refs(engine, oracle, fmt), got, f"fmt {fmt}")


@pytest.mark.parametrize("which", [0, 1])
def test_deep_cuts_equal_the_oracle_with_planted_multipliers(engine, oracle, which):
    name, base, count, cut = deep_cuts(engine)[which]
    fmt = (0, 3)[which]
    rng = np.random.default_rng(20261021 + which)
    if fmt == 0:
        slab = (rng.standard_normal((count, 2)) * 0.03).astype(np.float32).view(np.uint8).reshape(-1)
    else:
        slab = rng.integers(0, 256, count * FMT_BYTES[fmt], dtype=np.uint8)
    D = int(cut["decimate"])
    ref = oracle_cut(oracle, slab.tobytes(), fmt, SR, cut, first=int(cut["first"]) - base // D, plant=(oracle.shift_ratio(int(cut["shift_hz"]), SR), base))
    import torch
    for src in (slab, torch.from_numpy(slab.copy()).cuda()):
        got = engine.cuts_run(fmt, SR, DEEP_N, src, np.array([cut]), src_first=base, src_count=count)
        assert_same([ref], got, name)


@pytest.mark.parametrize("fmt", [0, 1])
def test_a_cut_depends_on_nothing_but_itself(engine, oracle, fmt):
    import torch
    cuts = strict_cuts(engine)
    refs = strict_refs(engine, oracle, fmt)
    data = np.frombuffer(stream(fmt), dtype=np.uint8)
    bps = FMT_BYTES[fmt]
    # alone
    for k in (0, 5, 11, 17, 23, 24, 31):
        assert_same([refs[k]], engine.cuts_run(fmt, SR, N_STREAM, data, cuts[k:k + 1]), f"alone {k}")
    # every cut twice, shuffled into a list of 64
    order = np.random.default_rng(7).permutation(np.concatenate([np.arange(32), np.arange(32)]))
    assert_same([refs[k] for k in order], engine.cuts_run(fmt, SR, N_STREAM, data, cuts[order]), "shuffled")
    # framed sources and outputs of every memory kind; the device slab is larger than needed
    offs, lo, count = engine.cuts_geometry(SR, N_STREAM, cuts)
    total = int(offs[-1])
    for kind, more, chunk in (("host", 0, 0), ("pinned", 0, 0), ("device", 1000, 0), ("host", 0, 65536), ("device", 0, 65536)):
        a, b = lo - more, lo + count + more
        src = framed(kind, fmt, 0, 1 << 16, data[a * bps:b * bps], 1 << 16, engine)
        out = framed_out(kind, 1 << 16, total * 8, engine)
        got = engine.cuts_run(fmt, SR, N_STREAM, src.body, cuts, src_first=a, src_count=b - a, pinned=kind == "pinned", out=out.body, chunk_bytes=chunk)
        if kind == "device":
            torch.cuda.synchronize()
        assert_same(refs, got, (kind, more, chunk))
        snap = out.snapshot()
        assert (snap[:out.lo] == GUARD_BYTE).all() and (snap[out.hi:] == GUARD_BYTE).all(), kind
        assert snap[out.lo:out.hi].tobytes() == b"".join(r.tobytes() for r in refs), kind
        assert (src.snapshot() == src.uploaded).all(), kind
        del got
        src.close()
        out.close()


def test_cuts_of_emissions_equal_the_fine_grained_calls(engine, oracle):
    x = burst_stream()
    n = x.shape[0]
    data = x.tobytes()
    plan = engine.Plan(engine.FMT_CF32, BURST_SR, n, width=64, stride=64)
    records, found = plan.emissions(data, np.full(64, 4.0, dtype=np.float32), min_cells=8)
    assert found == len(records) == 5
    cuts = np.array([engine.cut_of_emission(plan.desc, 0, r, engine.cut_rule(1, 2, 1)) for r in records], dtype=engine.CUT_DTYPE)
    assert (cuts["shift_hz"] != 0).all() and (cuts["count"] > 256).all()
    got = engine.cuts_run(engine.FMT_CF32, BURST_SR, n, data, cuts)
    exact = total = 0
    for c, g in zip(cuts, got):
        a, b = span_of(c)
        raw = engine.unpack(engine.FMT_CF32, data[a * 8:b * 8])
        shifted = engine.shift(raw, a, engine.shift_ratio(int(c["shift_hz"]), BURST_SR))
        made, fine = engine.lowpass_block(engine.lowpass_design(int(c["lowpass_hz"]), BURST_SR, int(c["taps"])), int(c["decimate"]), shifted)
        assert made == int(c["count"]) and bits_equal(fine, g), (c, int((fine.view(np.uint32) != g.view(np.uint32)).sum()))
        ref = oracle_cut(oracle, data, 0, BURST_SR, c)
        assert complex_ulp_err(ref, g).max() <= 1.0, c
        exact += int((ref.view(np.uint32) == g.view(np.uint32)).sum())
        total += ref.size
    assert exact >= 0.999 * total, (exact, total)


@pytest.mark.parametrize("B", [64, 1024])
def test_a_shift_free_cut_is_a_write_block(engine, B):
    fmt, lp = 3, (900_000, 8, 120)
    data = stream(fmt)
    plan = engine.Plan(fmt, SR, N_STREAM, lowpass=lp, width=B, epilogue=engine.EPI_CF32_BLOCKS)
    assert plan.n_windows >= 3
    blocks = plan.run_host(data).reshape(plan.n_windows, B, 2)
    cuts = np.array([(0, lp[0], lp[1], lp[2], b * B, B) for b in range(plan.n_windows)], dtype=engine.CUT_DTYPE)
    got = engine.cuts_run(fmt, SR, N_STREAM, data, cuts)
    assert_same(list(blocks), got, f"B {B}")


def test_degenerate_lists(engine, oracle):
    fmt = 0
    cuts = strict_cuts(engine)[:6].copy()
    refs = strict_refs(engine, oracle, fmt)[:6]
    cuts["count"][[1, 4]] = 0
    got = engine.cuts_run(fmt, SR, N_STREAM, stream(fmt), cuts)
    assert got[1].shape == got[4].shape == (0, 2)
    assert_same([refs[k] for k in (0, 2, 3, 5)], [got[k] for k in (0, 2, 3, 5)], "with empty cuts")
    assert engine.cuts_run(fmt, SR, N_STREAM, stream(fmt), cuts[:0]) == []
    # 4096 cuts of one sample: output i of a cut is that cut's own sample only while the filter is whole, so every one-sample cut is
    # read_at(first, 1) with its block's truncation: the reference's value for it
    ones = np.zeros(4096, dtype=engine.CUT_DTYPE)
    ones["shift_hz"], ones["lowpass_hz"], ones["decimate"], ones["taps"], ones["count"] = 999_983, 300_000, 4, 40, 1
    ones["first"] = 10_001 + 3 * np.arange(4096)
    got = engine.cuts_run(fmt, SR, N_STREAM, stream(fmt), ones)
    ch = oracle.Chain.from_bytes(stream(fmt), fmt, SR).shift(999_983).lowpass(300_000, 4, 40)
    for k in range(0, 4096, 97):
        made, y = ch.read_at(int(ones["first"][k]), 1)
        assert made == 1 and bits_equal(y, got[k]), k
