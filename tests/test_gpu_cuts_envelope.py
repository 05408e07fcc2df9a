"""The cut list across its whole envelope on the device (include/quadrs_hip.h, "cut list").  The tables, streams
and references are cuts_util.py's, and test_cuts_envelope_cpu.py holds their conditions on the reference alone; every comparison here is
byte for byte:
  * the envelope table (the corners of qd_cuts_plan.h's tile geometry) and the alignment table (every 16-byte load residue, first == 0,
    spans that end on the stream's last sample) in all four formats, from host, pinned and device memory;
  * a device source whose base lies at every residue modulo 16;
  * every sample code, runs of signed zeros, one NaN and one Inf sample, with and without a shift;
  * a shift-free cut, a first-order and a second-order one over one slab in one list, at samples where the two orders round differently;
  * 600 lane tables and 150 tap tables in one call; calls of more than kCutsBatchTiles tiles.
Every call that passes its own buffers hands over framed sources and guarded outputs; guards stay intact and sources unchanged."""
import numpy as np
import pytest

import cuts_util as U
from test_cuts_cpu import span_of
from util import FMT_BYTES, GUARD_BYTE, POISON_BYTES, Framed, bits_equal, framed, framed_out, poison

pytestmark = pytest.mark.gpu

FRAME = 1 << 16


def run_framed(engine, fmt, sr, n_samples, kind, data, cuts, src_first=0, chunk=0, out_kind=None, flat=False):
    """one cuts_run call from a framed source of memory `kind` into a guarded output of out_kind (None: the source's); checks the guards and
    the source and returns the cuts' outputs, numpy views of the payload as the call left it (flat: the payload itself, (total, 2))"""
    offs, _, _ = engine.cuts_geometry(sr, n_samples, cuts)
    total = int(offs[-1])
    out_kind = kind if out_kind is None else out_kind
    assert "pinned" not in (kind, out_kind) or kind == out_kind
    src = framed(kind, fmt, 0, FRAME, data, FRAME, engine)
    out = framed_out(out_kind, FRAME, total * 8, engine)
    try:
        got = engine.cuts_run(fmt, sr, n_samples, src.body, cuts, src_first=src_first, src_count=len(data) // FMT_BYTES[fmt], pinned=kind == "pinned",
                              out=out.body, chunk_bytes=chunk)
        assert len(got) == len(cuts)
        del got
        snap = out.snapshot()
        assert (snap[:out.lo] == GUARD_BYTE).all() and (snap[out.hi:] == GUARD_BYTE).all(), kind
        assert (src.snapshot() == src.uploaded).all(), kind
    finally:
        src.close()
        out.close()
    payload = snap[out.lo:out.hi].view(np.float32).reshape(-1, 2)
    return payload if flat else [payload[int(offs[k]):int(offs[k + 1])] for k in range(len(cuts))]


def assert_same(refs, got, what):
    assert len(refs) == len(got), what
    for k, (r, g) in enumerate(zip(refs, got)):
        assert r.shape == g.shape and bits_equal(r, g), (what, k, int((r.view(np.uint32) != g.view(np.uint32)).sum()), r.shape)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_envelope_and_alignment_tables_equal_the_oracle(engine, oracle, fmt):
    data = U.signal_stream(fmt)
    env, align = U.envelope_cuts(), U.align_cuts()
    refs = U.oracle_refs(oracle, "env", data, fmt, env) + U.oracle_refs(oracle, "align", data, fmt, align)
    cuts = np.concatenate([env, align])
    for kind in ("host", "device"):
        assert_same(refs, run_framed(engine, fmt, U.SR, U.N_STREAM, kind, data, cuts), (fmt, kind))
    assert_same(refs[len(env):], run_framed(engine, fmt, U.SR, U.N_STREAM, "pinned", data, align), (fmt, "pinned"))


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_a_device_base_at_every_residue(engine, oracle, fmt):
    """k_cuts takes its ragged head from the pointer: the same list from device sources whose base lies k whole samples off a 16-byte boundary,
    (i) views of one buffer with src_first moved along, (ii) the same slab laid k samples further into its allocation"""
    import torch
    bps, spv = FMT_BYTES[fmt], U.SPV[fmt]
    A, B = U.FLOOR, U.FLOOR + 13_000
    cuts = U.align_cuts()
    pick = np.array([A + 2 * spv + 3 <= span_of(c)[0] and span_of(c)[1] <= B for c in cuts])
    assert pick.sum() >= 128 and {bool(s) for s in cuts[pick]["shift_hz"]} == {False, True}
    refs = [r for r, p in zip(U.oracle_refs(oracle, "align", U.signal_stream(fmt), fmt, cuts), pick) if p]
    cuts = cuts[pick]
    slab = U.signal_stream(fmt)[A * bps:B * bps]
    offsets = list(range(spv)) + [spv + 1, 2 * spv + 3]
    assert {(k * bps) % 16 for k in offsets} == set(range(0, 16, bps))
    whole = framed("device", fmt, 0, FRAME, slab, FRAME, engine)
    assert whole.body.data_ptr() % 16 == 0
    for k in offsets:
        view = whole.body[k * bps:]
        assert view.data_ptr() % 16 == (k * bps) % 16
        assert_same(refs, engine.cuts_run(fmt, U.SR, U.N_STREAM, view, cuts, src_first=A + k, src_count=B - A - k), (fmt, "view", k))
    torch.cuda.synchronize()
    assert (whole.snapshot() == whole.uploaded).all()
    whole.close()
    for k in offsets[1:]:
        front = poison(0, FRAME + k * bps, 0) if fmt == 0 else np.full(FRAME + k * bps, POISON_BYTES[0], dtype=np.uint8)
        moved = Framed("device", front, slab, poison(fmt, FRAME, 0), engine)
        assert moved.body.data_ptr() % 16 == (k * bps) % 16
        assert_same(refs, engine.cuts_run(fmt, U.SR, U.N_STREAM, moved.body, cuts, src_first=A, src_count=B - A), (fmt, "moved", k))
        assert (moved.snapshot() == moved.uploaded).all()
        moved.close()


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_every_code_through_a_cut(engine, oracle, fmt):
    data, cuts = U.value_stream(fmt), U.value_cuts(fmt)
    n = data.size // FMT_BYTES[fmt]
    refs = U.oracle_refs(oracle, "codes", data, fmt, cuts)
    for kind in ("host", "device"):
        assert_same(refs, run_framed(engine, fmt, U.SR, n, kind, data, cuts), (fmt, kind))


def test_signed_zeros_through_a_cut(engine, oracle):
    data, _ = U.zero_stream()
    cuts = U.zero_cuts()
    refs = U.oracle_refs(oracle, "zeros", data, 0, cuts)
    assert any((r == 0).any() for r in refs)                                      # whole reaches of zeros: outputs that are zeros, with the reference's signs
    for kind in ("host", "device"):
        assert_same(refs, run_framed(engine, 0, U.SR, U.N_STREAM, kind, data, cuts), kind)


def test_a_nan_and_an_inf_sample_through_a_cut(engine, oracle):
    cuts = U.special_cuts()
    refs = U.oracle_refs(oracle, "special", U.special_stream(), 0, cuts)
    clean_refs = U.oracle_refs(oracle, "signal", U.special_stream(False), 0, cuts)
    for kind in ("host", "device"):
        got = run_framed(engine, 0, U.SR, U.N_STREAM, kind, U.special_stream(), cuts)
        clean = run_framed(engine, 0, U.SR, U.N_STREAM, kind, U.special_stream(False), cuts)
        assert_same(clean_refs, clean, kind)
        for c, r, g, cl in zip(cuts, refs, got, clean):
            nan = np.isnan(r)
            assert nan.any() or np.isinf(r).any(), c
            assert (np.isnan(g) == nan).all(), (kind, c)
            assert (r.view(np.uint32)[~nan] == g.view(np.uint32)[~nan]).all(), (kind, c)
            far = ~(U.reaches(c, U.NAN_AT) | U.reaches(c, U.INF_AT))
            assert far.sum() >= 16 and np.isfinite(g[far]).all() and bits_equal(g[far], cl[far]), (kind, c)


@pytest.mark.parametrize("k", range(len(U.SENSITIVE_CASES)))
def test_both_nco_orders_in_one_list(engine, oracle, k):
    sr, n_samples, base, slab, cuts = U.sensitive_case(k)
    refs = U.sensitive_refs(oracle, k)
    for order in ([0, 1, 2], [2, 1, 0]):
        for kind in ("host", "device"):
            got = run_framed(engine, 0, sr, n_samples, kind, slab, cuts[order], src_first=base)
            assert_same([refs[i] for i in order], got, (k, order, kind))


def test_many_tables_in_one_call(engine, oracle):
    import torch
    cuts = U.many_cuts()
    data = U.signal_stream(0)
    whole = run_framed(engine, 0, U.SR, U.N_STREAM, "device", data, cuts)
    assert_same(whole, run_framed(engine, 0, U.SR, U.N_STREAM, "host", data, cuts), "host")
    src = framed("device", 0, 0, FRAME, data, FRAME, engine)
    for i, (c, w) in enumerate(zip(cuts, whole)):                                  # one call a cut: its own lane table and taps table
        assert_same([w], engine.cuts_run(0, U.SR, U.N_STREAM, src.body, cuts[i:i + 1]), ("alone", i))
    torch.cuda.synchronize()
    assert (src.snapshot() == src.uploaded).all()
    src.close()
    raw = data.tobytes()
    for i in range(0, U.MANY_N, 15):                                               # 40 cuts against the fine-grained calls
        c = cuts[i]
        a, b = span_of(c)
        x = engine.shift(engine.unpack(engine.FMT_CF32, raw[a * 8:b * 8]), a, engine.shift_ratio(int(c["shift_hz"]), U.SR))
        made, fine = engine.lowpass_block(engine.lowpass_design(int(c["lowpass_hz"]), U.SR, int(c["taps"])), int(c["decimate"]), x)
        assert made == int(c["count"]) and bits_equal(fine, whole[i]), c
    refs = U.oracle_refs(oracle, "many", data, 0, cuts)
    ok = U.many_clean(oracle)
    assert_same([r for r, o in zip(refs, ok) if o], [w for w, o in zip(whole, ok) if o], "oracle")


def test_more_one_output_cuts_than_a_batch_holds(engine, oracle):
    """17 000 tiles of shifted cuts: the second batch reads the lane table that the first one filled"""
    ones = U.cap_ones()
    data = U.signal_stream(0)
    dev = run_framed(engine, 0, U.SR, U.N_STREAM, "device", data, ones, flat=True)              # device to device: nothing waits between the batches
    assert dev.shape == (ones.size, 2)
    assert bits_equal(dev, run_framed(engine, 0, U.SR, U.N_STREAM, "host", data, ones, flat=True)), "host"
    pieces = [run_framed(engine, 0, U.SR, U.N_STREAM, "device", data, ones[a:a + 4096], out_kind="host", flat=True) for a in range(0, ones.size, 4096)]
    assert bits_equal(dev, np.concatenate(pieces)), "pieces"
    ch = oracle.Chain.from_bytes(data, 0, U.SR).shift(U.CAP_SHAPE[0]).lowpass(*U.CAP_SHAPE[1:])
    for k in list(range(0, ones.size, 97)) + [16_383, 16_384, 16_385, ones.size - 1]:
        made, y = ch.read_at(int(ones["first"][k]), 1)
        assert made == 1 and bits_equal(y, dev[k:k + 1]), k


def test_one_cut_longer_than_a_batch_holds(engine, oracle):
    data, long = U.cap_long()
    n = data.size // 2
    c = long[0]
    first, count = int(c["first"]), int(c["count"])
    ref = U.oracle_refs(oracle, "long", data, 2, long)
    dev = run_framed(engine, 2, U.SR, n, "device", data, long)
    assert_same(ref, dev, "device")
    assert_same(ref, run_framed(engine, 2, U.SR, n, "host", data, long), "host")
    # short cuts of their own at the batch's seams: (1, 2) truncates nothing (T - T/2 <= D), so a short cut's outputs are the long cut's
    seams = list(range(256 * 4096, count, 256 * 4096))
    assert len(seams) == 4 and 256 * 4096 * 4 == U.header_constants()["kCutsBatchTiles"] * 256
    short = U.make_cuts([(0, int(c["lowpass_hz"]), 1, 2, first + m - 8, 16) for m in seams] + [(0, int(c["lowpass_hz"]), 1, 2, first + count - 300, 300)])
    got = run_framed(engine, 2, U.SR, n, "device", data, short)
    assert_same([ref[0][m - 8:m + 8] for m in seams] + [ref[0][count - 300:]], got, "short")
    assert_same(got, [dev[0][m - 8:m + 8] for m in seams] + [dev[0][count - 300:]], "short against long")
