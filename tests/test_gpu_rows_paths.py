"""QD_EPI_ROWS_F32, the paths tests/test_gpu_rows.py leaves unrun: every loader of k_bluestein<FMT, NCO> (A), a Bluestein width
behind shift + lowpass — the row-mode kernel with an NCO writing the carrier (B), the row-mode kernels with the second-order NCO
(C), one plan whose slice moves, i.e. every branch of ensure_rowtab (D), and rows at absolute indices past 2^32 of a long stream
(E).  The comparison rules are those of test_gpu_rows.py, none new:

  * power-of-two rows behind a shift: the NCO rule row by row (row i is window offs[i] of a stride-1 sink);
  * Bluestein rows: _bluestein_check, 2 ulp_f32 of the reference norm plus 1e-12 of the row's l1 norm, with NO row excluded also
    behind a shift.  That holds on a condition, asserted on the CPU before the comparison: the source span of the rows holds no
    REAL tie (util.real_ties: a multiplier component whose two f32 candidates lie more than 1e-13 apart).  The ambiguous
    components that do occur in these spans are zero crossings, 1e-19 ... 1e-14 apart.

Streams: those of test_gpu_rows.py; for E seeded slabs of 70 000 samples at `base` of a described 2^34 (cf32) / 2^33 (cs8) sample
stream, the reference being the oracle's chain over the slab with the ABSOLUTE multipliers planted through its override hook
(test_rows_cpu.py holds the translation of the row offsets)."""
import numpy as np
import pytest

from test_gpu_parity import assert_explained, record_observed
from test_gpu_rows import CHAINS, LP16, SR, _bluestein_check, _chain, _data, _lens, _plan, _slices
from test_rows_cpu import DEEP_CASES, DEEP_OUT_LEN, DEEP_SPAN
from util import FMT_BYTES, ambiguous_windows, bits_equal, real_ties

pytestmark = pytest.mark.gpu

SHIFTS = [280000, -1234567]


def _no_real_tie(oracle, engine, fmt, n, W, out_len, slice_, shift, lp, what):
    """the precondition of the Bluestein bound behind a shift: no real tie among the multipliers of the source samples the rows read"""
    _, first, count = engine.rows_geometry(fmt, SR, n, W, out_len, slice_, 1, shift_hz=shift, lowpass=lp)
    ambiguous, ties = real_ties(oracle.shift_ratio(shift, SR), first, count)
    assert not ties, (what, first, count, ties[:4])
    return ambiguous


def _nco_rule_rows(ref, got, offs, stages, W, what):
    """the NCO rule row by row; returns the number of rows that differ at all"""
    differing = np.nonzero((ref.view(np.uint32) != got.view(np.uint32)).any(axis=1))[0]
    for i in differing:
        assert_explained(ref[i:i + 1], got[i:i + 1], ((stages, W, 1, SR), int(offs[i])), f"{what} row {i}")
    return len(differing)


def _stages(shift, lp):
    return [("shift", shift)] + ([("lowpass", lp)] if lp else [])


# ------------------------------------------------------------------ A: the 12 loaders of k_bluestein

@pytest.mark.parametrize("shift,order", [(None, 0), (280000, 1), (280000, 2), (-1234567, 1), (-1234567, 2)])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_every_bluestein_loader(engine, oracle, fsk, fmt, shift, order):
    W, out_len = 100, 48
    data = _data(fsk, fmt)
    n = len(data) // FMT_BYTES[fmt]
    ch = _chain(oracle, data, fmt, shift, None)
    p = _plan(engine, fmt, n, W, shift, None, nco_order=order)
    assert f"k_bluestein<fmt {fmt}, nco {order}>" in p.kernel_name(), p.kernel_name()
    for windowing in (0, 1):
        for slice_ in (None, (10, 2000)):
            what = f"rows loader W={W} fmt{fmt} shift {shift} nco {order} windowing={windowing} slice={slice_}"
            if shift is not None:
                _no_real_tie(oracle, engine, fmt, n, W, out_len, slice_, shift, None, what)
            rc, ref, offs = ch.take_fft(W, out_len, slice_, windowing)
            assert rc == 0
            got = p.take_fft(data, out_len, slice_, windowing)
            _bluestein_check(ch, ref, got, offs, W, what)
    p.close()


# ------------------------------------------------------------------ B: row mode with an NCO into the carrier, then k_bluestein<0, 0>

@pytest.mark.parametrize("W,chain", [(12, "lp16"), (100, "lp16"), (100, "lp32")])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("fmt", [0, 1, 3])
def test_bluestein_width_behind_shift_and_lowpass(engine, oracle, fsk, fmt, order, W, chain):
    shift, out_len, lp = 280000, 32, CHAINS[chain]
    data = _data(fsk, fmt)
    n = len(data) // FMT_BYTES[fmt]
    L, R = _lens(n, lp)
    assert L == {("lp16", True): 4094, ("lp16", False): 2498, ("lp32", True): 2036, ("lp32", False): 1238}[(chain, fmt == 0)] and L >= W
    ch = _chain(oracle, data, fmt, shift, lp)
    p = _plan(engine, fmt, n, W, shift, lp, nco_order=order)
    name = p.kernel_name()
    assert f"nco {order}, RowGeo>" in name and name.endswith("| k_bluestein<fmt 0, nco 0>"), name
    for slice_ in (None, (7, R // 2)):
        what = f"rows composed W={W} fmt{fmt} shift {shift} nco {order} {chain} slice={slice_}"
        _no_real_tie(oracle, engine, fmt, n, W, out_len, slice_, shift, lp, what)
        rc, ref, offs = ch.take_fft(W, out_len, slice_, 1)
        assert rc == 0
        got = p.take_fft(data, out_len, slice_, 1)
        _bluestein_check(ch, ref, got, offs, W, what)
    p.close()


# ------------------------------------------------------------------ C: the 8 row-mode kernels with the second-order NCO

@pytest.mark.parametrize("chain", ["none", "lp16"])
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_row_mode_with_the_second_order_nco(engine, oracle, fsk, fmt, shift, chain):
    lp = CHAINS[chain]
    data = _data(fsk, fmt)
    n = len(data) // FMT_BYTES[fmt]
    L, R = _lens(n, lp)
    ch = _chain(oracle, data, fmt, shift, lp)
    rows = differing = 0
    for W, out_len in ((16, 33), (256, 32)):
        p = _plan(engine, fmt, n, W, shift, lp, nco_order=2)
        assert f"fmt {fmt}, nco 2, RowGeo>" in p.kernel_name(), p.kernel_name()
        slices = _slices(W, out_len, L, R)
        assert len(slices) >= 2
        for slice_ in slices:
            rc, ref, offs = ch.take_fft(W, out_len, slice_, 1)
            assert rc == 0
            got = p.take_fft(data, out_len, slice_, 1)
            rows += out_len
            differing += _nco_rule_rows(ref, got, offs, _stages(shift, lp), W, f"rows nco 2 fmt{fmt} shift {shift} {chain} W={W} slice={slice_}")
        p.close()
    record_observed(f"rows nco 2 behind shift {shift} fmt{fmt} {chain}", rows=rows, rows_differing=differing)


# ------------------------------------------------------------------ D: one plan, a moving slice

class _RowTab:
    """ensure_rowtab (quadrs_hip.hip) restated, to name the branch each call of the sequence takes: the rows' source range [lo, hi)
    needs table rows [lo / ROW, ceil((hi + ROW) / ROW)) — both callers add the guard row —; a table that covers them is KEPT, one
    whose capacity covers their number is REWRITTEN in place, any other is freed and GROWN to rows + rows / 8 + 16."""

    def __init__(self, ROW):
        self.ROW, self.row0, self.rows, self.cap = ROW, 0, 0, 0

    def ensure(self, lo, hi):
        r_lo, r_hi = lo // self.ROW, (hi + self.ROW + self.ROW - 1) // self.ROW
        if self.cap and r_lo >= self.row0 and r_hi <= self.row0 + self.rows:
            return "kept"
        rows = r_hi - r_lo
        branch = "rewritten"
        if rows > self.cap:
            self.cap, branch = rows + rows // 8 + 16, "grown"
        self.row0, self.rows = r_lo, rows
        return branch


MOVING = [("cf32 W=64", 0, 64, None), ("cs8 W=64 lp16", 1, 64, LP16), ("cf32 W=100", 0, 100, None), ("cs16 W=100", 3, 100, None)]


@pytest.mark.parametrize("case", MOVING, ids=[c[0] for c in MOVING])
def test_one_plan_a_moving_slice(engine, oracle, fsk, case):
    """The NCO row table of a rows plan (tabs_dev.main in row mode, rows of 512 / 1024 samples for cf32 / the integer formats;
    rows_tab512 under k_bluestein) outlives the call.  With R the sink samples a row may end at, the six slices take ensure_rowtab
    through: 1 (0.45 R, 0.50 R) the first table, a few rows, capacity rows + rows / 8 + 16 — 2 (0.46 R, 0.49 R) inside it: kept —
    3 (10, 0.03 R) below row0, fewer rows than the capacity: rewritten in place — 4 None, the whole sink, more rows than the
    capacity: freed and regrown — 5 slice 1 again, inside the large table: kept, and the rows are call 1's bit for bit — 6 a slice
    whose last row ends at the last admissible sample, past the rows of call 4 (whose last row starts a step before the sink's
    end): rewritten in place, up to the stream's last row plus the guard row.  _RowTab asserts that sequence from the rows' source
    ranges.  Odd calls hand over the whole stream as host bytes, even calls a fresh device tensor of exactly
    the rows' range: the pool workspaces (upload, rows, offsets) also shrink after they grew.  Every call is held to the oracle."""
    import torch
    _, fmt, W, lp = case
    shift, out_len = 280000, 32
    data = _data(fsk, fmt)
    bps = FMT_BYTES[fmt]
    n = len(data) // bps
    raw = np.frombuffer(data, dtype=np.uint8)
    L, R = _lens(n, lp)
    last = R - W - 2 * (out_len - 1)                       # step = 2 exactly: the last row sits at R - W
    a = (int(0.45 * R), int(0.50 * R))
    slices = [a, (int(0.46 * R), int(0.49 * R)), (10, int(0.03 * R)), None, a, (last, last + 2 * out_len)]
    blue = W & (W - 1) != 0
    tab = _RowTab(512 if blue or fmt == 0 else 1024)
    ch = _chain(oracle, data, fmt, shift, lp)
    p = _plan(engine, fmt, n, W, shift, lp, nco_order=0)
    assert ("k_bluestein" if blue else "RowGeo") in p.kernel_name() and "nco 1" in p.kernel_name(), p.kernel_name()
    branches, results = [], []
    rows = differing = 0
    for k, slice_ in enumerate(slices, 1):
        what = f"rows moving slice {case[0]} call {k} slice={slice_}"
        geo_offs, first, count = engine.rows_geometry(fmt, SR, n, W, out_len, slice_, 1, shift_hz=shift, lowpass=lp)
        branches.append(tab.ensure(first, first + count))
        rc, ref, offs = ch.take_fft(W, out_len, slice_, 1)
        assert rc == 0 and (offs == geo_offs).all(), what
        if blue:
            _no_real_tie(oracle, engine, fmt, n, W, out_len, slice_, shift, lp, what)
        if k % 2:
            got = p.take_fft(data, out_len, slice_, 1)
        else:
            slab = torch.from_numpy(raw[first * bps:(first + count) * bps].copy()).cuda()
            got = p.take_fft(slab, out_len, slice_, 1, src_first=first)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
        if blue:
            _bluestein_check(ch, ref, got, offs, W, what)
        else:
            rows += out_len
            differing += _nco_rule_rows(ref, got, offs, _stages(shift, lp), W, what)
        results.append(got)
    assert int(offs[-1]) + W == R and first + count == R * (lp[1] if lp else 1) + (lp[2] if lp else 0)
    assert branches == ["grown", "kept", "rewritten", "grown", "kept", "rewritten"], branches
    assert bits_equal(results[0], results[4])
    if not blue:
        record_observed(f"rows moving slice {case[0]}", rows=rows, rows_differing=differing)
    p.close()


# ------------------------------------------------------------------ E: rows deep in a stream

@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("case", DEEP_CASES, ids=[c[0] for c in DEEP_CASES])
def test_rows_deep_in_a_stream(engine, oracle, case, shift):
    """absolute sample indices past 2^32 (cs8) / next to 2^34 (cf32) in the loaders' byte offsets, the NCO row index, row_offsets and
    the NCO itself, whose second-order form the plan selects on its own here"""
    import torch
    name, fmt, N, base, W, lp, (s, e) = case
    D = lp[1] if lp else 1
    bps = FMT_BYTES[fmt]
    rng = np.random.default_rng(W * 11 + fmt)
    if fmt == 0:
        raw = (rng.standard_normal((DEEP_SPAN, 2)) * 0.03).astype(np.float32).view(np.uint8).reshape(-1)
    else:
        raw = rng.integers(0, 256, DEEP_SPAN * bps, dtype=np.uint8)
    # the reference: the slab as a stream of its own whose shift uses the multipliers of samples base, base + 1, ...
    ratio = oracle.shift_ratio(shift, SR)
    idx = np.arange(DEEP_SPAN, dtype=np.uint64)
    mult = oracle.shift_multipliers(ratio, [base + i for i in range(DEEP_SPAN)])
    ch = oracle.Chain.from_bytes(raw, fmt, SR).shift(shift)
    ch.override_shift(0, idx, mult[:, 0], mult[:, 1])
    if lp:
        ch = ch.lowpass(*lp)
    rc, ref, loc = ch.take_fft(W, DEEP_OUT_LEN, (s, e), 1)
    assert rc == 0
    q = base // D
    slice_ = (q + s, q + e)
    p = _plan(engine, fmt, N, W, shift, lp, nco_order=0)
    assert "nco 2" in p.kernel_name(), p.kernel_name()
    offs, first, count = engine.rows_geometry(fmt, SR, N, W, DEEP_OUT_LEN, slice_, 1, shift_hz=shift, lowpass=lp)
    assert (offs == np.uint64(q) + loc).all() and base <= first and first + count <= base + DEEP_SPAN
    slab = raw[(first - base) * bps:(first - base + count) * bps].copy()
    got = p.take_fft(slab, DEEP_OUT_LEN, slice_, 1, src_first=first)
    dev = p.take_fft(torch.from_numpy(slab).cuda(), DEEP_OUT_LEN, slice_, 1, src_first=first)
    torch.cuda.synchronize()
    assert bits_equal(got, dev.cpu().numpy()), name
    what = f"rows deep {name} shift {shift}"
    if W & (W - 1):
        ambiguous, ties = real_ties(ratio, first, count)
        assert not ties, (what, ties[:4])
        _bluestein_check(ch, ref, got, loc, W, what)
    else:
        differing = _nco_rule_rows(ref, got, offs, _stages(shift, lp), W, what)
        record_observed(what, rows=DEEP_OUT_LEN, rows_differing=differing,
                        rows_reading_an_ambiguous_component=ambiguous_windows((_stages(shift, lp), W, 1, SR), offs.astype(np.int64)))
    p.close()
