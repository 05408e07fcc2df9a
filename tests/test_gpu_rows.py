"""QD_EPI_ROWS_F32: take_fft's rows (src/ffts.rs:18-85) behind a fused chain  from -> [shift] -> [lowpass], against the oracle's
Chain.take_fft over the same chain.

  * power-of-two widths without a shift: bit for bit;
  * with a shift: the NCO near-tie rule of DESIGN.md section 5 (assert_explained), row by row — row i of the sink is the window
    that starts at sample offs[i], i.e. window offs[i] of a stride-1 sink;
  * every other width (Bluestein, f64): the bound of test_take_fft_any_width_against_f64_dft, 2 ulp_f32 of the reference norm
    plus 1e-12 of the row's l1 norm, also behind a lowpass (whose read_at blocks are bit-exact) and behind a shift.

Streams: the committed 65 536-sample head of the FSK recording (cf32) and 40 000 seeded samples of the integer formats."""
import numpy as np
import pytest

from test_gpu_footprint import FootprintRun, framed, framed_out
from test_gpu_parity import assert_explained, record_observed
from test_gpu_robustness import _synth_bytes
from util import FMT_BYTES, GUARD_BYTE, POISON_WORDS, bits_equal, real_ties

pytestmark = pytest.mark.gpu

SR = 21_000_000
N_INT = 40_000
LP16, LP32 = (2_000_000, 16, 40), (200_000, 32, 400)
CHAINS = {"none": None, "lp16": LP16, "lp32": LP32}
SHAPES = [(4, 9), (16, 33), (64, 32), (256, 32), (1024, 8)]
LDS_MAX = 160 * 1024


def _data(fsk, fmt):
    return fsk if fmt == 0 else _synth_bytes(fmt, N_INT, 7700 + fmt)


def _chain(oracle, data, fmt, shift=None, lp=None):
    ch = oracle.Chain.from_bytes(data, fmt, SR)
    if shift is not None:
        ch = ch.shift(shift)
    if lp is not None:
        ch = ch.lowpass(*lp)
    return ch


def _lens(n, lp):
    """(len() the sink reports, number of sink samples a row may end at)"""
    if lp is None:
        return n, n
    return 1 + (n - lp[2]) // lp[1], (n - lp[2]) // lp[1]


def _row_fits_lds(W, lp):
    """a 1024-point row behind the /32, 400-tap lowpass reads 33 168 samples = 259 KiB: past the 160 KiB LDS tile, the header's
    QD_ERR_UNSUPPORTED (asserted in test_refusals); everything else of the table fits"""
    D, T = (lp[1], lp[2]) if lp else (1, 0)
    return (W * D + T) * 8 <= LDS_MAX - 24 * 1024


def _slices(W, out_len, L, R):
    """None; an interior slice with step < W (overlapping rows); one with step >> W where the stream is long enough"""
    out = [None]
    step = max(1, W // 4)
    s = 7
    if s + step * out_len + 3 + W <= R:
        out.append((s, s + step * out_len + 3))          # (+ 3: visible > output_len also where step is 1)
    far = 3 * W + 1
    if 5 + far * out_len + W <= R and 5 + far * out_len < L:
        out.append((5, 5 + far * out_len))
    return out


def _plan(engine, fmt, n, W, shift=None, lp=None, **kw):
    return engine.Plan(fmt, SR, n, shift_hz=shift, lowpass=lp, width=W, stride=1, epilogue=engine.EPI_ROWS_F32, **kw)


def _cases(W_list, fmt, n, lp):
    L, R = _lens(n, lp)
    for W, out_len in W_list:
        if not _row_fits_lds(W, lp) or L < W or L - W <= out_len:
            continue
        for slice_ in _slices(W, out_len, L, R):
            for windowing in (0, 1):
                yield W, out_len, slice_, windowing


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_power_of_two_rows_bit_for_bit(engine, oracle, fsk, fmt, chain):
    lp = CHAINS[chain]
    data = _data(fsk, fmt)
    n = len(data) // FMT_BYTES[fmt]
    ch = _chain(oracle, data, fmt, None, lp)
    seen = 0
    plans = {}
    for W, out_len, slice_, windowing in _cases(SHAPES, fmt, n, lp):
        p = plans.get(W) or plans.setdefault(W, _plan(engine, fmt, n, W, None, lp))
        assert p.info.n_windows == 0 and p.info.out_bytes_per_window == 4 * W
        assert p.info.raw_per_window == W * (lp[1] if lp else 1) + (lp[2] if lp else 0)
        rc, ref, _ = ch.take_fft(W, out_len, slice_, windowing)
        assert rc == 0, (W, out_len, slice_)
        got = p.take_fft(data, out_len, slice_, windowing)
        assert bits_equal(ref, got), (fmt, chain, W, out_len, slice_, windowing, int((ref.view(np.uint32) != got.view(np.uint32)).sum()))
        seen += 1
    assert seen >= {"none": 24, "lp16": 20, "lp32": 12}[chain], seen
    for p in plans.values():
        p.close()


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("shift", [280000, -1234567])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_power_of_two_rows_behind_a_shift(engine, oracle, fsk, fmt, shift, chain):
    lp = CHAINS[chain]
    data = _data(fsk, fmt)
    n = len(data) // FMT_BYTES[fmt]
    ch = _chain(oracle, data, fmt, shift, lp)
    stages = [("shift", shift)] + ([("lowpass", lp)] if lp else [])
    rows = differing = 0
    for W, out_len, slice_, windowing in _cases([(16, 33), (64, 32), (256, 32)], fmt, n, lp):
        if windowing == 0 and slice_ is not None:
            continue
        p = _plan(engine, fmt, n, W, shift, lp)
        rc, ref, offs = ch.take_fft(W, out_len, slice_, windowing)
        assert rc == 0
        got = p.take_fft(data, out_len, slice_, windowing)
        p.close()
        rows += out_len
        for i in np.nonzero((ref.view(np.uint32) != got.view(np.uint32)).any(axis=1))[0]:
            differing += 1
            assert_explained(ref[i:i + 1], got[i:i + 1], ((stages, W, 1, SR), int(offs[i])), f"rows fmt{fmt} shift {shift} {chain} W={W} row {i}")
    record_observed(f"rows behind shift {shift} fmt{fmt} {chain}", rows=rows, rows_differing=differing)
    assert rows > 0


def _bluestein_check(ch, ref, got, offs, W, what):
    worst_ulp, exact = 0.0, 0
    for r in range(ref.shape[0]):
        nread, seg = ch.read_at(int(offs[r]), W)
        assert nread == W
        l1 = float(np.abs(seg.astype(np.float64)).sum())
        err = np.abs(got[r].astype(np.float64) - ref[r].astype(np.float64))
        allowed = 2.0 * np.spacing(ref[r]).astype(np.float64) + 1e-12 * l1
        assert (err <= allowed).all(), (what, r, float((err / allowed).max()))
        worst_ulp = max(worst_ulp, float((err / np.spacing(ref[r]).astype(np.float64)).max()))
        exact += int((got[r].view(np.uint32) == ref[r].view(np.uint32)).sum())
    record_observed(what, rows=int(ref.shape[0]), worst_ulp=worst_ulp, exact_fraction=exact / ref.size)


@pytest.mark.parametrize("chain", ["none", "lp16"])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("W,out_len", [(100, 48), (12, 48), (4095, 4)])
def test_bluestein_rows(engine, oracle, fsk, W, out_len, fmt, chain):
    """widths that are not powers of two.  4095 behind the /16 lowpass is not a case: the sink holds 4094 (cf32) / 2498 (cs8)
    samples, fewer than one row."""
    lp = CHAINS[chain]
    data = _data(fsk, fmt)
    n = len(data) // FMT_BYTES[fmt]
    if lp is not None and W == 4095:
        assert _lens(n, lp)[0] < W
        with pytest.raises(engine.QuadrsError) as e:
            _plan(engine, fmt, n, W, None, lp)
        assert e.value.code == engine._ffi.ERR_PANIC          # len < width (src/ffts.rs:29)
        return
    ch = _chain(oracle, data, fmt, None, lp)
    p = _plan(engine, fmt, n, W, None, lp)
    for windowing in (0, 1):
        for slice_ in (None, (10, 2000)):
            rc, ref, offs = ch.take_fft(W, out_len, slice_, windowing)
            assert rc == 0
            got = p.take_fft(data, out_len, slice_, windowing)
            _bluestein_check(ch, ref, got, offs, W, f"plan rows W={W} fmt{fmt} {chain} windowing={windowing} slice={slice_}")
    p.close()


def test_bluestein_rows_behind_a_shift(engine, oracle, fsk):
    """cf32, shift 280000, W = 100: the same bound with no row excluded, on a condition asserted first: the source span of the rows
    holds no REAL tie, i.e. no multiplier component whose two f32 candidates (util.nco_candidates) lie more than 1e-13 apart —
    such a tie moves a bin by at most a tenth of the bound's l1 term.  At 280000 / 21 MHz the period is 75 samples, so ambiguous
    components do occur, the sin of every 75th sample (874 in [0, 65536)): zero crossings, whose candidates are 1e-19 ... 1e-14
    apart."""
    n = len(fsk) // 8
    _, first, count = engine.rows_geometry(0, SR, n, 100, 48, None, 1, shift_hz=280000)
    ambiguous, ties = real_ties(oracle.shift_ratio(280000, SR), first, count)
    assert ambiguous > 0 and not ties, (ambiguous, ties[:4])
    ch = _chain(oracle, fsk, 0, 280000, None)
    p = _plan(engine, 0, n, 100, 280000, None)
    rc, ref, offs = ch.take_fft(100, 48, None, 1)
    assert rc == 0
    got = p.take_fft(fsk, 48, None, 1)
    _bluestein_check(ch, ref, got, offs, 100, "plan rows W=100 cf32 shift 280000")
    p.close()


def test_equivalences(engine, oracle, fsk):
    n = len(fsk) // 8
    x = np.frombuffer(fsk, dtype=np.float32).reshape(-1, 2)
    # a cf32 plan without stages is qd_take_fft
    for W, out_len in ((64, 32), (100, 48), (4, 9)):
        p = _plan(engine, 0, n, W)
        for windowing in (0, 1):
            for slice_ in (None, (10, 2000)):
                a = engine.take_fft(x, W, out_len, slice_, windowing)
                b = p.take_fft(fsk, out_len, slice_, windowing)
                assert bits_equal(a, b), (W, windowing, slice_)
        p.close()
    # rows at i S under a rectangular window are the norms sink's first windows: step = S exactly
    W, S, nr = 64, 16, 40
    for lp in (None, LP16):
        pr = _plan(engine, 0, n, W, None, lp)
        pn = engine.Plan(0, SR, n, lowpass=lp, width=W, stride=S, epilogue=engine.EPI_NORMS_F32)
        rows = pr.take_fft(fsk, nr, (0, nr * S), 0)
        norms = pn.run_host(fsk, 0, nr)
        assert bits_equal(rows, norms), lp
        pr.close(); pn.close()


@pytest.mark.parametrize("fmt,lp", [(1, None), (0, LP16)])
def test_slabs(engine, oracle, fsk, fmt, lp):
    import torch
    data = _data(fsk, fmt)
    bps = FMT_BYTES[fmt]
    n = len(data) // bps
    W, out_len, slice_ = 64, 32, (10, 2000)
    p = _plan(engine, fmt, n, W, None, lp)
    whole = p.take_fft(data, out_len, slice_, 1)
    rc, ref, _ = _chain(oracle, data, fmt, None, lp).take_fft(W, out_len, slice_, 1)
    assert rc == 0 and bits_equal(ref, whole)
    _, first, count = engine.rows_geometry(fmt, SR, n, W, out_len, slice_, 1, lowpass=lp)
    raw = np.frombuffer(data, dtype=np.uint8)
    # exactly the rows' range, on the device
    slab = torch.from_numpy(raw[first * bps:(first + count) * bps].copy()).cuda()
    got = p.take_fft(slab, out_len, slice_, 1, src_first=first)
    torch.cuda.synchronize()
    assert bits_equal(whole, got.cpu().numpy())
    # one sample short: the last row is not inside the slab
    short = torch.from_numpy(raw[first * bps:(first + count - 1) * bps].copy()).cuda()
    with pytest.raises(engine.QuadrsError) as e:
        p.take_fft(short, out_len, slice_, 1, src_first=first)
    assert e.value.code == engine._ffi.ERR_SHORT
    # ... and on the host
    with pytest.raises(engine.QuadrsError) as e:
        p.take_fft(raw[first * bps:(first + count - 1) * bps].copy(), out_len, slice_, 1, src_first=first)
    assert e.value.code == engine._ffi.ERR_SHORT
    # a slab whose first sample is off the load-vector grid: an odd sample index at an address one sample into an allocation
    f2 = first - 1
    assert f2 % 2 == 1 and f2 >= 1
    big = torch.from_numpy(raw[(f2 - 1) * bps:(first + count) * bps].copy()).cuda()
    odd = big[bps:]
    assert odd.data_ptr() % (2 * bps) != 0
    got = p.take_fft(odd, out_len, slice_, 1, src_first=f2)
    torch.cuda.synchronize()
    assert bits_equal(whole, got.cpu().numpy())
    p.close()


@pytest.mark.parametrize("W,lp", [(64, LP16), (100, LP16)])
def test_footprint(engine, oracle, fsk, W, lp):
    """source slab and output between poisoned frames and 0xA5 guards: no guard byte changes, the source is not written, and the
    rows are those of the unframed run (the chain kernel in row mode; the Bluestein kernel over its read_at blocks)"""
    n = len(fsk) // 8
    out_len, slice_ = 32, (10, 2000)
    p = _plan(engine, 0, n, W, None, lp)
    plain = p.take_fft(fsk, out_len, slice_, 1)
    _, first, count = engine.rows_geometry(0, SR, n, W, out_len, slice_, 1, lowpass=lp)
    raw = np.frombuffer(fsk, dtype=np.uint8)
    for which in range(len(POISON_WORDS)):
        src = framed("device", 0, which, 1 << 20, raw[first * 8:(first + count) * 8], 1 << 20, engine)
        out = framed_out("device", 64 << 10, out_len * W * 4, engine)
        p.take_fft(src.body, out_len, slice_, 1, src_first=first, out=out.body)
        run = FootprintRun(out, src)
        assert (run.front == GUARD_BYTE).all() and (run.back == GUARD_BYTE).all(), (W, which)
        assert (run.src_now == run.src_uploaded).all()
        assert bits_equal(plain, run.payload.view(np.float32).reshape(out_len, W)), (W, which)
        src.close(); out.close()
    # a host slab of exactly the rows' range gives the same rows
    rows = p.take_fft(raw[first * 8:(first + count) * 8].copy(), out_len, slice_, 1, src_first=first)
    assert bits_equal(plain, rows)
    p.close()


def _code(engine, fn):
    try:
        fn()
    except engine.QuadrsError as e:
        return e.code
    return 0


def test_refusals(engine, fsk):
    import ctypes as C
    E = engine._ffi
    n = len(fsk) // 8
    p = _plan(engine, 0, n, 64, None, LP16)
    out = np.zeros((4, 64), dtype=np.float32)
    buf = np.frombuffer(fsk, dtype=np.uint8)
    rc = E.lib().qd_plan_run(p._h, buf.ctypes.data_as(C.c_void_p), E.MEM_HOST, 0, n, 0, 1, out.ctypes.data_as(C.c_void_p), E.MEM_HOST, None)
    assert rc == E.ERR_INVALID and b"qd_plan_take_fft" in E.lib().qd_last_error() and b"qd_rows_geometry" in E.lib().qd_last_error()
    assert _code(engine, lambda: p.src_range(0, 1)) == E.ERR_INVALID
    assert _code(engine, p.complete_windows) == E.ERR_INVALID
    assert _code(engine, lambda: p.run_sharded_host(fsk)) == E.ERR_INVALID
    p.close()
    # a cascade behind this sink
    casc = [("lowpass", LP16), ("lowpass", (100_000, 4, 40))]
    assert _code(engine, lambda: engine.Plan(0, SR, n, stages=casc, width=64, epilogue=engine.EPI_ROWS_F32)) == E.ERR_UNSUPPORTED
    # ... while a [shift] [lowpass] list is the one-stage plan
    q = engine.Plan(0, SR, n, stages=[("shift", 280000), ("lowpass", LP16)], width=64, epilogue=engine.EPI_ROWS_F32)
    one = _plan(engine, 0, n, 64, 280000, LP16)
    assert bits_equal(q.take_fft(fsk, 8, None, 1), one.take_fft(fsk, 8, None, 1))
    q.close(); one.close()
    # widths that are not built, rows larger than the LDS tile
    assert _code(engine, lambda: _plan(engine, 0, n, 5000)) == E.ERR_UNSUPPORTED
    assert _code(engine, lambda: _plan(engine, 0, n, 1024, None, (200_000, 64, 400))) == E.ERR_PANIC     # 1018 sink samples < 1024 (src/ffts.rs:29)
    big = 200_000                                             # a longer (described, never read) stream: the row itself is refused
    assert _code(engine, lambda: _plan(engine, 0, big, 1024, None, (200_000, 64, 400))) == E.ERR_UNSUPPORTED
    assert _code(engine, lambda: _plan(engine, 0, big, 1024, None, LP32)) == E.ERR_UNSUPPORTED
    # output_len 0 is nothing to do
    p = _plan(engine, 0, n, 64)
    assert p.take_fft(fsk, 0, (10, 2000), 1).shape == (0, 64)
    p.close()
