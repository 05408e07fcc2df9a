"""qd_rows_geometry (host arithmetic, no device) against the oracle's take_fft: the row offsets `offs` element for element, the
source range the rows read, and the status codes of src/ffts.rs:27-48 plus the failing read_exact_at of a row whose source span
does not fit the stream.  Streams: the committed 65 536-sample head of the FSK recording (cf32, 21 Msps)."""
import numpy as np
import pytest

SR = 21_000_000
CHAINS = {
    "none": dict(),
    "shift": dict(shift_hz=280000),
    "lp16": dict(lowpass=(2_000_000, 16, 40)),
    "shift_lp32": dict(shift_hz=280000, lowpass=(200_000, 32, 400)),
}
SHAPES = [(4, 7), (64, 32), (256, 32), (100, 48)]


def _oracle_chain(oracle, data, kw):
    ch = oracle.Chain.from_bytes(data, oracle.FMT_CF32, SR)
    if "shift_hz" in kw:
        ch = ch.shift(kw["shift_hz"])
    if "lowpass" in kw:
        ch = ch.lowpass(*kw["lowpass"])
    return ch


def _DT(kw):
    return (kw["lowpass"][1], kw["lowpass"][2]) if "lowpass" in kw else (1, 0)


def _sink_len(n, kw):
    D, T = _DT(kw)
    return 1 + (n - T) // D if T else n          # LowPass::len, src/filter.rs:47


def _stream_for_exact_end(fsk, kw):
    """the longest head of the recording whose sink has a last sample with a whole source span: (n - T) a multiple of D"""
    D, T = _DT(kw)
    n = len(fsk) // 8
    n -= (n - T) % D
    return fsk[:n * 8], n


def _last_row_at_stream_end(n, kw, W, out_len):
    """a slice whose LAST row's source span ends exactly at the last source sample: off_last = (n - T) / D - W.  step = 2 exactly,
    so round(step i) = 2 i and the last row sits at start + 2 (out_len - 1)"""
    D, T = _DT(kw)
    assert (n - T) % D == 0
    target = (n - T) // D - W
    start = target - 2 * (out_len - 1)
    return (start, start + 2 * out_len)


def _code(engine, fn):
    try:
        fn()
    except engine.QuadrsError as e:
        return e.code
    return 0


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("W,out_len", SHAPES)
def test_offsets_and_source_range(engine, oracle, fsk, name, W, out_len):
    kw = CHAINS[name]
    fsk, n = _stream_for_exact_end(fsk, kw)
    D, T = _DT(kw)
    ch = _oracle_chain(oracle, fsk, kw)
    for slice_ in (None, (10, 2000), _last_row_at_stream_end(n, kw, W, out_len)):
        for windowing in (0, 1):
            rc, _, ref_offs = ch.take_fft(W, out_len, slice_, windowing)
            if rc != 0:
                # (10, 2000) with 100- and 256-point rows on the 2036 samples behind the /32 lowpass: the last rows reach past the stream, the
                # reference's read_exact_at fails there (src/ffts.rs:62) and so does ours
                last = slice_[0] + int(np.floor((slice_[1] - slice_[0]) / out_len * (out_len - 1) + 0.5))
                assert slice_ == (10, 2000) and name == "shift_lp32" and (last + W) * D + T > n, (slice_, rc)
                assert _code(engine, lambda: engine.rows_geometry(engine.FMT_CF32, SR, n, W, out_len, slice_, windowing, **kw)) == 3
                continue
            offs, first, count = engine.rows_geometry(engine.FMT_CF32, SR, n, W, out_len, slice_, windowing, **kw)
            assert offs.dtype == np.uint64 and (offs == ref_offs).all(), (slice_, offs, ref_offs)
            lo = int(ref_offs.min()) * D
            hi = int(ref_offs.max()) * D + W * D + T
            assert (first, count) == (lo, hi - lo), (slice_, first, count, lo, hi)
    s, e = _last_row_at_stream_end(n, kw, W, out_len)
    _, first, count = engine.rows_geometry(engine.FMT_CF32, SR, n, W, out_len, (s, e), 1, **kw)
    assert first + count == n


@pytest.mark.parametrize("name", list(CHAINS))
def test_status_codes(engine, oracle, fsk, name):
    kw = CHAINS[name]
    n = len(fsk) // 8
    ch = _oracle_chain(oracle, fsk, kw)
    L = _sink_len(n, kw)
    W, out_len = 64, 32
    cases = {
        "end <= start": ((500, 500), 2),
        "end < start": ((500, 100), 2),
        "end == len": ((10, L), 2),
        "end > len": ((10, L + 5), 2),
        "visible == output_len": ((100, 100 + out_len), 1),
        "visible < output_len": ((100, 110), 1),
    }
    for what, (slice_, want) in cases.items():
        rc, _, _ = ch.take_fft(W, out_len, slice_, 1)
        assert rc == want, (what, rc)
        got = _code(engine, lambda: engine.rows_geometry(engine.FMT_CF32, SR, n, W, out_len, slice_, 1, **kw))
        assert got == want, (what, got, engine._ffi.lib().qd_last_error())


@pytest.mark.parametrize("name", list(CHAINS))
def test_stream_shorter_than_the_width(engine, oracle, fsk, name):
    """len < W: `len - width` underflows without a slice (src/ffts.rs:29)"""
    kw = CHAINS[name]
    D, T = _DT(kw)
    n = T + 10 * D                               # a sink of 11 samples
    data = fsk[:n * 8]
    rc, _, _ = _oracle_chain(oracle, data, kw).take_fft(64, 4, None, 1)
    assert rc == 2
    assert _code(engine, lambda: engine.rows_geometry(engine.FMT_CF32, SR, n, 64, 4, None, 1, **kw)) == 2


@pytest.mark.parametrize("name", ["lp16", "shift_lp32"])
def test_last_row_cannot_be_read_in_full(engine, oracle, fsk, name):
    """LowPass::len over-reports by one (src/filter.rs:45-48): the slice (0, len - 1) passes both asserts, and with a width that
    reaches the sink's last sample the last row's read_exact_at comes back short — the oracle's rc is non-zero, ours 3."""
    kw = CHAINS[name]
    n = len(fsk) // 8
    L = _sink_len(n, kw)
    W, out_len = 64, 8
    # step = 2 exactly: the last row sits at start + 2 (out_len - 1) = L - W, whose span ends past the stream
    start = L - W - 2 * (out_len - 1)
    found = (start, start + 2 * out_len)
    assert found[1] <= L - 1
    rc, _, _ = _oracle_chain(oracle, fsk, kw).take_fft(W, out_len, found, 1)
    assert rc != 0, found
    got = _code(engine, lambda: engine.rows_geometry(engine.FMT_CF32, SR, n, W, out_len, found, 1, **kw))
    assert got == 3, (found, got)
    assert b"row 7" in engine._ffi.lib().qd_last_error()
    # one decimated sample earlier the same rows read in full, in both
    ok = (found[0] - 1, found[1] - 1) if found[0] else None
    if ok:
        rc, _, ref_offs = _oracle_chain(oracle, fsk, kw).take_fft(W, out_len, ok, 1)
        offs, _, _ = engine.rows_geometry(engine.FMT_CF32, SR, n, W, out_len, ok, 1, **kw)
        assert rc == 0 and (offs == ref_offs).all()


def test_plan_calls_are_declared(engine):
    """the binding resolves the two new entry points (no device needed)"""
    L = engine._ffi.lib()
    assert L.qd_rows_geometry and L.qd_plan_take_fft and engine.EPI_ROWS_F32 == 5
