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


# ------------------------------------------------------------------ rows deep in a stream (tests/test_gpu_rows_paths.py, section E)
#
# A long stream is described, a slab of DEEP_SPAN samples at `base` exists.  (name, fmt, n_samples, base, W, lowpass, local slice):
# the slice is in the sink's samples of the slab; the plan is handed (base / D + s, base / D + e).

LP16 = (2_000_000, 16, 40)
DEEP_SPAN = 70_000
DEEP_OUT_LEN = 24
_BASE_CF32 = (1 << 34) - (1 << 20)
_BASE_CS8 = ((1 << 32) + 777_777) // 32 * 32
DEEP_CASES = [
    ("cf32 W=64", 0, 1 << 34, _BASE_CF32, 64, None, (300, 6300)),
    ("cf32 W=256 lp16", 0, 1 << 34, _BASE_CF32, 256, LP16, (40, 3500)),
    ("cf32 W=100", 0, 1 << 34, _BASE_CF32, 100, None, (300, 6300)),
    ("cs8 W=64", 1, 1 << 33, _BASE_CS8, 64, None, (300, 6300)),
    ("cs8 W=100 lp16", 1, 1 << 33, _BASE_CS8, 100, LP16, (40, 3500)),
]


@pytest.mark.parametrize("case", DEEP_CASES, ids=[c[0] for c in DEEP_CASES])
@pytest.mark.parametrize("shift", [280000, -1234567])
def test_deep_slices_are_the_local_ones_moved_by_base(engine, oracle, case, shift):
    """the translation the deep GPU reference rests on: rows of the slice (base / D + s, base / D + e) of the long stream sit at
    base / D + the rows of (s, e) of a DEEP_SPAN-sample stream (which are the oracle's), and read [min off D, max off D + W D + T)"""
    _, fmt, N, base, W, lp, (s, e) = case
    D, T = (lp[1], lp[2]) if lp else (1, 0)
    assert base % D == 0 and base + DEEP_SPAN <= N
    q = base // D
    offs, first, count = engine.rows_geometry(fmt, SR, N, W, DEEP_OUT_LEN, (q + s, q + e), 1, shift_hz=shift, lowpass=lp)
    loc, lfirst, lcount = engine.rows_geometry(fmt, SR, DEEP_SPAN, W, DEEP_OUT_LEN, (s, e), 1, shift_hz=shift, lowpass=lp)
    assert (offs == np.uint64(q) + loc).all(), (offs, loc)
    assert first == int(offs.min()) * D == base + lfirst
    assert count == int(offs.max()) * D + W * D + T - first == lcount
    assert base <= first and first + count <= base + DEEP_SPAN and int(offs.max()) >= 1 << 28
    ch = oracle.Chain.from_bytes(bytes(DEEP_SPAN * 2), oracle.FMT_CS8, SR).shift(shift)
    if lp:
        ch = ch.lowpass(*lp)
    rc, _, ref_offs = ch.take_fft(W, DEEP_OUT_LEN, (s, e), 1)
    assert rc == 0 and (ref_offs == loc).all()


# ------------------------------------------------------------------ the NCO rule on rows: a control that it bites

def _unexplained_rows(stages, W, ref, got, offs):
    """the rows the NCO rule does not explain, applied row by row as the GPU tests apply it: row i is window offs[i] of a stride-1 sink"""
    from util import explain_check
    return [i for i in range(ref.shape[0]) if explain_check((stages, W, 1, SR), ref[i:i + 1], got[i:i + 1], int(offs[i]))]


def test_row_rule_catches_one_ulp_of_one_multiplier(oracle, fsk):
    """Two oracle chains over the same 8192 samples behind a shift of 321334 Hz, one of them with ONE multiplier component moved (the
    override hook).  At that frequency sample 3426's sin (0.4632207...) lies within NCO_ABS_ERR of an f32 rounding boundary and
    nothing else in [1, 8192) is ambiguous.  A cos moved by one f32 ulp at sample 3700 must leave exactly the rows that read sample
    3700 unexplained; sample 3426's sin moved to its other candidate changes its rows too, and the rule explains them."""
    from util import ambiguous_components
    f, W, out_len, slice_ = 321334, 64, 32, (3000, 4000)
    data = fsk[:8192 * 8]
    ratio = oracle.shift_ratio(f, SR)
    amb = ambiguous_components(ratio, 1, 8192)
    assert [(n, comp) for n, comp, _ in amb] == [(3426, 1)] and len(amb[0][2]) == 2
    stages = [("shift", f)]
    rc, ref, offs = oracle.Chain.from_bytes(data, oracle.FMT_CF32, SR).shift(f).take_fft(W, out_len, slice_, 1)
    assert rc == 0

    def moved(n, comp, value):
        c, s = oracle.shift_multipliers(ratio, [n])[0]
        ch = oracle.Chain.from_bytes(data, oracle.FMT_CF32, SR).shift(f)
        ch.override_shift(0, [n], [value if comp == 0 else c], [value if comp == 1 else s])
        rc, rows, o = ch.take_fft(W, out_len, slice_, 1)
        assert rc == 0 and (o == offs).all()
        reading = [i for i in range(out_len) if int(offs[i]) <= n < int(offs[i]) + W]
        differing = [i for i in range(out_len) if rows[i].tobytes() != ref[i].tobytes()]
        # (a row that reads the sample under the window's edge may round the change away: Blackman-Harris is 6e-5 there)
        assert len(reading) == 2 and differing and set(differing) <= set(reading), (n, reading, differing)
        return rows, differing

    c, _ = oracle.shift_multipliers(ratio, [3700])[0]
    rows, differing = moved(3700, 0, np.nextafter(np.float32(c), np.float32(2)))
    assert differing == [21, 22] and _unexplained_rows(stages, W, ref, rows, offs) == differing
    _, s = oracle.shift_multipliers(ratio, [3426])[0]
    other = [v for v in amb[0][2] if v != np.float32(s)]
    assert len(other) == 1
    rows, differing = moved(3426, 1, other[0])
    assert _unexplained_rows(stages, W, ref, rows, offs) == []


def test_real_ties_of_the_two_test_shifts(oracle):
    """util.real_ties over [0, 65536) at 21 MHz: 874 ambiguous components at shift 280000 (period 75 samples: the sin of every 75th
    sample is a zero crossing) and 1 at -1234567, none of them a real tie; a component whose candidates are two neighbouring f32
    values of ordinary size is one"""
    from util import real_ties
    assert real_ties(oracle.shift_ratio(280000, SR), 0, 65536) == (874, [])
    assert real_ties(oracle.shift_ratio(-1234567, SR), 0, 65536) == (1, [])
    n_amb, ties = real_ties(oracle.shift_ratio(321334, SR), 1, 8191)
    assert n_amb == 1 and [(t[0], t[1]) for t in ties] == [(3426, 1)] and ties[0][3] - ties[0][2] > 1e-8


def test_plan_calls_are_declared(engine):
    """the binding resolves the two new entry points (no device needed)"""
    L = engine._ffi.lib()
    assert L.qd_rows_geometry and L.qd_plan_take_fft and engine.EPI_ROWS_F32 == 5
