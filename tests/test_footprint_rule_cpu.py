"""The footprint checker's own machinery on the CPU (no GPU): a numpy model of a one-stage FIR chain run through
util.footprint_violations with the frames and guards the GPU tests use.  The clean model passes; mutated to read one sample
past its slab, to skip its last window, or to write one element past its payload, each mutation is reported (and as what)."""
import numpy as np
import pytest

from util import (GUARD_BYTE, POISON_WORDS, FootprintRun, Framed, footprint_violations, framed, framed_out, poison)

W, D, T = 16, 4, 12                   # windows side by side: window w reads samples [w W D, w W D + W D + T), writes W f32 norms
TAPS = (np.hanning(T + 2)[1:-1] / 5).astype(np.float32)


def _stream(n, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * 0.1).astype(np.float32)


def _window(x):
    """one window of the model from its W D + T samples (x: complex64)"""
    y = np.array([(x[k * D:k * D + T] * TAPS).sum() for k in range(W)])
    return np.abs(np.fft.fft(y)).astype(np.float32)


def _src_range(w0, n):
    return w0 * W * D, (n - 1) * W * D + W * D + T


def _model(buf, slab_at, out, out_at, n, over_read=False, skip_last=False, over_write=False):
    """the 'kernel': reads the whole buffer it was given through a pointer to the slab, like a device kernel could"""
    x = buf.view(np.float32).reshape(-1, 2)
    x = x[:, 0] + 1j * x[:, 1]
    s0 = slab_at // 8
    o = out.view(np.float32)
    for w in range(n - (1 if skip_last else 0)):
        seg = x[s0 + w * W * D:s0 + w * W * D + W * D + T].copy()
        if over_read and w == n - 1:
            seg[(W - 1) * D + T - 1] += x[s0 + w * W * D + W * D + T]     # the sample behind the slab, into the last tap's input
        o[out_at // 4 + w * W:out_at // 4 + (w + 1) * W] = _window(seg)
    if over_write:
        o[out_at // 4 + n * W] = 0.0


def _run(w0, n, **mutation):
    data = _stream(40 * W * D + T)
    first, count = _src_range(w0, n)
    z = data[:, 0] + 1j * data[:, 1]
    ref = np.stack([_window(z[(w0 + w) * W * D:(w0 + w) * W * D + W * D + T]) for w in range(n)])
    runs = []
    for which in range(len(POISON_WORDS)):
        src = framed("host", 0, which, 4096, data[first:first + count], 4096)
        out = framed_out("host", 4096, n * W * 4)
        _model(src._buf, src.lo, out._buf, out.lo, n, **mutation)
        runs.append(FootprintRun(out, src))
    return runs, ref


@pytest.mark.parametrize("w0,n", [(0, 40), (3, 11), (37, 3)])
def test_clean_model_passes(w0, n):
    runs, ref = _run(w0, n)
    assert footprint_violations(runs, ref) == []
    assert footprint_violations(runs, ref, rule=lambda payload: []) == []


def test_frames_and_guards_are_what_they_claim():
    f = framed("host", 0, 0, 64, np.zeros(24, np.uint8), 64)
    assert np.isnan(f.snapshot()[:64].view(np.float32)).all() and np.isnan(f.snapshot()[f.hi:].view(np.float32)).all()
    g = framed("host", 0, 1, 64, np.zeros(24, np.uint8), 64)
    assert (g.snapshot()[:64].view(np.float32) == np.finfo(np.float32).max).all()
    assert set(poison(1, 8, 0)) == {0x80} and set(poison(3, 8, 1)) == {0x7F}
    o = framed_out("host", 32, 16)
    assert (o.snapshot() == GUARD_BYTE).all() and o.body.size == 16 and f.body.size == 24
    assert isinstance(o, Framed)


def test_reading_one_sample_past_the_slab_is_reported():
    runs, ref = _run(3, 11, over_read=True)
    bad = footprint_violations(runs, ref)
    assert any(b.startswith("poison:") for b in bad), bad           # the two fills disagree
    assert any(b.startswith("oracle:") for b in bad), bad           # and neither is the oracle's
    assert np.isnan(runs[0].payload.view(np.float32)[-W:]).all()    # the NaN fill reaches the whole last window
    assert not any(b.startswith(("guard:", "unwritten:")) for b in bad), bad


def test_skipping_the_last_window_is_reported():
    runs, ref = _run(3, 11, skip_last=True)
    bad = footprint_violations(runs, ref)
    assert any(b.startswith("unwritten:") and f"first element {10 * W}" in b for b in bad), bad
    assert not any(b.startswith(("poison:", "guard:")) for b in bad), bad
    # under a rule that accepts any payload the stale window is still found by comparison with the oracle
    assert any(b.startswith("unwritten:") for b in footprint_violations(runs, ref, rule=lambda payload: [])), bad


def test_writing_one_element_past_the_payload_is_reported():
    runs, ref = _run(3, 11, over_write=True)
    bad = footprint_violations(runs, ref)
    assert any(b.startswith("guard:") and "back guard" in b and "+0 bytes" in b for b in bad), bad
    assert not any(b.startswith(("poison:", "oracle:", "unwritten:")) for b in bad), bad


def test_a_written_source_is_reported():
    runs, ref = _run(0, 5)
    runs[0].src_uploaded = runs[0].src_now = None                    # pageable host sources are not inspected ...
    assert footprint_violations(runs, ref) == []
    runs[1].src_uploaded = np.zeros(8, np.uint8)
    runs[1].src_now = np.array([0, 0, 1, 0, 0, 0, 0, 0], np.uint8)   # ... device and pinned ones are
    assert any(b.startswith("source:") and "byte 2" in b for b in footprint_violations(runs, ref))
