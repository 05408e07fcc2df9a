"""The three-multiplication NCO rotation on the GPU (-m gpu), held to the NCO rule (util.unexplained_windows) where nothing hides a flip.

Shape: shift 280 000 Hz at 21 Msps -> sparkfft -width 4 -stride 4, no lowpass, over a stream of 1 + 0i (cs8: 127 + 0i), 2^18 windows a
case: a window reads four multipliers and its four bins are sums of them, so a multiplier component that rounds the other way changes
its window.  The referee is the oracle over the slab with the reference's f32 multipliers of the ABSOLUTE indices planted through
override_shift (as util.deep_reference does).  Runtime-geometry kernel (rows of 512 samples cf32, 1024 cs8) and the built-in wave-local
kernel (rows of 512), first and second order forced through the plan's options, each at three depths of a described 2^34-sample
stream: first order at sample 0, at 2^27 rad and in the last 2^20 samples below the 2^28 rad switch; second order in the first 2^20
above it, at 2^30 rad and at the stream's end (2^30.4 rad: at this ratio 2^32 rad lies past sample 2^34).  Asserted: no unexplained
window at eps = NCO_ABS_ERR (2e-15), and none at 1.6e-15 either — the derived bound is 1.51e-15 (qd_nco.h), so the tighter run shows
that the margin is real; it is no new tolerance.

One cfg3'-shaped case (shift -> 200-tap lowpass / 32 -> 128-point FFT) on 2^22 samples: the built-in kernel's windows, a window
sub-range from a slab that starts one sample early (off every load vector: the 256-thread per-sample kernel) and the runtime-geometry
kernel agree word for word, and the built-in kernel's output equals the oracle's under the rule."""
import math

import numpy as np
import pytest

from util import NCO_ABS_ERR, shift_ratios, shift_spans, unexplained_windows

pytestmark = pytest.mark.gpu

SR, HZ, W = 21_000_000, 280_000, 4
N_DESCRIBED = (1 << 34) - 4096              # (the sink's loop counts windows in 32 bits: 2^32 - 1024 windows of four samples)
N_WIN = 1 << 18
ALIGN = 4096                                     # samples: a multiple of both row lengths and of every tile of the kernels below
RATIO = math.tau * HZ / SR
_SWITCH = int((1 << 28) / RATIO)                 # last sample with |place| <= 2^28 rad


def _down(n):
    return n // ALIGN * ALIGN


DEPTHS = {
    1: [("sample 0", 0), ("2^27 rad", _down(int((1 << 27) / RATIO))), ("below the switch", _down(_SWITCH + 1 - N_WIN * W))],
    2: [("above the switch", _down(_SWITCH) + ALIGN), ("2^30 rad", _down(int((1 << 30) / RATIO))), ("end", None)],
}
CASES = [(fmt, "generic", order, d) for fmt in (0, 1) for order in (1, 2) for d in range(3)] + \
        [(0, "builtin", 1, 2), (0, "builtin", 2, 0), (1, "builtin", 2, 2)]


def _case_id(c):
    return f"{'cf32' if c[0] == 0 else 'cs8'}-{c[1]}-order{c[2]}-{DEPTHS[c[2]][c[3]][0].replace(' ', '_')}"


_REFS = {}


def _reference(oracle, fmt, base, count, n):
    """the oracle's norms of windows [base / 4, base / 4 + n) of the constant stream, from the slab [base, base + count)"""
    key = (fmt, base, count, n)
    if key not in _REFS:
        raw = np.tile(np.array([1.0, 0.0], dtype=np.float32).view(np.uint8) if fmt == 0 else np.array([127, 0], dtype=np.uint8), count)
        c, s = oracle.shift_multipliers_f64(RATIO, base, count)
        ch = oracle.Chain.from_bytes(raw, fmt, SR).shift(HZ)
        ch.override_shift(0, np.arange(count, dtype=np.uint64), c.astype(np.float32), s.astype(np.float32))
        ref = ch.spark_fft(W, W, max_windows=n, want_codes=False)[0]
        raw.setflags(write=False)
        ref.setflags(write=False)
        _REFS[key] = (raw, ref)
    return _REFS[key]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_flat_stream_windows_differ_only_at_near_ties(engine, oracle, case):
    import torch
    fmt, policy, order, d = case
    opts = engine.plan_options(kernel_policy=engine.KERNEL_GENERIC if policy == "generic" else engine.KERNEL_NO_PLAN_TIME, nco_order=order)
    p = engine.Plan(fmt, SR, N_DESCRIBED, shift_hz=HZ, width=W, stride=W, options=opts)
    name = p.kernel_name()
    assert f"nco {order}" in name and ("k_spark" in name) == (policy == "builtin"), name
    total = int(p.n_windows)
    base = DEPTHS[order][d][1]
    if base is None:                             # the stream's last windows
        w0 = (total - N_WIN) // (ALIGN // W) * (ALIGN // W)
        n, base = total - w0, w0 * W
        count = N_DESCRIBED - base
    else:
        w0, n, count = base // W, N_WIN, (N_WIN + 1) * W
    if order == 1:
        assert (base + count) * RATIO <= (1 << 28) + 8 * RATIO, (base, count)      # the first-order form's own range (one window of slack: never read)
    assert p.src_range(w0, n)[0] == base and sum(p.src_range(w0, n)) <= base + count
    raw, ref = _reference(oracle, fmt, base, count, n)
    src = torch.from_numpy(raw.copy()).cuda()
    out = torch.full((n, W), float("nan"), dtype=torch.float32, device="cuda")
    p.run_device(src, out, w0, n, src_first=base, src_count=count)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    p.close()
    desc = ([("shift", HZ)], W, W, SR)
    differing = int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum())
    bad = {}
    for eps in (NCO_ABS_ERR, 1.6e-15):
        bad[eps] = unexplained_windows(ref, got, lambda w: shift_spans(desc, w), shift_ratios(desc), w0, eps=eps)
    print(f"{_case_id(case)}: {name[:60]} windows {n} from {w0}: differing {differing}, unexplained {[len(b) for b in bad.values()]}")
    assert np.isfinite(got).all()
    assert bad[NCO_ABS_ERR] == [], bad[NCO_ABS_ERR][:8]
    assert bad[1.6e-15] == [], bad[1.6e-15][:8]


def test_headline_shape_kernels_agree_word_for_word(engine, oracle):
    """cfg3' on 2^22 samples (1023 windows, a window a tile: every workgroup of the built-in kernel takes several)"""
    n, lp = 1 << 22, (200_000, 32, 200)
    rng = np.random.default_rng(20261021)
    raw = (rng.standard_normal((n, 2)) * 0.03).astype(np.float32).view(np.uint8).reshape(-1)
    built = engine.Plan(0, SR, n, shift_hz=HZ, lowpass=lp, width=128, stride=128, options=engine.plan_options(kernel_policy=engine.KERNEL_NO_PLAN_TIME))
    gen = engine.Plan(0, SR, n, shift_hz=HZ, lowpass=lp, width=128, stride=128, options=engine.plan_options(kernel_policy=engine.KERNEL_GENERIC))
    assert int(built.info.kernel_kind) == 1 and "k_chain" in built.kernel_name() and "FixedGeo" in built.kernel_name(), built.kernel_name()
    assert int(gen.info.kernel_kind) == 0, gen.kernel_name()
    nw = int(built.n_windows)
    assert nw == int(gen.n_windows) and nw > 1000
    a = built.run_host(raw)
    b = gen.run_host(raw)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # windows [5, nw - 3) from a slab that starts one sample before the first one they read: the per-sample kernel
    w0, m = 5, nw - 8
    first, count = built.src_range(w0, m)
    assert (first - 1) % 2 == 1
    c = built.run_host(raw[(first - 1) * 8:(first + count) * 8], w0, m, src_first=first - 1)
    assert np.array_equal(c.view(np.uint32), a[w0:w0 + m].view(np.uint32))
    ref = oracle.Chain.from_bytes(raw, 0, SR).shift(HZ).lowpass(*lp).spark_fft(128, 128, want_codes=False)[0]
    assert ref.shape == a.shape
    desc = ([("shift", HZ), ("lowpass", lp)], 128, 128, SR)
    bad = unexplained_windows(ref, a, lambda w: shift_spans(desc, w), shift_ratios(desc), 0)
    print(f"cfg3' shape: {nw} windows, differing from the oracle {int((a.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum())}, unexplained {len(bad)}")
    assert bad == [], bad[:8]
    built.close()
    gen.close()
