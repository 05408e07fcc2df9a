"""The mark sink (QD_EPI_MARK_U8): one byte per sparkfft window, 0 where the reference would print the row blank (every norm < min in
f32, src/fft.rs:54-55), 1 otherwise.

Two references for every shape: (a) the engine's own glyph plan with the same parameters — marks == (glyph != 0).any(axis=1), byte for
byte, the equivalence the header states; (b) the oracle's codes.  Without a shift stage (b) is exact.  With one, an NCO multiplier may
round the other way where it is ambiguous, which moves a norm by an ulp or so: a window is left out of (b) only
when one of its ORACLE norms lies within 4 f32-ulps of `min`, and at most 1 % of the windows may be left out — `min` and the seeds below
were chosen so that the oracle alone meets that (asserted).

The source is an on/off keyed tone plus noise; `min` lies between the off and the on level of the chain's output (the geometric mean of
the largest off-window norm and the smallest on-window maximum of the oracle, rounded to two digits), so both byte values occur."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SR = 21_000_000


def ook(n, tone, period, fmt=0, seed=1, amp=0.02, noise=0.0004):
    """cf32 (or cs8) bytes of n samples: a tone of `tone` cycles per sample, on for the first half of every `period` samples"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    z = amp * np.exp(2j * np.pi * tone * t) * ((t % period) < period // 2)
    z = z + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.stack([z.real, z.imag], axis=1).astype(np.float32)
    if fmt == 0:
        return x.tobytes()
    assert fmt == 1
    return np.clip(np.round(x * 127 * 20), -128, 127).astype(np.int8).tobytes()


# name: (fmt, sample_rate, n_samples, tone (cycles / sample), keying period (samples), chain, W, S, min, plan options)
# chain: dict(shift_hz=, lowpass=) of a one-stage plan or dict(stages=) of a cascade.  The tone sits where the chain's passband ends up.
CFG3P = dict(shift_hz=280000, lowpass=(200_000, 32, 200))
CFG2 = dict(shift_hz=280000, lowpass=(2_000_000, 16, 40))
CFG4 = dict(lowpass=(5_000_000, 8, 512))
GENERIC, SPECIALISE = dict(kernel_policy=1), dict(kernel_policy=2)
# `min` per chain: between the off and the on level of the oracle's per-window maxima (see the module docstring)
MIN_NOLP16 = 0.035
MIN_NOLP64 = 0.049
MIN_NOLP128 = 0.08
MIN_NOLP128_CS8 = 1.6
MIN_CFG3P = 0.018
MIN_CFG2 = 0.33
MIN_CFG4 = 4.9
MIN_LL = 0.038
MIN_SLS = 0.041
MIN_2ST = 1.5
FSK_MIN = 0.115
SHAPES = {
    # no lowpass: the wave-local kernels (k_spark, built in and built for the width; k_spark2: W = 128 at plan time), k_chain for overlaps
    "nolp_w16": (0, SR, 40_000, 0.0131, 2_000, {}, 16, 16, MIN_NOLP16, {}),
    "nolp_w16_jit": (0, SR, 40_000, 0.0131, 2_000, {}, 16, 16, MIN_NOLP16, SPECIALISE),
    "nolp_w64_s16": (0, SR, 40_000, 0.0131, 2_000, {}, 64, 16, MIN_NOLP64, {}),
    "nolp_w64_s16_jit": (0, SR, 40_000, 0.0131, 2_000, {}, 64, 16, MIN_NOLP64, SPECIALISE),
    "nolp_w128_cf32": (0, SR, 60_000, 0.0131, 4_000, {}, 128, 128, MIN_NOLP128, {}),
    "nolp_w128_cf32_jit": (0, SR, 60_000, 0.0131, 4_000, {}, 128, 128, MIN_NOLP128, SPECIALISE),
    "nolp_w128_s32_jit": (0, SR, 60_000, 0.0131, 4_000, {}, 128, 32, MIN_NOLP128, SPECIALISE),
    "nolp_w128_cs8": (1, SR, 60_000, 0.0131, 4_000, {}, 128, 128, MIN_NOLP128_CS8, {}),
    "nolp_w128_cs8_jit": (1, SR, 60_000, 0.0131, 4_000, {}, 128, 128, MIN_NOLP128_CS8, SPECIALISE),
    # cfg3' (deferred FFT on one wave), cfg2, cfg4 (four-wave deferred FFT for the other sinks): ~40 / ~40 / 5 windows; then generic
    "cfg3p": (0, SR, 41 * 4096 + 200, -280000 / SR, 8 * 4096, CFG3P, 128, 128, MIN_CFG3P, {}),
    "cfg2": (0, SR, 41 * 2048 + 40, -280000 / SR, 8 * 2048, CFG2, 128, 128, MIN_CFG2, {}),
    "cfg4": (0, 100_000_000, 5 * 8192 + 512 + 8, 0.01, 2 * 8192, CFG4, 1024, 1024, MIN_CFG4, {}),
    "cfg3p_generic": (0, SR, 41 * 4096 + 200, -280000 / SR, 8 * 4096, CFG3P, 128, 128, MIN_CFG3P, GENERIC),
    "cfg2_generic": (0, SR, 41 * 2048 + 40, -280000 / SR, 8 * 2048, CFG2, 128, 128, MIN_CFG2, GENERIC),
    "cfg4_generic": (0, 100_000_000, 5 * 8192 + 512 + 8, 0.01, 2 * 8192, CFG4, 1024, 1024, MIN_CFG4, GENERIC),
    # cascades (k_cascade): lowpass lowpass, and shift lowpass shift
    "casc_LL": (0, 2_000_000, 60 * 128 * 16 + 400, 0.001, 8 * 128 * 16,
                dict(stages=[("lowpass", (200_000, 4, 40)), ("lowpass", (30_000, 4, 64))]), 128, 128, MIN_LL, {}),
    "casc_SLS": (0, 2_000_000, 60 * 128 * 4 + 400, -300_000 / 2_000_000 - 0.0015, 8 * 128 * 4,
                 dict(stages=[("shift", 300_000), ("lowpass", (200_000, 4, 40)), ("shift", 3_000)]), 128, 128, MIN_SLS, {}),
    # a window past one workgroup's LDS: the two-stage plan hands the sink to its second stage
    "two_stage": (0, SR, 5 * 32768 + 200 + 32, 0.0003, 2 * 32768, dict(lowpass=(200_000, 32, 200)), 1024, 1024, MIN_2ST, {}),
}
CHECKED = ("nolp_w64_s16", "cfg3p")      # the shapes that also run as sub-ranges, twice, in chunks and in shards


def chain_kw(chain):
    return dict(chain)


def oracle_chain(O, data, fmt, sr, chain):
    ch = O.Chain.from_bytes(data, fmt, sr)
    stages = chain.get("stages")
    if stages is None:
        stages = ([("shift", chain["shift_hz"])] if "shift_hz" in chain else []) + ([("lowpass", chain["lowpass"])] if "lowpass" in chain else [])
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch, any(k == "shift" for k, _ in stages)


def near_min(norms, mn, ulps=4):
    """windows with a norm within `ulps` f32-ulps of mn"""
    mn = np.float32(mn)
    return (np.abs(norms.astype(np.float64) - np.float64(mn)) <= ulps * np.float64(np.spacing(mn))).any(axis=1)


_cache = {}


def reference(O, name):
    """(data, oracle norms, oracle marks, excusable windows) of a shape: computed once, shared, never written to"""
    if name not in _cache:
        fmt, sr, n, tone, period, chain, W, S, mn, _ = SHAPES[name]
        key = (fmt, sr, n, tone, period, repr(chain), W, S, mn)
        for other, val in _cache.items():
            if val[0] == key:
                _cache[name] = val
                break
        else:
            data = ook(n, tone, period, fmt)
            ch, shifted = oracle_chain(O, data, fmt, sr, chain)
            norms, codes = ch.spark_fft(W, S, (mn, 1.0))
            marks = (codes != 0).any(axis=1).astype(np.uint8)
            excuse = near_min(norms, mn) if shifted else np.zeros(len(marks), dtype=bool)
            for a in (norms, marks, excuse):
                a.setflags(write=False)
            _cache[name] = (key, data, norms, marks, excuse)
    return _cache[name][1:]


def plans(engine, name):
    fmt, sr, n, _, _, chain, W, S, mn, opts = SHAPES[name]
    kw = dict(chain_kw(chain), width=W, stride=S, rng=(mn, 1.0), **opts)
    return engine.Plan(fmt, sr, n, epilogue=engine.EPI_MARK_U8, **kw), engine.Plan(fmt, sr, n, epilogue=engine.EPI_GLYPH_U8, **kw)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_marks_equal_glyph_rows_and_oracle(engine, oracle, name):
    data, norms, ref, excuse = reference(oracle, name)
    assert 0.2 < ref.mean() < 0.8, ref.mean()                    # both byte values occur
    assert excuse.mean() <= 0.01, excuse.mean()                  # the oracle alone: at most 1 % of the windows near `min`
    pm, pg = plans(engine, name)
    assert pm.info.out_bytes_per_window == 1 and pm.n_windows == pg.n_windows == len(ref)
    assert pm.src_range(0, pm.n_windows) == pg.src_range(0, pg.n_windows)
    marks = pm.run_host(data)
    glyph = pg.run_host(data)
    print(name, pm.kernel_name()[:60], "mean", marks.mean(), "excused", int(excuse.sum()))
    assert marks.dtype == np.uint8 and marks.shape == (len(ref),)
    assert 0.2 < marks.mean() < 0.8, marks.mean()
    assert np.array_equal(marks, (glyph != 0).any(axis=1).astype(np.uint8))          # (a)
    bad = (marks != ref) & ~excuse
    assert not bad.any(), np.nonzero(bad)[0][:10]                                      # (b)


def test_cupboard_readme_run_lengths(engine, oracle, cupboard):
    """README "Worked example: OOK in sed": sparkfft -width 4 -stride 2 on the cupboard capture, rows to blank / not blank, `uniq -c`.
    The README quotes the runs 8 . / 8 X / 16 . / 17 X / 15 . / 16 X between two "..." (README.md:133-141): they are not the head of
    the stream — the capture opens with 286 blank rows and the preamble's runs of 8 — but the six runs around the first run of 17.
    That is what is asserted: the first 17 is a marked run and its neighbourhood reads 8, 8, 16, 17, 15, 16 from a blank run on."""
    n = len(cupboard) // 8
    ch = oracle.Chain.from_bytes(cupboard, 0, 400)
    _, codes = ch.spark_fft(4, 2, (0.001, 1.0))
    ref = (codes != 0).any(axis=1).astype(np.uint8)
    for opts in ({}, SPECIALISE, GENERIC):                      # k_spark0 where a build is to be had (SPECIALISE), else the generic kernels
        kw = dict(width=4, stride=2, rng=(0.001, 1.0), **opts)
        pm = engine.Plan(0, 400, n, epilogue=engine.EPI_MARK_U8, **kw)
        marks = pm.run_host(cupboard)
        glyph = engine.Plan(0, 400, n, epilogue=engine.EPI_GLYPH_U8, **kw).run_host(cupboard)
        print(pm.kernel_name()[:60])
        assert np.array_equal(marks, (glyph != 0).any(axis=1).astype(np.uint8))
        assert np.array_equal(marks, ref)
        edges = np.flatnonzero(np.diff(marks)) + 1
        runs = np.diff(np.concatenate([[0], edges, [len(marks)]])).tolist()
        assert marks[0] == 0                                    # so even-numbered runs are blank
        i = runs.index(17)
        assert i % 2 == 1 and runs[i - 3:i + 3] == [8, 8, 16, 17, 15, 16], runs


def test_fsk_readme_chain(engine, oracle, fsk):
    """the README's FSK chain on the head of its capture: shift 280000, 400 taps / 32, W 64 / S 16 (the streaming kernel)"""
    n, mn = len(fsk) // 8, FSK_MIN
    ch = oracle.Chain.from_bytes(fsk, 0, SR).shift(280000).lowpass(200_000, 32, 400)
    norms, codes = ch.spark_fft(64, 16, (mn, 1.0))
    ref = (codes != 0).any(axis=1).astype(np.uint8)
    excuse = near_min(norms, mn)
    assert 0.2 < ref.mean() < 0.8 and excuse.mean() <= 0.01, (ref.mean(), excuse.mean())
    for opts in ({}, SPECIALISE):
        kw = dict(shift_hz=280000, lowpass=(200_000, 32, 400), width=64, stride=16, rng=(mn, 1.0), **opts)
        marks = engine.Plan(0, SR, n, epilogue=engine.EPI_MARK_U8, **kw).run_host(fsk)
        glyph = engine.Plan(0, SR, n, epilogue=engine.EPI_GLYPH_U8, **kw).run_host(fsk)
        assert np.array_equal(marks, (glyph != 0).any(axis=1).astype(np.uint8))
        assert not ((marks != ref) & ~excuse).any()



@pytest.mark.parametrize("name", CHECKED)
def test_subranges_twice_chunks_and_shards(engine, oracle, name):
    import torch
    data, _, _, _ = reference(oracle, name)
    fmt, sr, n, _, _, chain, W, S, mn, opts = SHAPES[name]
    pm, _ = plans(engine, name)
    whole = pm.run_host(data)
    nw = pm.n_windows
    # a window sub-range out of a slab that starts inside the stream
    w0, cnt = nw // 3 + 1, nw // 2
    first, count = pm.src_range(w0, cnt)
    bps = 8 if fmt == 0 else 2
    part = pm.run_host(data[first * bps:(first + count) * bps], first_window=w0, n_windows=cnt, src_first=first)
    assert np.array_equal(part, whole[w0:w0 + cnt])
    # run_device twice into the same buffer
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.full((nw,), 0xA5, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        pm.run_device(src, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), whole)
    # a host run in 64 KiB chunks, and three shards
    kw = dict(chain_kw(chain), width=W, stride=S, rng=(mn, 1.0), epilogue=engine.EPI_MARK_U8, **opts)
    assert np.array_equal(engine.Plan(fmt, sr, n, chunk_bytes=1 << 16, **kw).run_host(data), whole)
    assert np.array_equal(engine.Plan(fmt, sr, n, shard_devices=[0, 0, 0], **kw).run_sharded_host(data), whole)


def test_footprint_exactly_n_bytes(engine, oracle):
    """the output lies between 0xA5 guards: exactly n_windows bytes are written (each is 0 or 1), the guards stay intact"""
    import torch
    name = "cfg3p"
    data, _, ref, excuse = reference(oracle, name)
    pm, _ = plans(engine, name)
    nw, G = pm.n_windows, 4096
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    buf = torch.full((nw + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    pm.run_device(src, buf[G:G + nw])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:G] == 0xA5).all() and (got[G + nw:] == 0xA5).all()
    assert (got[G:G + nw] <= 1).all()                          # every byte of the window range was written
    assert not ((got[G:G + nw] != ref) & ~excuse).any()


@pytest.mark.parametrize("name", ["nolp_w16", "nolp_w128_cf32_jit", "cfg3p", "cfg4", "casc_LL", "two_stage"])
def test_all_blank_and_all_marked(engine, name):
    fmt, sr, n, tone, period, chain, W, S, _, opts = SHAPES[name]
    kw = dict(chain_kw(chain), width=W, stride=S, epilogue=engine.EPI_MARK_U8, **opts)
    zeros = bytes(n * (8 if fmt == 0 else 2))
    blank = engine.Plan(fmt, sr, n, **kw).run_host(zeros)        # the default min, 0.08
    assert blank.size and not blank.any()
    marked = engine.Plan(fmt, sr, n, rng=(0.0, 1.0), **kw).run_host(zeros)       # no norm is < 0
    assert (marked == 1).all()
    nan = engine.Plan(fmt, sr, n, rng=(float("nan"), 1.0), **kw).run_host(zeros)   # a NaN min compares false
    assert (nan == 1).all()
