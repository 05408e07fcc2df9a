"""qd_plan_summarize on the GPU: bit for bit against qd_summary_fold of the oracle's norms (chains without a shift) or of the same
plan's qd_plan_run output (chains with one), over every plan kind; independent of batches, memory kinds and splits; values, refusals
and footprint.  Golden files only."""
import ctypes as C

import numpy as np
import pytest

from test_summary_cpu import F32, np_summary, same

pytestmark = pytest.mark.gpu


def quantised(fsk, fmt, reps=1):
    """the FSK head as bytes of another sample format (any bytes are a valid stream; these keep the signal's shape)"""
    x = np.tile(np.frombuffer(fsk, dtype=F32), reps)
    x = x / np.abs(x).max()
    if fmt == 1:
        return np.round(x * 127).astype(np.int8).tobytes()
    if fmt == 2:
        return (np.round(x * 127) + 128).astype(np.uint8).tobytes()
    if fmt == 3:
        return np.round(x * 32767).astype("<i2").tobytes()
    return x.astype(F32).tobytes()


# name -> (format, sample rate, stream, plan keywords, oracle stages or None when the chain shifts)
def _cases(cupboard, fsk):
    return {
        "cf32_w4_s2": (0, 400, cupboard, dict(width=4, stride=2), []),
        "cs8_fir_w64_s16": (1, 21_000_000, quantised(fsk, 1), dict(lowpass=(200000, 32, 400), width=64, stride=16), [("lowpass", (200000, 32, 400))]),
        "cu8_fir_w128": (2, 21_000_000, quantised(fsk, 2), dict(lowpass=(2_000_000, 16, 40), width=128), [("lowpass", (2_000_000, 16, 40))]),
        "cs16_w1024": (3, 21_000_000, quantised(fsk, 3), dict(width=1024), []),
        "cf32_w64_s16": (0, 21_000_000, fsk, dict(width=64, stride=16), []),
        "cascade_w16_s8": (0, 21_000_000, fsk, dict(stages=[("lowpass", (2_000_000, 4, 40)), ("lowpass", (500_000, 4, 40))], width=16, stride=8),
                           [("lowpass", (2_000_000, 4, 40)), ("lowpass", (500_000, 4, 40))]),
        "two_stage_w1024": (1, 21_000_000, quantised(fsk, 1, reps=4), dict(lowpass=(200000, 32, 40), width=1024), [("lowpass", (200000, 32, 40))]),
        "shift_fir_w64_s16": (0, 21_000_000, fsk, dict(shift_hz=280000, lowpass=(200000, 32, 400), width=64, stride=16), None),
        "shift_w128": (1, 21_000_000, quantised(fsk, 1), dict(shift_hz=-1_000_000, width=128), None),
    }


NAMES = ["cf32_w4_s2", "cs8_fir_w64_s16", "cu8_fir_w128", "cs16_w1024", "cf32_w64_s16", "cascade_w16_s8", "two_stage_w1024", "shift_fir_w64_s16",
         "shift_w128"]


@pytest.fixture(scope="module")
def world(engine, oracle, cupboard, fsk):
    """per case, made once: the plan, the stream (host bytes and a device tensor) and the reference norms of every complete window"""
    import torch
    cache, cases = {}, _cases(cupboard, fsk)

    def get(name):
        if name not in cache:
            fmt, rate, data, kw, stages = cases[name]
            n = len(data) // {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
            plan = engine.Plan(fmt, rate, n, **kw)
            dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            complete = plan.complete_windows()
            W = kw["width"]
            if stages is None:
                # a shift: the plan's own qd_plan_run output OVER THE SAME RANGE, which other tests hold to the oracle (a range that
                # starts off the kernel's row grid runs the per-sample kernel, whose NCO may round a near-tie the other way)
                def ref_of(first=0, count=complete, plan=plan, dev=dev, W=W):
                    out = torch.empty(count, W, dtype=torch.float32, device="cuda")
                    plan.run_device(dev, out, first, count)
                    torch.cuda.synchronize()
                    return out.cpu().numpy()
            else:
                ch = oracle.Chain.from_bytes(data, fmt, rate)
                for _, (f, d, t) in stages:
                    ch = ch.lowpass(f, d, t)
                norms = ch.spark_fft(W, kw.get("stride"), max_windows=complete, want_codes=False)[0]
                assert norms.shape == (complete, W)

                def ref_of(first=0, count=complete, norms=norms):
                    return norms[first:first + count]
            assert complete >= 1
            cache[name] = (plan, data, dev, ref_of, (fmt, rate, n, kw, complete))
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_matches_the_fold_of_the_reference_norms(engine, world, name):
    plan, data, dev, ref_of, spec = world(name)
    n = spec[4]
    G = max(int(plan.info.tile_windows), 1)
    if name == "two_stage_w1024":
        assert plan.info.raw_per_window * 8 > 160 * 1024          # the window's cf32 samples do not fit the LDS tile: stage A + stage B
    assert same(plan.summarize(dev, n_windows=n), np_summary(ref_of()))
    for first, count in {(0, 1), (0, max(G - 1, 1)), (0, G + 1), (1, G + 1), (n // 2, n - n // 2), (n - 1, 1)}:
        if first + count <= n:
            assert same(plan.summarize(dev, first, count), np_summary(ref_of(first, count))), (first, count)
    assert plan.summarize(dev, n_windows=n).tobytes() == engine.summary_fold(ref_of()).tobytes()


@pytest.mark.parametrize("name", ["cf32_w64_s16", "shift_fir_w64_s16", "cascade_w16_s8"])
def test_partition_independence(engine, world, name):
    plan, data, dev, ref_of, (fmt, rate, n_samples, kw, n) = world(name)
    whole = plan.summarize(dev, n_windows=n)
    assert same(whole, np_summary(ref_of()))
    # host, pinned and device sources
    assert plan.summarize(data, n_windows=n).tobytes() == whole.tobytes()
    pin = engine.PinnedBuffer(len(data))
    pin.array[:] = np.frombuffer(data, dtype=np.uint8)
    assert plan.summarize(pin.array, n_windows=n, pinned=True).tobytes() == whole.tobytes()
    pin.close()
    # the smallest chunk_bytes: at least three batches of norms where the stream has that many
    small = engine.Plan(fmt, rate, n_samples, chunk_bytes=1 << 16, **kw)
    if name == "cf32_w64_s16":
        assert n * kw["width"] * 4 >= 3 * (1 << 16)
    assert small.summarize(dev, n_windows=n).tobytes() == whole.tobytes()
    assert small.summarize(data, n_windows=n).tobytes() == whole.tobytes()
    # [0, a) (+) [a, n) == [0, n); behind a shift a part's values are those of qd_plan_run over THAT range (see `world`), which
    # test_matches_the_fold_of_the_reference_norms holds, so the arbitrary splits are made on the chains without one
    for a in (() if "shift_hz" in kw else (1, n // 3, n - 1)):
        merged = plan.summarize(dev, 0, a).merge(plan.summarize(dev, a, n - a))
        assert merged.tobytes() == whole.tobytes(), a


def test_all_zero_stream(engine):
    import torch
    n, W = 1 << 16, 128
    plan = engine.Plan(engine.FMT_CF32, 1_000_000, n, width=W)
    s = plan.summarize(torch.zeros(n, 2, dtype=torch.float32, device="cuda"))
    assert s.n_windows == plan.n_windows and s.hist[0] == s.n_windows * W and int(s.hist.sum()) == s.hist[0]
    assert s.min == 0 and s.max == 0 and s.n_nan == 0 and not s.peak.any() and not s.floor.any()


@pytest.mark.parametrize("W", [2, 64])
def test_planted_nan_and_inf(engine, fsk, W):
    x = np.frombuffer(fsk, dtype=F32).reshape(-1, 2)[:8192].copy()
    x[3 * W] = (np.nan, 0.25)                      # window 3
    x[5 * W + 1] = (np.inf, 0.0)                   # window 5
    x[9 * W] = (0.5, -np.nan)
    plan = engine.Plan(engine.FMT_CF32, 21_000_000, x.shape[0], width=W)
    ref = engine.summary_fold(plan.run_host(x))
    s = plan.summarize(x)
    assert s.tobytes() == ref.tobytes()
    assert s.n_nan > 0 and int(s.hist.sum()) + s.n_nan == s.n_windows * W
    assert s.n_nan + int(s.hist[2040]) >= 3          # windows 3, 5 and 9 each hold a non-finite value


def test_refusals(engine, fsk, cupboard):
    from quadrs_amd import _ffi
    n = len(fsk) // 8

    def code(plan, *a, **k):
        with pytest.raises(engine.QuadrsError) as e:
            plan.summarize(fsk, *a, **k)
        return e.value.code
    for epi in (engine.EPI_GLYPH_U8, engine.EPI_BUCKET2_U8, engine.EPI_MARK_U8):
        assert code(engine.Plan(0, 21_000_000, n, width=64, epilogue=epi)) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, 21_000_000, n, lowpass=(2_000_000, 16, 40), width=1024, epilogue=engine.EPI_CF32_BLOCKS), n_windows=1) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, 21_000_000, n, width=64, stride=1, epilogue=engine.EPI_ROWS_F32), n_windows=1) == _ffi.ERR_INVALID
    assert code(engine.Plan(0, 21_000_000, n, width=64, shard_devices=[0, 0])) == _ffi.ERR_UNSUPPORTED
    plan = engine.Plan(0, 21_000_000, n, width=64)
    assert code(plan, 0, plan.n_windows + 1) == _ffi.ERR_SHORT
    assert code(plan, plan.n_windows, 1) == _ffi.ERR_SHORT
    s = plan.summarize(fsk, 5, 0)
    assert s.tobytes() == engine.summary_init(64).tobytes()


def test_folds_leave_the_run_statistics_alone(engine, fsk):
    """qd_plan_get_stats describes the last qd_plan_run: the folds walk the same host ring and keep no statistics of their own"""
    n = 40_000
    data = fsk[:n * 8]
    plan = engine.Plan(engine.FMT_CF32, 21_000_000, n, width=64, stride=16, chunk_bytes=1 << 16)
    plan.run_host(data)
    fields = [f for f, _ in type(plan.stats())._fields_]
    before = [getattr(plan.stats(), f) for f in fields]
    assert plan.stats().chunks >= 3 and plan.stats().bytes_h2d > 0 and plan.stats().wall_ms > 0
    plan.summarize(data)
    plan.pool(data, 3)
    plan.mean(data, 3)
    assert [getattr(plan.stats(), f) for f in fields] == before


def test_footprint(engine, world):
    from quadrs_amd import _ffi
    plan, data, dev, ref_of, _ = world("cf32_w64_s16")
    ref = ref_of()
    W, guard = 64, 32
    buf = np.frombuffer(data, dtype=np.uint8)
    arr = np.full(2 * guard + W, F32(-7.5), dtype=F32), np.full(2 * guard + W, F32(-7.5), dtype=F32)
    raw = np.full(2 * 64 + C.sizeof(_ffi.Summary), 0xA5, dtype=np.uint8)
    sum_p = C.cast(raw.ctypes.data + 64, C.POINTER(_ffi.Summary))
    ptr = [C.c_void_p(a.ctypes.data + 4 * guard) for a in arr]
    _ffi.check(_ffi.lib().qd_plan_summarize(plan._h, buf.ctypes.data_as(C.c_void_p), _ffi.MEM_HOST, 0, buf.size // 8, 0, ref.shape[0], sum_p,
                                            ptr[0], ptr[1], None))
    exp = np_summary(ref)
    for a, key in zip(arr, ("peak", "floor")):
        assert (a[:guard] == F32(-7.5)).all() and (a[guard + W:] == F32(-7.5)).all()
        assert a[guard:guard + W].tobytes() == exp[key].tobytes()
    assert (raw[:64] == 0xA5).all() and (raw[64 + C.sizeof(_ffi.Summary):] == 0xA5).all()
    assert sum_p.contents.n_windows == ref.shape[0] and np.array_equal(np.ctypeslib.as_array(sum_p.contents.hist), exp["hist"])
