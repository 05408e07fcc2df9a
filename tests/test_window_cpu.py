"""qd_chain_desc.windowing without a GPU: the window table against the oracle's, the status codes of the field, the geometry calls'
independence of it, and the CLI's -window grammar (every verb that builds a window plan; `rows -window` keeps its own)."""
import ctypes as C
import os

import numpy as np
import pytest

from quadrs_amd import _ffi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsk-example-head65536.sr21M.cf32")
SR = 21_000_000


@pytest.mark.parametrize("W", [2, 3, 4, 100, 128, 4096])
def test_window_design_equals_the_oracles_table(engine, oracle, W):
    ref = np.zeros(W, dtype=np.float32)
    oracle.lib().qo_blackman_harris(W, ref.ctypes.data_as(C.c_void_p))
    got = engine.window_design(engine.WINDOW_BH, W)
    assert got.dtype == np.float32 and got.tobytes() == ref.tobytes()
    assert engine.window_design(engine.WINDOW_RECT, W).tobytes() == np.ones(W, np.float32).tobytes()
    assert (engine.WINDOW_RECT, engine.WINDOW_BH) == (0, 1)


def test_window_design_refusals(engine):
    for bad in (2, -1, 7):
        with pytest.raises(engine.QuadrsError) as ei:
            engine.window_design(bad, 16)
        assert ei.value.code == _ffi.ERR_INVALID
    assert _ffi.lib().qd_window_design(1, 16, None) == _ffi.ERR_INVALID
    assert engine.window_design(1, 0).size == 0


def test_the_field_sits_where_the_padding_was(engine):
    assert _ffi.ChainDesc.windowing.offset == _ffi.ChainDesc.mode.offset + 4 and _ffi.ChainDesc.windowing.size == 4
    assert C.sizeof(_ffi.ChainDesc) == _ffi.ChainDesc.windowing.offset + 4 == 112


STAGE_LISTS = [None, [("lowpass", (200_000, 4, 40)), ("lowpass", (30_000, 4, 64))]]


@pytest.mark.parametrize("stages", STAGE_LISTS, ids=["one-stage", "cascade"])
@pytest.mark.parametrize("epi", ["NORMS_F32", "GLYPH_U8", "BUCKET2_U8", "MARK_U8"])
def test_unknown_windowing_is_refused_before_any_device_call(engine, stages, epi):
    kw = dict(stages=stages) if stages else dict(shift_hz=280000, lowpass=(200_000, 32, 400))
    for bad in (2, -1):
        with pytest.raises(engine.QuadrsError) as ei:
            engine.Plan(engine.FMT_CF32, SR, 65536, width=64, stride=16, epilogue=getattr(engine, "EPI_" + epi), windowing=bad, **kw)
        assert ei.value.code == _ffi.ERR_INVALID and "windowing" in str(ei.value)


@pytest.mark.parametrize("stages", STAGE_LISTS, ids=["one-stage", "cascade"])
def test_the_write_sink_refuses_a_window(engine, stages):
    kw = dict(stages=stages) if stages else dict(lowpass=(200_000, 32, 400))
    with pytest.raises(engine.QuadrsError) as ei:
        engine.Plan(engine.FMT_CF32, SR, 1 << 20, width=0x1000, epilogue=engine.EPI_CF32_BLOCKS, windowing=1, **kw)
    assert ei.value.code == _ffi.ERR_INVALID and "windowing" in str(ei.value)


def test_a_rows_plan_ignores_the_field(engine):
    """QD_EPI_ROWS_F32 takes its window from qd_rows_desc: any value of the chain description's field passes the argument checks (without
    a device the creation then fails on its first device call, never as QD_ERR_INVALID)"""
    for v in (0, 1, 2, -5):
        try:
            engine.Plan(engine.FMT_CF32, SR, 65536, width=64, epilogue=engine.EPI_ROWS_F32, windowing=v).close()
        except engine.QuadrsError as e:
            assert e.code != _ffi.ERR_INVALID and "windowing" not in str(e), (v, str(e))


def _desc(epi, windowing, width=64, stride=16):
    d = _ffi.ChainDesc()
    d.struct_size = C.sizeof(_ffi.ChainDesc)
    d.format, d.sample_rate, d.n_samples = 0, SR, 300_000
    d.width, d.stride, d.epilogue, d.windowing = width, stride, epi, windowing
    return d


def _bytes(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


@pytest.mark.parametrize("stages", [[("shift", 280000), ("lowpass", (200_000, 32, 400))], STAGE_LISTS[1]], ids=["routed", "cascade"])
def test_stages_geometry_does_not_read_the_field(engine, stages):
    from quadrs_amd.engine import stage_array
    got = []
    for v in (0, 1, 2):
        d = _desc(engine.EPI_NORMS_F32, v)
        info, done = _ffi.PlanInfo(), C.c_uint64()
        assert _ffi.lib().qd_stages_geometry(C.byref(d), stage_array(stages), len(stages), C.byref(info), C.byref(done)) == 0
        got.append((_bytes(info), done.value))
    assert got[0] == got[1] == got[2] and got[0][1] > 0


def test_rows_geometry_does_not_read_the_field(engine):
    got = []
    for v in (0, 1, 2):
        d = _desc(engine.EPI_ROWS_F32, v, stride=1)
        d.has_lowpass, d.lowpass_hz, d.decimate, d.taps = 1, 200_000, 32, 400
        r = engine.rows_desc(10, (0, 640), 1)
        offs = np.zeros(10, dtype=np.uint64)
        a, b = C.c_uint64(), C.c_uint64()
        assert _ffi.lib().qd_rows_geometry(C.byref(d), C.byref(r), offs.ctypes.data_as(C.c_void_p), 10, C.byref(a), C.byref(b)) == 0
        got.append((offs.tobytes(), a.value, b.value))
    assert got[0] == got[1] == got[2] and got[0][2] > 0


# ------------------------------------------------------------------ the CLI's grammar

@pytest.fixture(scope="module")
def cli():
    from quadrs_amd import build as B
    B.build()
    return B.build_cli()


def _run(cli, *args):
    import subprocess
    return subprocess.run([cli, "-parse-only", "from", GOLDEN, *args], capture_output=True, timeout=60)


VERBS = {
    "sparkfft": ["-width", "64"],
    "bucket": ["-by", "freq", "2"],
    "marks": ["-min", "0.1"],
    "levels": [],
    "peaks": ["-pool", "3", "P"],
    "means": ["-pool", "3", "P"],
    "powers": ["-pool", "3", "P"],
    "spreads": ["-pool", "3", "P"],
    "quantiles": ["-q", "0.5", "-range", "0:1", "P"],
    "bands": ["-split", "4", "P"],
    "picture": ["-size", "64x64", "P"],
}


def _with(verb, *flags):
    """the verb's command line with `flags` among its named arguments (they come before the positional ones)"""
    tail = VERBS[verb]
    n_pos = 1 if tail and tail[-1] == "P" else 0
    if verb == "bucket":
        n_pos = 1
    named, pos = tail[:len(tail) - n_pos], tail[len(tail) - n_pos:]
    return [verb, *named, *flags, *pos]


@pytest.mark.parametrize("verb", sorted(VERBS))
def test_every_window_plan_verb_takes_the_flag(cli, verb):
    plain = _run(cli, *_with(verb))
    assert plain.returncode == 0, plain.stderr
    bh = _run(cli, *_with(verb, "-window", "bh"))
    assert bh.returncode == 0, bh.stderr
    assert bh.stdout == plain.stdout + b"window=bh\n"             # the verb's own line is unchanged, the window follows it
    rect = _run(cli, *_with(verb, "-window", "rect"))
    assert rect.returncode == 0 and rect.stdout == plain.stdout    # rect is the default
    hann = _run(cli, *_with(verb, "-window", "hann"))
    assert hann.returncode == 2 and b"-window takes bh or rect" in hann.stderr
    twice = _run(cli, *_with(verb, "-window", "bh", "-window", "bh"))
    assert twice.returncode == 2 and b"'-window' specified more than once" in twice.stderr


def test_other_verbs_keep_their_grammar(cli):
    assert _run(cli, "lowpass", "-window", "bh", "200000").returncode == 2
    assert _run(cli, "write", "-window", "bh", "P").returncode == 2
    r = _run(cli, "rows", "-window", "rect", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1].endswith(b"window=rect") and b"window=bh" not in r.stdout
    assert _run(cli, "rows", "P").stdout.split(b"\n")[1].endswith(b"window=bh")
