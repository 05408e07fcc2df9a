"""The CLI's `rows` sink: take_fft's rows (src/ffts.rs:18-85) behind the chain, written as PREFIX.sr{rate}.w{W}x{count}.pgm (binary
PGM, pixel (norm / 10. * 256.) as u8 — the reference view's blue channel, src/eui/mod.rs:104).  A fusable chain runs one
QD_EPI_ROWS_F32 plan, a cascade pulls the rows through the iterator chain into qd_take_fft; both against the oracle's rows.  The tests
that compute start the CLI, which opens the GPU; this process never does."""
import os
import subprocess

import numpy as np
import pytest

from util import explain_check

SR = 21_000_000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsk-example-head65536.sr21M.cf32")
CHAIN = ["shift", "280000", "lowpass", "-decimate", "16", "2000000"]
STAGES = [("shift", 280000), ("lowpass", (2_000_000, 16, 40))]
W, COUNT = 64, 32


@pytest.fixture(scope="module")
def cli():
    from quadrs_amd import build as B
    B.build()
    return B.build_cli()


def run(cli, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([cli, *args], capture_output=True, env=e, timeout=600)


def sat_u8(rows):
    """Rust's `(norm / 10. * 256.) as u8` in f32: truncation, saturating, NaN -> 0"""
    v = rows.astype(np.float32) / np.float32(10.0) * np.float32(256.0)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def read_pgm(path):
    raw = open(path, "rb").read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    assert magic == b"P5" and maxval == b"255" and len(body) == w * h, (magic, dims, maxval, len(body))
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w)


def _oracle_rows(oracle, stages):
    ch = oracle.Chain.from_bytes(open(GOLDEN, "rb").read(), oracle.FMT_CF32, SR)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    rc, rows, offs = ch.take_fft(W, COUNT, None, 1)
    assert rc == 0
    return rows, offs


def _rate(stages):
    r = SR
    for kind, arg in stages:
        if kind == "lowpass":
            r //= arg[1]
    return r


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_rows_picture_fused_and_unfused(cli, oracle, tmp_path):
    ref, offs = _oracle_rows(oracle, STAGES)
    want = sat_u8(ref)
    pics = {}
    for tag, env in (("fused", None), ("iter", {"QUADRS_HIP_NO_FUSE": "1"})):
        prefix = str(tmp_path / tag)
        r = run(cli, "from", GOLDEN, *CHAIN, "rows", "-width", str(W), "-count", str(COUNT), prefix, env=env)
        assert r.returncode == 0, r.stderr
        path = f"{prefix}.sr{_rate(STAGES)}.w{W}x{COUNT}.pgm"
        assert os.path.exists(path), os.listdir(tmp_path)
        pics[tag] = read_pgm(path)
        assert pics[tag].shape == (COUNT, W)
        # with the shift, a row may differ only where the NCO rule explains it (row i is window offs[i] of a stride-1 sink); none expected
        for i in np.nonzero((pics[tag] != want).any(axis=1))[0]:
            bad = explain_check((STAGES, W, 1, SR), np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8), int(offs[i]))
            assert not bad, (tag, int(i), "a differing row reads no ambiguous NCO multiplier")
    assert (pics["fused"] == pics["iter"]).all()
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", GOLDEN, *CHAIN, "rows", "-width", str(W), "-count", str(COUNT), str(tmp_path / "fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_rows_behind_a_cascade_take_the_iterator_path(cli, oracle, tmp_path):
    chain = ["lowpass", "-decimate", "4", "2000000", "lowpass", "-power", "100", "-decimate", "4", "200000"]
    stages = [("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 4, 200))]
    ref, _ = _oracle_rows(oracle, stages)
    prefix = str(tmp_path / "casc")
    r = run(cli, "from", GOLDEN, *chain, "rows", "-width", str(W), "-count", str(COUNT), prefix)
    assert r.returncode == 0, r.stderr
    pic = read_pgm(f"{prefix}.sr{_rate(stages)}.w{W}x{COUNT}.pgm")
    assert (pic == sat_u8(ref)).all()


def test_rows_parse_only(cli):
    r = run(cli, "-parse-only", "from", "x.sr21M.cs8", "rows", "P")
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().splitlines()[-1] == "rows width=512 count=2048 slice=all window=bh"
    r = run(cli, "-parse-only", "from", "x.sr21M.cs8", "rows", "-width", "100", "-count", "7", "-slice", "10:2k", "-window", "rect", "P")
    assert r.stdout.decode().splitlines()[-1] == "rows width=100 count=7 slice=10:2000 window=rect"
    r = run(cli, "-parse-only", "from", "x.sr21M.cs8", "rows", "-window", "hann", "P")
    assert r.returncode == 2 and b"bh or rect" in r.stderr
    assert b"rows [-width 512]" in run(cli).stderr
