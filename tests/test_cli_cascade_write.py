"""The CLI's `write` sink behind a cascade: the full 0x1000-sample read_at blocks come from one fused plan (qd::k_cascade_write), the
ragged end from the block iterator, and the file holds the reference's bytes (do_write, src/lib.rs:178-213).  These tests start the
CLI, which opens the GPU; this process never does."""
import os
import subprocess

import numpy as np
import pytest

from util import explain_check

pytestmark = [pytest.mark.gpu, pytest.mark.spawns_gpu_ranks]

SR = 21_000_000
BLK = 0x1000
L1 = ["lowpass", "-decimate", "4", "2000000"]
L2 = ["lowpass", "-power", "100", "-decimate", "8", "200000"]
ST1, ST2 = ("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200))
CHAINS = {
    "LL": (L1 + L2, [ST1, ST2]),
    "SLL": (["shift", "280000"] + L1 + L2, [("shift", 280_000), ST1, ST2]),
    "LS": (["lowpass", "-power", "200", "-decimate", "16", "2000000", "shift", "20000"], [("lowpass", (2_000_000, 16, 400)), ("shift", 20_000)]),
    "LLS": (L1 + L2 + ["shift", "20000"], [ST1, ST2, ("shift", 20_000)]),
}


@pytest.fixture(scope="module")
def cli():
    from quadrs_amd import build as B
    B.build()
    return B.build_cli()


def run(cli, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([cli, *args], capture_output=True, env=e, timeout=600)


def _signal(n, fmt, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    z = 0.2 * np.exp(2j * np.pi * (-0.0133) * t) * np.sign(np.sin(2 * np.pi * t / 2187.0) + 1e-9)
    z = z + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.stack([z.real, z.imag], axis=1)
    if fmt == "cf32":
        return x.astype(np.float32).tobytes()
    return np.clip(np.round(x * 127 * 2), -128, 127).astype(np.int8).tobytes()


def _span_step(stages):
    span, D = BLK, 1
    for kind, arg in reversed(stages):
        if kind == "lowpass":
            span, D = span * arg[1] + arg[2], D * arg[1]
    return span, BLK * D


def _write(cli, tmp_path, tag, src, chain, env=None, gpus=None):
    prefix = str(tmp_path / tag)
    pre = ["-gpus", str(gpus)] if gpus else []
    r = run(cli, *pre, "from", src, *chain, "write", prefix, env=env)
    outs = [f for f in os.listdir(tmp_path) if f.startswith(tag + ".sr")]
    assert len(outs) == 1, (outs, r.stderr)
    return r, np.fromfile(str(tmp_path / outs[0]), dtype=np.float32).reshape(-1, 2)


@pytest.mark.parametrize("fmt", ["cf32", "cs8"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_cascade_write_file(cli, oracle, tmp_path, name, fmt):
    chain, stages = CHAINS[name]
    span, step = _span_step(stages)
    n = span + 5 * step + 54_321                            # six full blocks and a ragged end
    data = _signal(n, fmt, seed=len(name) * 3 + len(fmt))
    src = str(tmp_path / f"sig.sr21M.{fmt}")
    with open(src, "wb") as f:
        f.write(data)
    ch = oracle.Chain.from_bytes(data, oracle.FMT_CF32 if fmt == "cf32" else oracle.FMT_CS8, SR)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    rc, n_ref, ref = ch.do_write(ch.len() + 2 * BLK)
    full = 0
    while ch.read_at(full * BLK, BLK)[0] == BLK:
        full += 1
    assert full == 6

    r, got = _write(cli, tmp_path, "fused", src, chain)
    # the reference's end-of-stream assert (assert_ne!(0, read)): a chain of two lowpasses may over-report its length
    assert (r.returncode != 0) == (rc != 0), (r.returncode, rc, r.stderr)
    if rc != 0:
        assert b"short read" in r.stderr, r.stderr
    assert got.shape == ref.shape, (got.shape, ref.shape)
    slow_r, slow = _write(cli, tmp_path, "iter", src, chain, env={"QUADRS_HIP_NO_FUSE": "1"})
    assert slow_r.returncode == r.returncode
    # the ragged end is the iterator's in both runs
    assert got[full * BLK:].tobytes() == slow[full * BLK:].tobytes()
    head_ref, head = ref[:full * BLK].reshape(full, -1), got[:full * BLK].reshape(full, -1)
    if any(k == "shift" for k, _ in stages):
        assert explain_check((stages, BLK, BLK, SR), head_ref, head) == []
    else:
        assert got.tobytes() == ref.tobytes()
        assert got.tobytes() == slow.tobytes()
    two_r, two = _write(cli, tmp_path, "two", src, chain, gpus=2)
    assert two_r.returncode == r.returncode and two.tobytes() == got.tobytes()


def test_three_lowpasses_write_through_the_iterator(cli, oracle, tmp_path):
    chain = L1 + ["lowpass", "-decimate", "2", "400000"] + ["lowpass", "-decimate", "2", "100000"]
    stages = [ST1, ("lowpass", (400_000, 2, 40)), ("lowpass", (100_000, 2, 40))]
    n = 300_017
    data = _signal(n, "cf32", seed=41)
    src = str(tmp_path / "sig.sr21M.cf32")
    with open(src, "wb") as f:
        f.write(data)
    ch = oracle.Chain.from_bytes(data, oracle.FMT_CF32, SR)
    for _, arg in stages:
        ch = ch.lowpass(*arg)
    rc, _, ref = ch.do_write(ch.len() + 2 * BLK)
    r, got = _write(cli, tmp_path, "three", src, chain)
    assert (r.returncode != 0) == (rc != 0), r.stderr
    assert got.tobytes() == ref.tobytes() and got.shape[0] > BLK
    _, slow = _write(cli, tmp_path, "three_iter", src, chain, env={"QUADRS_HIP_NO_FUSE": "1"})
    assert slow.tobytes() == got.tobytes()
