"""The CLI's -window bh: `sparkfft` prints the oracle-rendered text of the reference's windowed rows (take_fft with windowing 1 over
the same chain, stepping by the stride), the fused plan and the iterator chain (QUADRS_HIP_NO_FUSE=1: the same two products on the
host) print the same bytes, and `means` writes the same picture either way.  The chain has no shift, so norms are exact.  The tests
start the CLI, which opens the GPU; this process never does."""
import os

import numpy as np
import pytest

from test_cli_peaks import GOLDEN, SR, cli, pixels, read_pgm, run  # noqa: F401  (cli: fixture)
from test_mean_cpu import ref_mean

CHAIN = ["lowpass", "-power", "200", "-decimate", "32", "200000"]
RATE = SR // 32
W = 64


def windowed_norms(oracle, S):
    """every window `sparkfft -width 64 -stride S` prints behind CHAIN, under the Blackman-Harris window: the reference's take_fft rows"""
    ch = oracle.Chain.from_bytes(open(GOLDEN, "rb").read(), oracle.FMT_CF32, SR).lowpass(200000, 32, 400)
    n = oracle.lib().qo_spark_window_count(ch.len(), W, S)
    assert n * S < ch.len() and (n - 1) * S + W <= ch.len()
    rc, rows, offs = ch.take_fft(W, n, (0, n * S), 1)
    assert rc == 0 and np.array_equal(offs, S * np.arange(n, dtype=np.uint64))
    return rows


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_sparkfft_window_bh(cli, oracle):
    S = 16
    norms = windowed_norms(oracle, S)
    lo, hi = (f"{float(np.quantile(norms, q)):.3g}" for q in (0.3, 0.97))
    rmin, rmax = np.float32(float(lo)), np.float32(float(hi))
    g = oracle.lib().qo_glyph_code
    codes = np.array([g(float(v), float(rmin), float(rmax)) for v in norms.reshape(-1)], dtype=np.uint8).reshape(norms.shape)
    assert len(np.unique(codes)) >= 5                      # the range exercises the glyph ladder
    want = oracle.render(RATE, codes)
    args = ("from", GOLDEN, *CHAIN, "sparkfft", "-width", str(W), "-stride", str(S), "-window", "bh", "-range", f"{lo}:{hi}")
    fused = run(cli, *args)
    assert fused.returncode == 0, fused.stderr
    assert fused.stdout == want
    it = run(cli, *args, env={"QUADRS_HIP_NO_FUSE": "1"})
    assert it.returncode == 0, it.stderr
    assert it.stdout == fused.stdout
    rect = run(cli, *[a for a in args if a not in ("-window", "bh")])
    assert rect.returncode == 0 and rect.stdout != fused.stdout and rect.stdout.count(b"\n") == fused.stdout.count(b"\n")


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_means_window_bh(cli, oracle, tmp_path):
    S, pool = 8, 7
    norms = windowed_norms(oracle, S)
    n = norms.shape[0]
    rows = -(-n // pool)
    want = pixels(ref_mean(norms, pool)[0], (0.0, float(np.float32(norms.max()))))
    rng = f"0:{float(np.float32(norms.max())):.9g}"
    pics = {}
    for tag, env in (("fused", None), ("iter", {"QUADRS_HIP_NO_FUSE": "1"})):
        prefix = str(tmp_path / tag)
        r = run(cli, "from", GOLDEN, *CHAIN, "means", "-width", str(W), "-stride", str(S), "-pool", str(pool), "-window", "bh", "-range", rng, prefix, env=env)
        assert r.returncode == 0 and r.stdout == b"", (tag, r.stderr)
        name = f"{tag}.sr{RATE}.w{W}x{rows}.mean.pgm"
        assert name in os.listdir(tmp_path), os.listdir(tmp_path)
        pics[tag] = read_pgm(str(tmp_path / name))
    assert pics["iter"].tobytes() == pics["fused"].tobytes()
    assert pics["fused"].tobytes() == want.tobytes() and want.any()
