"""The CLI's `quantiles` sink: the percentile pictures PREFIX.sr{rate}.w{W}x{rows}.q{Q}.pgm of the README's FSK chain against the referees
of test_density_cpu (np.add.at counts, integer quantile) over the oracle's spark_fft norms; fused (qd_plan_density), through the iterator
chain (qd_density_fold + qd_density_quantile) and split over -gpus 2 the same bytes; the grammar and the refusal of an existing file.
The tests that compute start the CLI, which opens the GPU; this process never does."""
import os

import numpy as np
import pytest

from test_cli_peaks import CHAIN, GOLDEN, RATE, W, cli, explained, norms, pixels, read_pgm, run  # noqa: F401  (cli, norms: fixtures)
from test_density_cpu import F32, ref_counts, ref_quantile

RANGE = (0.002, 0.05)


def bucket(x):
    return int(np.array([x], F32).view(np.uint32)[0] & 0x7FFFFFFF) >> 20


def grid(rng):
    level0 = bucket(rng[0])
    return level0, min(256, bucket(rng[1]) - level0 + 1)


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_quantiles_fused_unfused_and_two_gpus(cli, norms, tmp_path):
    S, count = 8, 40
    ref = norms[S]
    n = ref.shape[0]
    pool = max(1, -(-n // count))
    rows = -(-n // pool)
    assert pool > 1 and n % pool                   # several windows a row, and a ragged last one
    level0, L = grid(RANGE)
    assert 8 < L < 256
    counts = ref_counts(ref, pool, level0, L)
    qs = ("0.5", "0.9", "0")
    want = {q: pixels(ref_quantile(counts, level0, float(q))[0], RANGE) for q in qs}
    assert (want["0.5"] != want["0.9"]).any() and len(np.unique(want["0.5"])) > 2
    pics = {}
    for tag, pre, env in (("fused", [], None), ("iter", [], {"QUADRS_HIP_NO_FUSE": "1"}), ("two", ["-gpus", "2"], None)):
        prefix = str(tmp_path / tag)
        r = run(cli, *pre, "from", GOLDEN, *CHAIN, "quantiles", "-width", str(W), "-stride", str(S), "-count", str(count), "-q", ",".join(qs),
                "-range", "%g:%g" % RANGE, prefix, env=env)
        assert r.returncode == 0 and r.stdout == b"", (tag, r.stderr)
        names = [f"{tag}.sr{RATE}.w{W}x{rows}.q{q}.pgm" for q in qs]
        assert sorted(f for f in os.listdir(tmp_path) if f.startswith(tag + ".")) == sorted(names), os.listdir(tmp_path)
        pics[tag] = {q: read_pgm(str(tmp_path / name)) for q, name in zip(qs, names)}
        for q in qs:
            assert pics[tag][q].shape == (rows, W)
            assert explained(pics[tag][q], want[q], pool, S, n)
    for tag in ("iter", "two"):
        for q in qs:
            assert pics[tag][q].tobytes() == pics["fused"][q].tobytes(), (tag, q)
    assert pics["fused"]["0.5"].any()
    # -pool with one quantile
    prefix = str(tmp_path / "pooled")
    r = run(cli, "from", GOLDEN, *CHAIN, "quantiles", "-width", str(W), "-stride", "16", "-pool", "7", "-q", "0.25", "-range", "%g:%g" % RANGE, prefix)
    assert r.returncode == 0, r.stderr
    ref = norms[16]
    n16 = ref.shape[0]
    got = read_pgm(f"{prefix}.sr{RATE}.w{W}x{-(-n16 // 7)}.q0.25.pgm")
    assert explained(got, pixels(ref_quantile(ref_counts(ref, 7, level0, L), level0, 0.25)[0], RANGE), 7, 16, n16)
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", GOLDEN, *CHAIN, "quantiles", "-width", str(W), "-stride", str(S), "-count", str(count), "-q", "0.9", "-range", "%g:%g" % RANGE,
            str(tmp_path / "fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr


def test_quantiles_grammar(cli):
    r = run(cli, "-parse-only", "from", GOLDEN, "quantiles", "-q", "0.5", "-range", "0.25:4", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"quantiles width=128 stride=128 count=2048 q=0.5 range=0.25:4", r.stdout
    r = run(cli, "-parse-only", "from", GOLDEN, "quantiles", "-width", "64", "-stride", "16", "-pool", "3", "-q", "0.5,0.9,1", "-range", "0:1", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"quantiles width=64 stride=16 pool=3 q=0.5,0.9,1 range=0:1", r.stdout
    base = ("-parse-only", "from", GOLDEN, "quantiles")
    assert run(cli, *base, "-range", "0:1", "P").returncode == 2                                   # -q is required
    assert run(cli, *base, "-q", "0.5", "P").returncode == 2                                       # -range is required
    assert run(cli, *base, "-q", "0.5", "-range", "0:1").returncode == 2                           # the prefix
    assert run(cli, *base, "-q", "1.5", "-range", "0:1", "P").returncode == 2
    assert run(cli, *base, "-q", "0.5,", "-range", "0:1", "P").returncode == 2
    assert run(cli, *base, "-q", "nan", "-range", "0:1", "P").returncode == 2
    assert run(cli, *base, "-q", ",".join(["0.5"] * 9), "-range", "0:1", "P").returncode == 2
    assert run(cli, *base, "-q", "0.5", "-range", "0:1", "-pool", "3", "-count", "4", "P").returncode == 2
    assert run(cli, *base, "-q", "0.5", "-range", "0:1", "-pool", "0", "P").returncode == 2
    assert run(cli, *base, "-q", "0.5", "-range", "01", "P").returncode == 2
    assert run(cli, *base, "-q", "0.5", "-range", "0:1", "-floor", "yes", "P").returncode == 2
    u = run(cli)
    assert u.returncode == 2
    assert b"quantiles [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) -q 0.5[,0.9,...] -range MIN:MAX FILENAME_PREFIX" in u.stderr
