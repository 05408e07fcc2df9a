"""The CLI's `spreads` sink: the deviation-trace picture PREFIX.sr{rate}.w{W}x{rows}.std.pgm of the README's FSK chain against the integer
referee's std (test_spread_cpu) of the oracle's spark_fft norms; fused (qd_plan_spread), through the iterator chain (qd_spread_fold +
qd_spread_finish) and split over -gpus 2 the same bytes; -pool / -count, -range and its error, and the refusal of an existing file.  The
tests that compute start the CLI, which opens the GPU; this process never does."""
import os

import numpy as np
import pytest

from test_cli_peaks import CHAIN, GOLDEN, RATE, W, cli, explained, norms, pixels, read_pgm, run  # noqa: F401  (cli, norms: fixtures)
from test_spread_cpu import ref_spread


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_spreads_fused_unfused_and_two_gpus(cli, norms, tmp_path):
    S, count = 8, 40
    ref = norms[S]
    n = ref.shape[0]
    pool = max(1, -(-n // count))
    rows = -(-n // pool)
    assert pool > 1 and n % pool                   # several windows a row, and a ragged last one
    std = ref_spread(ref, pool)[0]
    # the default pixel rule (v / 10 * 256) leaves this chain's deviations black; -range puts them on the scale
    rng = (0.0, float(np.float32(float(std.max()) * 1.01)))        # an f32 value: its decimal form reads back as itself
    want = pixels(std, rng)
    assert want.any() and (want < 255).all()
    pics = {}
    for tag, pre, env in (("fused", [], None), ("iter", [], {"QUADRS_HIP_NO_FUSE": "1"}), ("two", ["-gpus", "2"], None)):
        prefix = str(tmp_path / tag)
        r = run(cli, *pre, "from", GOLDEN, *CHAIN, "spreads", "-width", str(W), "-stride", str(S), "-count", str(count), "-range", "%r:%r" % rng, prefix,
                env=env)
        assert r.returncode == 0 and r.stdout == b"", (tag, r.stderr)
        name = f"{tag}.sr{RATE}.w{W}x{rows}.std.pgm"
        assert name in os.listdir(tmp_path) and len(os.listdir(tmp_path)) == len(pics) + 1, os.listdir(tmp_path)
        pics[tag] = read_pgm(str(tmp_path / name))
        assert pics[tag].shape == (rows, W)
        assert explained(pics[tag], want, pool, S, n)
    for tag in ("iter", "two"):
        assert pics[tag].tobytes() == pics["fused"].tobytes(), tag
    assert pics["fused"].any()
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", GOLDEN, *CHAIN, "spreads", "-width", str(W), "-stride", str(S), "-count", str(count), str(tmp_path / "fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_spreads_count_pool_and_default_rule(cli, norms, tmp_path):
    # -width 64 -count 40 at the default stride: fewer windows than rows asked for, so pool = 1 and every deviation is +0: a black picture
    ref = norms[64]
    n = ref.shape[0]
    assert n < 40 and not np.isnan(ref).any()
    prefix = str(tmp_path / "plain")
    r = run(cli, "from", GOLDEN, *CHAIN, "spreads", "-width", str(W), "-count", "40", prefix)
    assert r.returncode == 0, r.stderr
    assert os.listdir(tmp_path) == [f"plain.sr{RATE}.w{W}x{n}.std.pgm"]
    assert not read_pgm(f"{prefix}.sr{RATE}.w{W}x{n}.std.pgm").any()
    # -pool 7 under the default pixel rule, v / 10 * 256
    S, pool = 16, 7
    ref = norms[S]
    n = ref.shape[0]
    rows = -(-n // pool)
    prefix = str(tmp_path / "pooled")
    r = run(cli, "from", GOLDEN, *CHAIN, "spreads", "-width", str(W), "-stride", str(S), "-pool", str(pool), prefix)
    assert r.returncode == 0, r.stderr
    got = read_pgm(f"{prefix}.sr{RATE}.w{W}x{rows}.std.pgm")
    assert explained(got, pixels(ref_spread(ref, pool)[0]), pool, S, n)
    # -count R is -pool ceil(windows / R)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert run(cli, "from", GOLDEN, *CHAIN, "spreads", "-width", str(W), "-stride", str(S), "-count", str(rows), a).returncode == 0
    assert run(cli, "from", GOLDEN, *CHAIN, "spreads", "-width", str(W), "-stride", str(S), "-pool", str(-(-n // rows)), b).returncode == 0
    tail = f".sr{RATE}.w{W}x{-(-n // -(-n // rows))}.std.pgm"
    assert open(a + tail, "rb").read() == open(b + tail, "rb").read()


def test_spreads_grammar(cli):
    r = run(cli, "-parse-only", "from", GOLDEN, "spreads", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"spreads width=128 stride=128 count=2048 range=no"
    r = run(cli, "-parse-only", "from", GOLDEN, "spreads", "-width", "64", "-stride", "16", "-pool", "3", "-range", "0:1", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"spreads width=64 stride=16 pool=3 range=yes"
    assert run(cli, "-parse-only", "from", GOLDEN, "spreads", "-pool", "3", "-count", "4", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "spreads", "-pool", "0", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "spreads", "-floor", "yes", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "spreads", "-range", "01", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "spreads").returncode == 2
    u = run(cli)
    assert u.returncode == 2 and b"  spreads [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) [-range MIN:MAX] FILENAME_PREFIX" in u.stderr


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_spreads_range_error(cli, tmp_path):
    """-range lo:hi with lo >= hi is refused by name before anything is written"""
    for bad in ("0.5:0.5", "1:0"):
        r = run(cli, "from", GOLDEN, *CHAIN, "spreads", "-width", str(W), "-pool", "3", "-range", bad, str(tmp_path / "p"))
        assert r.returncode != 0 and b"spreads -range takes lo:hi with lo < hi" in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []
