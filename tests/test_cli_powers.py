"""The CLI's `powers` sink: the RMS-trace picture PREFIX.sr{rate}.w{W}x{rows}.rms.pgm of the README's FSK chain against the integer
referee's rms (test_power_cpu) of the oracle's spark_fft norms; fused (qd_plan_power), through the iterator chain (qd_power_fold +
qd_power_finish) and split over -gpus 2 the same bytes; -pool / -count, -range and the refusal of an existing file.  The tests that
compute start the CLI, which opens the GPU; this process never does."""
import os

import numpy as np
import pytest

from test_cli_peaks import CHAIN, GOLDEN, RATE, W, cli, explained, norms, pixels, read_pgm, run  # noqa: F401  (cli, norms: fixtures)
from test_power_cpu import ref_power


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_powers_fused_unfused_and_two_gpus(cli, norms, tmp_path):
    S, count = 8, 40
    ref = norms[S]
    n = ref.shape[0]
    pool = max(1, -(-n // count))
    rows = -(-n // pool)
    assert pool > 1 and n % pool                   # several windows a row, and a ragged last one
    want = pixels(ref_power(ref, pool)[0])
    pics = {}
    for tag, pre, env in (("fused", [], None), ("iter", [], {"QUADRS_HIP_NO_FUSE": "1"}), ("two", ["-gpus", "2"], None)):
        prefix = str(tmp_path / tag)
        r = run(cli, *pre, "from", GOLDEN, *CHAIN, "powers", "-width", str(W), "-stride", str(S), "-count", str(count), prefix, env=env)
        assert r.returncode == 0 and r.stdout == b"", (tag, r.stderr)
        name = f"{tag}.sr{RATE}.w{W}x{rows}.rms.pgm"
        assert name in os.listdir(tmp_path) and len(os.listdir(tmp_path)) == len(pics) + 1, os.listdir(tmp_path)
        pics[tag] = read_pgm(str(tmp_path / name))
        assert pics[tag].shape == (rows, W)
        assert explained(pics[tag], want, pool, S, n)
    for tag in ("iter", "two"):
        assert pics[tag].tobytes() == pics["fused"].tobytes(), tag
    assert pics["fused"].any()
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", GOLDEN, *CHAIN, "powers", "-width", str(W), "-stride", str(S), "-count", str(count), str(tmp_path / "fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_powers_count_pool_and_range(cli, norms, tmp_path):
    # -width 64 -count 40 at the default stride: fewer windows than rows asked for, so pool = 1 and the picture is the norms' own
    ref = norms[64]
    n = ref.shape[0]
    assert n < 40
    prefix = str(tmp_path / "plain")
    r = run(cli, "from", GOLDEN, *CHAIN, "powers", "-width", str(W), "-count", "40", prefix)
    assert r.returncode == 0, r.stderr
    assert os.listdir(tmp_path) == [f"plain.sr{RATE}.w{W}x{n}.rms.pgm"]
    pic = read_pgm(f"{prefix}.sr{RATE}.w{W}x{n}.rms.pgm")
    assert explained(pic, pixels(ref), 1, 64, n)
    # -pool 7 with a range inside the spread of this chain's rms rows
    S, pool, rng = 16, 7, (0.006, 0.02)
    ref = norms[S]
    n = ref.shape[0]
    rows = -(-n // pool)
    prefix = str(tmp_path / "ranged")
    r = run(cli, "from", GOLDEN, *CHAIN, "powers", "-width", str(W), "-stride", str(S), "-pool", str(pool), "-range", "0.006:0.02", prefix)
    assert r.returncode == 0, r.stderr
    rms = ref_power(ref, pool)[0]
    got = read_pgm(f"{prefix}.sr{RATE}.w{W}x{rows}.rms.pgm")
    assert explained(got, pixels(rms, rng), pool, S, n)
    assert 0 < (pixels(rms, rng) == 255).mean() < 1 and (pixels(rms, rng) == 0).any()     # the range saturates at both ends
    assert (got != pixels(rms)).any()                                                      # ... and is not the default rule
    # -count R is -pool ceil(windows / R)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert run(cli, "from", GOLDEN, *CHAIN, "powers", "-width", str(W), "-stride", str(S), "-count", str(rows), a).returncode == 0
    assert run(cli, "from", GOLDEN, *CHAIN, "powers", "-width", str(W), "-stride", str(S), "-pool", str(-(-n // rows)), b).returncode == 0
    tail = f".sr{RATE}.w{W}x{-(-n // -(-n // rows))}.rms.pgm"
    assert open(a + tail, "rb").read() == open(b + tail, "rb").read()


def test_powers_grammar(cli):
    r = run(cli, "-parse-only", "from", GOLDEN, "powers", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"powers width=128 stride=128 count=2048 range=no"
    r = run(cli, "-parse-only", "from", GOLDEN, "powers", "-width", "64", "-stride", "16", "-pool", "3", "-range", "0:1", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"powers width=64 stride=16 pool=3 range=yes"
    assert run(cli, "-parse-only", "from", GOLDEN, "powers", "-pool", "3", "-count", "4", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "powers", "-pool", "0", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "powers", "-floor", "yes", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "powers").returncode == 2
    u = run(cli)
    assert u.returncode == 2 and b"   powers [-width 128] [-stride =width] (-pool WINDOWS | -count 2048) [-range MIN:MAX] FILENAME_PREFIX" in u.stderr
