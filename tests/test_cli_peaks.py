"""The CLI's `peaks` sink: the max-hold picture PREFIX.sr{rate}.w{W}x{rows}.peak.pgm (and .floor.pgm) of the README's FSK chain against
the oracle's spark_fft norms folded in numpy; fused (qd_plan_pool), through the iterator chain (qd_pool_fold) and split over -gpus 2 the
same bytes; -pool / -count, -range, -floor and the refusal of an existing file.  The tests that compute start the CLI, which opens the
GPU; this process never does."""
import os
import subprocess

import numpy as np
import pytest

from test_pool_cpu import np_pool
from util import explain_check

SR = 21_000_000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsk-example-head65536.sr21M.cf32")
CHAIN = ["shift", "280000", "lowpass", "-power", "200", "-decimate", "32", "200000"]      # the README's FSK example
STAGES = [("shift", 280000), ("lowpass", (200000, 32, 400))]
RATE = SR // 32
W = 64
F32 = np.float32


@pytest.fixture(scope="module")
def cli():
    from quadrs_amd import build as B
    B.build()
    return B.build_cli()


def run(cli, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([cli, *args], capture_output=True, env=e, timeout=300)


def sat_u8(v):
    """Rust's `as u8` of an f32: truncation, saturating, NaN -> 0"""
    v = np.where(np.isnan(v), F32(0), v)
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def pixels(rows, rng=None):
    rows = rows.astype(F32)
    if rng is None:
        return sat_u8(rows / F32(10.0) * F32(256.0))
    lo, hi = F32(rng[0]), F32(rng[1])
    with np.errstate(invalid="ignore"):
        return sat_u8((rows - lo) / (hi - lo) * F32(256.0))


def read_pgm(path):
    raw = open(path, "rb").read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    assert magic == b"P5" and maxval == b"255" and len(body) == w * h, (magic, dims, maxval, len(body))
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w)


@pytest.fixture(scope="module")
def norms(oracle):
    """stride -> the oracle's norms of every window sparkfft prints behind CHAIN"""
    ch = oracle.Chain.from_bytes(open(GOLDEN, "rb").read(), oracle.FMT_CF32, SR).shift(280000).lowpass(200000, 32, 400)
    assert ch.sample_rate() == RATE
    return {S: ch.spark_fft(W, S, want_codes=False)[0] for S in (8, 16, 64)}


def explained(pic, want, pool, S, n):
    """a row of the picture may differ from the oracle's only where the NCO rule explains one of the windows it folds; none expected"""
    for r in np.nonzero((pic != want).any(axis=1))[0]:
        group = range(int(r) * pool, min((int(r) + 1) * pool, n))
        assert any(not explain_check((STAGES, W, S, SR), np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8), w) for w in group), \
            (int(r), "a differing row folds no window that reads an ambiguous NCO multiplier")
    return True


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_peaks_fused_unfused_and_two_gpus(cli, norms, tmp_path):
    S, count = 8, 40
    ref = norms[S]
    n = ref.shape[0]
    pool = max(1, -(-n // count))
    rows = -(-n // pool)
    assert pool > 1 and n % pool                   # several windows a row, and a ragged last one
    want = [pixels(a) for a in np_pool(ref, pool)]
    pics = {}
    for tag, pre, env in (("fused", [], None), ("iter", [], {"QUADRS_HIP_NO_FUSE": "1"}), ("two", ["-gpus", "2"], None)):
        prefix = str(tmp_path / tag)
        r = run(cli, *pre, "from", GOLDEN, *CHAIN, "peaks", "-width", str(W), "-stride", str(S), "-count", str(count), "-floor", "yes", prefix, env=env)
        assert r.returncode == 0 and r.stdout == b"", (tag, r.stderr)
        stem = f"{prefix}.sr{RATE}.w{W}x{rows}"
        assert sorted(os.listdir(tmp_path))[-2:] == sorted(os.path.basename(stem) + e for e in (".floor.pgm", ".peak.pgm")), os.listdir(tmp_path)
        pics[tag] = [read_pgm(stem + ".peak.pgm"), read_pgm(stem + ".floor.pgm")]
        for which in (0, 1):
            assert pics[tag][which].shape == (rows, W)
            assert explained(pics[tag][which], want[which], pool, S, n)
    for tag in ("iter", "two"):
        assert pics[tag][0].tobytes() == pics["fused"][0].tobytes() and pics[tag][1].tobytes() == pics["fused"][1].tobytes(), tag
    assert pics["fused"][0].any() and (pics["fused"][0] >= pics["fused"][1]).all()
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", GOLDEN, *CHAIN, "peaks", "-width", str(W), "-stride", str(S), "-count", str(count), str(tmp_path / "fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_peaks_count_pool_range_and_floor(cli, norms, tmp_path):
    # -width 64 -count 40 at the default stride: fewer windows than rows asked for, so pool = 1 and the picture is the norms' own
    ref = norms[64]
    n = ref.shape[0]
    assert n < 40
    prefix = str(tmp_path / "plain")
    r = run(cli, "from", GOLDEN, *CHAIN, "peaks", "-width", str(W), "-count", "40", prefix)
    assert r.returncode == 0, r.stderr
    assert os.listdir(tmp_path) == [f"plain.sr{RATE}.w{W}x{n}.peak.pgm"]                 # no floor picture unless asked for
    pic = read_pgm(f"{prefix}.sr{RATE}.w{W}x{n}.peak.pgm")
    assert explained(pic, pixels(ref), 1, 64, n)
    # -pool 7 with the range `levels` reports for this chain's scale, and the floor picture
    S, pool, rng = 16, 7, (0.001, 0.05)
    ref = norms[S]
    n = ref.shape[0]
    rows = -(-n // pool)
    prefix = str(tmp_path / "ranged")
    r = run(cli, "from", GOLDEN, *CHAIN, "peaks", "-width", str(W), "-stride", str(S), "-pool", str(pool), "-range", "0.001:0.05", "-floor", "yes", prefix)
    assert r.returncode == 0, r.stderr
    peak, floor = np_pool(ref, pool)
    got = [read_pgm(f"{prefix}.sr{RATE}.w{W}x{rows}.{k}.pgm") for k in ("peak", "floor")]
    for pic, rows_ref in zip(got, (peak, floor)):
        want = pixels(rows_ref, rng)
        assert explained(pic, want, pool, S, n)
    assert 0 < (pixels(peak, rng) == 255).mean() < 1 and (pixels(floor, rng) == 0).any()   # the range saturates at both ends
    assert (got[0] != pixels(peak)).any()                                                   # ... and is not the default rule


def test_peaks_grammar(cli):
    r = run(cli, "-parse-only", "from", GOLDEN, "peaks", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"peaks width=128 stride=128 count=2048 range=no floor=0"
    r = run(cli, "-parse-only", "from", GOLDEN, "peaks", "-width", "64", "-stride", "16", "-pool", "3", "-range", "0:1", "-floor", "yes", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"peaks width=64 stride=16 pool=3 range=yes floor=1"
    assert run(cli, "-parse-only", "from", GOLDEN, "peaks", "-pool", "3", "-count", "4", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "peaks", "-pool", "0", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "peaks").returncode == 2
    u = run(cli)
    assert u.returncode == 2 and b"   peaks [-width 128] [-stride =width] (-pool WINDOWS | -count 2048)" in u.stderr
