"""The CLI's `picture` sink: the waterfall PREFIX.sr{rate}.w{W}.{pxw}x{pxh}.ppm of the README's FSK chain against the oracle's spark_fft
norms painted by test_picture_cpu's referee; fused (qd_plan_picture), through the iterator chain (qd_picture_fold) and split over -gpus 2
the same bytes; the defaults, -scan, the file name and the refusal of an existing file.  The tests that compute start the CLI, which opens
the GPU; this process never does."""
import os
import subprocess

import numpy as np
import pytest

from test_picture_cpu import GAP, ref_geometry, ref_picture
from util import explain_check

SR = 21_000_000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsk-example-head65536.sr21M.cf32")
CHAIN = ["shift", "280000", "lowpass", "-power", "200", "-decimate", "32", "200000"]      # the README's FSK example
STAGES = [("shift", 280000), ("lowpass", (200000, 32, 400))]
RATE = SR // 32


@pytest.fixture(scope="module")
def cli():
    from quadrs_amd import build as B
    B.build()
    return B.build_cli()


def run(cli, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([cli, *args], capture_output=True, env=e, timeout=300)


def read_ppm(path):
    raw = open(path, "rb").read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    assert magic == b"P6" and maxval == b"255" and len(body) == w * h * 3, (magic, dims, maxval, len(body))
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)                               # top row first: the buffer as it lies


@pytest.fixture(scope="module")
def norms(oracle):
    """(W, S) -> the oracle's norms of every window sparkfft prints behind CHAIN"""
    ch = oracle.Chain.from_bytes(open(GOLDEN, "rb").read(), oracle.FMT_CF32, SR).shift(280000).lowpass(200000, 32, 400)
    assert ch.sample_rate() == RATE
    return {(W, S): ch.spark_fft(W, S, want_codes=False)[0] for W, S in ((64, 16), (8, 1))}


def explained(pic, want, W, S, w, stretch):
    """a pixel may differ from the oracle's picture only where the NCO rule explains its window; none expected"""
    h = pic.shape[0]
    rh = stretch * W + GAP
    rows, cols = np.nonzero((pic != want).any(axis=2))
    for p in sorted({(h - 1 - int(r)) // rh * w + int(x) for r, x in zip(rows, cols)}):
        assert not explain_check((STAGES, W, S, SR), np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8), p), \
            (p, "a differing column's window reads no ambiguous NCO multiplier")
    return True


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_picture_fused_unfused_and_two_gpus(cli, norms, tmp_path):
    W, S, w, stretch, scan, scale = 64, 16, 50, 2, 7, 0.05
    ref = norms[(W, S)]
    n = ref.shape[0]
    rh = stretch * W + GAP
    h = 2 * rh + 70                                # three strips, the last cut inside a bin's stretch
    _, strips, max_windows = ref_geometry(W, w, h, stretch)
    assert strips == 3 and 2 * w < n < max_windows                                            # the third strip is ragged: -gpus 2 gets 2 + 1 strips
    want = ref_picture(ref, W, w, h, stretch, scan, scale)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50
    pics = {}
    for tag, pre, env in (("fused", [], None), ("iter", [], {"QUADRS_HIP_NO_FUSE": "1"}), ("two", ["-gpus", "2"], None)):
        prefix = str(tmp_path / tag)
        r = run(cli, *pre, "from", GOLDEN, *CHAIN, "picture", "-width", str(W), "-stride", str(S), "-size", f"{w}x{h}", "-stretch", str(stretch),
                "-scan", str(scan), "-scale", str(scale), prefix, env=env)
        assert r.returncode == 0, (tag, r.stderr)
        assert r.stdout == (f"picture width={W} stride={S} size={w}x{h} stretch={stretch} scan={scan} scale=0.0500000007 strips={strips} "
                            f"max_windows={max_windows} painted={n}\n").encode(), (tag, r.stdout)
        name = f"{tag}.sr{RATE}.w{W}.{w}x{h}.ppm"
        assert name in os.listdir(tmp_path), os.listdir(tmp_path)
        pics[tag] = read_ppm(str(tmp_path / name))
        assert pics[tag].shape == (h, w, 3) and explained(pics[tag], want, W, S, w, stretch)
    for tag in ("iter", "two"):
        assert pics[tag].tobytes() == pics["fused"].tobytes(), tag
    first = pics["fused"][h - stretch * W:]                                                   # the bottom strip: windows 0 ... 49
    assert not first[:, 0].any() and not first[:, 49].any() and first[:, 1].any()             # markers count windows, not columns: 0 and 49 ...
    assert not pics["fused"][h - 1 - rh - stretch * W + 1:h - rh, 6].any()                    # ... and window 56 = 50 + 6 in the second strip
    # an existing output file is refused, with the write sink's message; -overwrite yes replaces it
    args = ["from", GOLDEN, *CHAIN, "picture", "-width", str(W), "-stride", str(S), "-size", f"{w}x{h}", "-stretch", str(stretch)]
    r = run(cli, *args, str(tmp_path / "fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr
    assert read_ppm(str(tmp_path / f"fused.sr{RATE}.w{W}.{w}x{h}.ppm")).tobytes() == pics["fused"].tobytes()
    r = run(cli, *args, "-overwrite", "yes", str(tmp_path / "fused"))
    assert r.returncode == 0, r.stderr
    again = read_ppm(str(tmp_path / f"fused.sr{RATE}.w{W}.{w}x{h}.ppm"))
    assert explained(again, ref_picture(ref, W, w, h, stretch, 0, 2.29), W, S, w, stretch)


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_picture_defaults_and_scan(cli, norms, tmp_path):
    # only -size: the reference's Params (-width 8 -stride 1 -stretch 4), its scale 2.29, and no marker columns
    ref = norms[(8, 1)]
    n = ref.shape[0]
    w, h = 300, 100                                # row_height 48: three strips, 900 windows looked at
    assert n > 900
    prefix = str(tmp_path / "plain")
    r = run(cli, "from", GOLDEN, *CHAIN, "picture", "-size", f"{w}x{h}", prefix)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"picture width=8 stride=1 size=300x100 stretch=4 scan=0 scale=2.28999996 strips=3 max_windows=900 painted=900\n"
    assert os.listdir(tmp_path) == [f"plain.sr{RATE}.w8.{w}x{h}.ppm"]
    pic = read_ppm(f"{prefix}.sr{RATE}.w8.{w}x{h}.ppm")
    assert explained(pic, ref_picture(ref, 8, w, h, 4, 0, 2.29), 8, 1, w, 4)
    assert not pic[h - 48:h - 32].any() and not pic[h - 96:h - 80].any()                      # the gaps above the first and the second strip
    assert (pic[0] == pic[3]).all()                                                           # the third strip shows bin 0's four rows
    # -scan 1, the reference's default, blackens every column
    r = run(cli, "from", GOLDEN, *CHAIN, "picture", "-size", f"{w}x{h}", "-scan", "1", str(tmp_path / "black"))
    assert r.returncode == 0, r.stderr
    assert not read_ppm(str(tmp_path / f"black.sr{RATE}.w8.{w}x{h}.ppm")).any()


def test_picture_grammar(cli):
    r = run(cli, "-parse-only", "from", GOLDEN, "picture", "-size", "640x480", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"picture width=8 stride=1 size=640x480 stretch=4 scan=0 scale=2.28999996 overwrite=0"
    r = run(cli, "-parse-only", "from", GOLDEN, "picture", "-width", "64", "-stride", "16", "-size", "101x77", "-stretch", "3", "-scan", "7", "-scale", "0.5",
            "-overwrite", "yes", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"picture width=64 stride=16 size=101x77 stretch=3 scan=7 scale=0.5 overwrite=1"
    assert run(cli, "-parse-only", "from", GOLDEN, "picture", "P").returncode == 2            # -size is required
    for bad in ("640", "0x480", "640x0", "x480", "640x", "axb"):
        assert run(cli, "-parse-only", "from", GOLDEN, "picture", "-size", bad, "P").returncode == 2, bad
    assert run(cli, "-parse-only", "from", GOLDEN, "picture", "-size", "4x4", "-stretch", "0", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "picture", "-size", "4x4", "-scale", "0", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "picture", "-size", "4x4", "-bogus", "1", "P").returncode == 2
    assert run(cli, "-parse-only", "from", GOLDEN, "picture", "-size", "4x4").returncode == 2
    u = run(cli)
    assert u.returncode == 2 and b" picture [-width 8] [-stride 1] -size PXWxPXH [-stretch 4] [-scan 0] [-scale 2.29] [-overwrite no]" in u.stderr
