"""The CLI's `bands` sink: PREFIX.sr{rate}.w{W}.k{K}.level.f32 / .peak_bin.u32 and the -pick line of the README's two chains against
qd_bands_fold of the plan's own norms (which a fresh Python process fetches: this one never opens the GPU); fused (qd_plan_bands),
through the iterator chain (qd_bands_fold) and split over -gpus 2 | 3 the same bytes; a chain the library does not fuse; the grammar."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_cli_peaks import cli, run  # noqa: F401  (cli: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CUPBOARD = os.path.join(GOLDEN, "cupboard-superdec.sr400.cf32")
FSK = os.path.join(GOLDEN, "fsk-example-head65536.sr21M.cf32")
F32 = np.float32
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"

# the README's examples: (file, sample rate, the chain's words, the engine's stage list, rate after the chain, width, stride)
README = {
    "cupboard": (CUPBOARD, 400, [], [], 400, 4, 2),
    "fsk": (FSK, 21_000_000, ["shift", "280000", "lowpass", "-decimate", "4", "2000000", "lowpass", "-power", "100", "-decimate", "8", "200000"],
            [("shift", 280000), ("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200))], 21_000_000 // 32, 16, 16),
}

FETCH = """
import sys
import numpy as np
sys.path.insert(0, %r)
import quadrs_amd as Q
path, rate, stages, W, S, out = %r
data = open(path, "rb").read()
plan = Q.Plan(Q.FMT_CF32, rate, len(data) // 8, stages=stages, width=W, stride=S) if stages else Q.Plan(Q.FMT_CF32, rate, len(data) // 8, width=W, stride=S)
np.save(out, plan.run_host(data, n_windows=plan.complete_windows()))
"""


def plan_norms(tmp_path, name):
    """the norms of the chain's complete windows by qd_plan_run, from a process of its own"""
    path, rate, _, stages, _, W, S = README[name]
    out = str(tmp_path / (name + ".norms.npy"))
    r = subprocess.run([sys.executable, "-c", FETCH % (ROOT, (path, rate, stages, W, S, out))], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.load(out)


def files(prefix, rate, W, K):
    stem = f"{prefix}.sr{rate}.w{W}.k{K}"
    return open(stem + ".level.f32", "rb").read(), open(stem + ".peak_bin.u32", "rb").read()


def digits(pick):
    return "".join("." if p == 255 else DIGITS[p] for p in pick).encode()


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
@pytest.mark.parametrize("name", ["cupboard", "fsk"])
def test_readme_chains_fused_unfused_and_split(cli, engine, tmp_path, name):
    path, _, chain, _, rate, W, S = README[name]
    norms = plan_norms(tmp_path, name)
    n = norms.shape[0]
    assert n >= 20 and norms.shape[1] == W
    ragged = [(0, W // 2 + 1), (1, 2), (W // 4, W), (1, 2)]
    for tag, words, bands in (("split", ["-split", "2", "-pick"], [(0, W // 2), (W // 2, W)]),
                              ("bins", ["-bins", ",".join("%d:%d" % b for b in ragged)], ragged)):
        level, _, _, _, peak_bin, pick = engine.bands_fold(norms, bands)
        K = len(bands)
        got = {}
        hows = [("fused", [], None), ("iter", [], {"QUADRS_HIP_NO_FUSE": "1"}), ("two", ["-gpus", "2"], None)]
        for how, pre, env in hows + ([("three", ["-gpus", "3"], None)] if tag == "split" else []):
            prefix = str(tmp_path / f"{tag}_{how}")
            r = run(cli, *pre, "from", path, *chain, "bands", "-width", str(W), "-stride", str(S), *words, prefix, env=env)
            assert r.returncode == 0, (tag, how, r.stderr)
            lines = r.stdout.split(b"\n")
            assert lines[0] == b"bands width=%d stride=%d k=%d windows=%d" % (W, S, K, n), lines[0]
            assert lines[1:] == ([digits(pick), b""] if tag == "split" else [b""]), (tag, how)
            got[how] = files(prefix, rate, W, K)
            assert sorted(f for f in os.listdir(tmp_path) if f.startswith(f"{tag}_{how}.")) == \
                [f"{tag}_{how}.sr{rate}.w{W}.k{K}.level.f32", f"{tag}_{how}.sr{rate}.w{W}.k{K}.peak_bin.u32"]
        assert got["fused"] == (level.tobytes(), peak_bin.tobytes()), tag
        for how in got:
            assert got[how] == got["fused"], (tag, how)
        if tag == "split" and name == "fsk":
            assert set(pick) == {0, 1}                                   # both tones are there
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", path, *chain, "bands", "-width", str(W), "-stride", str(S), "-split", "2", str(tmp_path / "split_fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_a_chain_the_library_refuses_goes_through_the_iterator(cli, engine, oracle, tmp_path):
    """three lowpass stages are no fused shape (QD_ERR_UNSUPPORTED from qd_plan_create_stages): the verb pulls the windows through the
    iterator chain and qd_bands_fold.  Without a shift the oracle's norms are the engine's exactly."""
    chain = ["lowpass", "-decimate", "2", "4000000", "lowpass", "-decimate", "2", "2000000", "lowpass", "-decimate", "2", "1000000"]
    with pytest.raises(engine.QuadrsError) as e:
        engine.stages_geometry(engine.FMT_CF32, 21_000_000, 65536, [("lowpass", (4_000_000, 2, 40)), ("lowpass", (2_000_000, 2, 40)), ("lowpass", (1_000_000, 2, 40))],
                               width=32, stride=32)
    assert e.value.code == engine._ffi.ERR_UNSUPPORTED
    W, K, rate = 32, 4, 21_000_000 // 8
    prefix = str(tmp_path / "three")
    r = run(cli, "from", FSK, *chain, "bands", "-width", str(W), "-split", str(K), "-pick", prefix)
    assert r.returncode == 0, r.stderr
    ch = oracle.Chain.from_bytes(open(FSK, "rb").read(), oracle.FMT_CF32, 21_000_000)
    ch = ch.lowpass(4_000_000, 2, 40).lowpass(2_000_000, 2, 40).lowpass(1_000_000, 2, 40)
    norms = ch.spark_fft(W, W, want_codes=False)[0]
    bands = [(k * W // K, (k + 1) * W // K) for k in range(K)]
    level, _, _, _, peak_bin, pick = engine.bands_fold(norms, bands)
    lines = r.stdout.split(b"\n")
    n = int(lines[0].rsplit(b"=", 1)[1])
    assert 20 <= n <= norms.shape[0]                       # the windows whose read succeeds: the chain's len over-reports at the tail
    assert lines[0] == b"bands width=32 stride=32 k=4 windows=%d" % n and lines[1] == digits(pick[:n])
    assert files(prefix, rate, W, K) == (level[:n].tobytes(), peak_bin[:n].tobytes())


def test_bands_grammar(cli):
    base = ("-parse-only", "from", FSK, "bands")
    r = run(cli, *base, "-split", "4", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"bands width=128 stride=128 k=4 bins=0:32,32:64,64:96,96:128 pick=0", r.stdout
    r = run(cli, *base, "-pick", "-width", "64", "-stride", "16", "-bins", "0:3,5:64,5:64", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"bands width=64 stride=16 k=3 bins=0:3,5:64,5:64 pick=1", r.stdout
    r = run(cli, *base, "-width", "64", "-bins", "0:64", "-pick", "P")                 # -pick takes no value, wherever it stands
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"bands width=64 stride=64 k=1 bins=0:64 pick=1", r.stdout
    assert run(cli, *base, "P").returncode == 2                                       # -bins or -split
    assert run(cli, *base, "-split", "4").returncode == 2                             # the prefix
    assert run(cli, *base, "-split", "4", "-bins", "0:1", "P").returncode == 2
    assert run(cli, *base, "-split", "3", "P").returncode == 2                        # K divides W
    assert run(cli, *base, "-split", "0", "P").returncode == 2
    assert run(cli, *base, "-width", "1024", "-split", "256", "P").returncode == 2   # at most 255 bands
    assert run(cli, *base, "-split", "64", "-pick", "P").returncode == 2              # one digit a window: K <= 36
    assert run(cli, *base, "-split", "32", "-pick", "P").returncode == 0
    assert run(cli, *base, "-split", "64", "P").returncode == 0
    for bad in ("0:129", "5:5", "7:3", "0:", ":4", "04", "0:4,", "a:b", "-1:4", "0:4:8"):
        assert run(cli, *base, "-bins", bad, "P").returncode == 2, bad
    assert run(cli, *base, "-bins", ",".join(["0:1"] * 256), "P").returncode == 2
    assert run(cli, *base, "-bins", ",".join(["0:1"] * 37), "-pick", "P").returncode == 2
    assert run(cli, *base, "-split", "2", "-pick", "-pick", "P").returncode == 2
    assert run(cli, *base, "-split", "2", "-floor", "yes", "P").returncode == 2
    assert run(cli, "bands", "-split", "2", "P").returncode == 1                      # no input
    u = run(cli)
    assert u.returncode == 2
    assert b"   bands [-width 128] [-stride =width] (-bins LO:HI[,LO:HI...] | -split K) [-pick] FILENAME_PREFIX" in u.stderr
