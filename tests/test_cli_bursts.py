"""The CLI's `bursts` sink: PREFIX.sr{rate}.w{W}.bursts / .on.u64 and the printed records of the README's two chains against
engine.bursts_of of the plan's own norms (which a fresh Python process fetches: this one never opens the GPU); fused (qd_plan_bursts) and
through the iterator chain (qd_bursts_fold, qd_bursts_finish) the same bytes; -level, -levels FILE, -times, -min, -cap below found,
-print; the grammar and the -gpus message."""
import os

import numpy as np
import pytest

from test_bursts_cpu import BURST
from test_cli_bands import CUPBOARD, FSK, README, plan_norms
from test_cli_peaks import cli, run  # noqa: F401  (cli: fixture)

F32 = np.float32


def files(prefix, rate, W):
    stem = f"{prefix}.sr{rate}.w{W}"
    return open(stem + ".bursts", "rb").read(), open(stem + ".on.u64", "rb").read()


def printed(lst, k):
    return [b"%d %d %d %d %s" % (r["first"], r["length"], r["bin"], r["peak_at"], (b"%.9g" % r["peak"])) for r in lst[:k]]


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
@pytest.mark.parametrize("name", ["cupboard", "fsk"])
def test_readme_chains_fused_and_unfused(cli, engine, tmp_path, name):
    path, _, chain, _, rate, W, S = README[name]
    norms = plan_norms(tmp_path, name)
    n = norms.shape[0]
    assert n >= 20 and norms.shape[1] == W
    median = np.nanmedian(norms, axis=0).astype(F32)
    level = F32(np.quantile(norms.astype(np.float64), 0.9))
    floor_file = str(tmp_path / "floor.f32")
    median.tofile(floor_file)
    full = engine.bursts_of(norms, median * F32(1.5), 2, cap=n * W)
    assert full[1] > 4
    small = full[1] - 2
    cases = {
        "level": (["-level", repr(float(level))], engine.bursts_of(norms, level, 1, cap=n * W), 0),
        "levels": (["-levels", floor_file, "-times", "1.5", "-min", "2", "-print", "3"], full, 3),
        "cap": (["-levels", floor_file, "-times", "1.5", "-min", "2", "-cap", str(small), "-print", str(small + 5)],
                engine.bursts_of(norms, median * F32(1.5), 2, cap=small), small),
        "count": (["-level", repr(float(level)), "-cap", "0", "-print", "2"], engine.bursts_of(norms, level, 1, cap=0), 0),
    }
    for tag, (words, (lst, found, counts), shown) in cases.items():
        assert found > 0, tag
        got = {}
        for how, env in (("fused", None), ("iter", {"QUADRS_HIP_NO_FUSE": "1"})):
            prefix = str(tmp_path / f"{tag}_{how}")
            r = run(cli, "from", path, *chain, "bursts", "-width", str(W), "-stride", str(S), *words, prefix, env=env)
            assert r.returncode == 0, (tag, how, r.stderr)
            lines = r.stdout.split(b"\n")
            min_len = 2 if "-min" in words else 1
            assert lines[0] == b"bursts width=%d stride=%d min=%d windows=%d found=%d written=%d" % (W, S, min_len, n, found, lst.size), lines[0]
            assert lines[1:] == printed(lst, shown) + [b""], (tag, how)
            got[how] = files(prefix, rate, W)
            assert sorted(f for f in os.listdir(tmp_path) if f.startswith(f"{tag}_{how}.")) == \
                [f"{tag}_{how}.sr{rate}.w{W}.bursts", f"{tag}_{how}.sr{rate}.w{W}.on.u64"]
        assert got["fused"] == (lst.tobytes(), counts.tobytes()), tag
        assert got["iter"] == got["fused"], tag
    assert cases["cap"][1][1] == full[1] and cases["cap"][1][0].tobytes() == full[0][:small].tobytes()
    assert np.frombuffer(files(str(tmp_path / "levels_fused"), rate, W)[0], dtype=BURST)["length"].min() >= 2
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", path, *chain, "bursts", "-width", str(W), "-stride", str(S), "-level", "1", str(tmp_path / "level_fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr
    # a thresholds file of another width
    r = run(cli, "from", path, *chain, "bursts", "-width", str(2 * W), "-levels", floor_file, str(tmp_path / "wrong"))
    assert r.returncode == 1 and b"exactly %d f32 values" % (2 * W) in r.stderr, r.stderr
    # an inadmissible threshold is the library's refusal
    r = run(cli, "from", path, *chain, "bursts", "-width", str(W), "-stride", str(S), "-level", "1", "-times", "-2", str(tmp_path / "neg"))
    assert r.returncode == 1 and b"threshold" in r.stderr and not os.path.exists(str(tmp_path / f"neg.sr{rate}.w{W}.bursts")), r.stderr


def test_bursts_grammar(cli):
    base = ("-parse-only", "from", FSK, "bursts")
    r = run(cli, *base, "-level", "0.25", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"bursts width=128 stride=128 level=0.25 times=1 min=1 cap=1048576 print=0", r.stdout
    r = run(cli, *base, "-width", "64", "-stride", "16", "-levels", "floor.f32", "-times", "3", "-min", "4", "-cap", "10", "-print", "7", "-window", "bh", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1:3] == [b"bursts width=64 stride=16 levels=floor.f32 times=3 min=4 cap=10 print=7", b"window=bh"], r.stdout
    assert run(cli, *base, "-level", "inf", "-cap", "0", "P").returncode == 0
    assert run(cli, *base, "P").returncode == 2                                       # -level or -levels
    assert run(cli, *base, "-level", "1").returncode == 2                             # the prefix
    assert run(cli, *base, "-level", "1", "-levels", "F", "P").returncode == 2
    assert run(cli, *base, "-level", "loud", "P").returncode == 2
    assert run(cli, *base, "-level", "1x", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-times", "k", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-min", "0", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-cap", str((1 << 25) + 1), "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-cap", str(1 << 25), "P").returncode == 0
    assert run(cli, *base, "-level", "1", "-level", "2", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-window", "hann", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-floor", "yes", "P").returncode == 2
    assert run(cli, "bursts", "-level", "1", "P").returncode == 1                     # no input
    u = run(cli)
    assert u.returncode == 2
    assert b"  bursts [-width 128] [-stride =width] (-level X | -levels FILE) [-times K] [-min 1] [-cap 1048576] [-print 0] FILENAME_PREFIX \\\n" in u.stderr
    assert b"bands, bursts and picture also take [-window bh|rect]" in u.stderr


def test_gpus_is_refused_before_any_device_is_touched(cli, tmp_path):
    for path in (CUPBOARD, FSK):
        r = run(cli, "-gpus", "2", "from", path, "bursts", "-width", "4", "-level", "1", str(tmp_path / "P"))
        assert r.returncode == 1 and b"a run crosses the seam" in r.stderr and b"-gpus" in r.stderr, r.stderr
        assert os.listdir(tmp_path) == []
