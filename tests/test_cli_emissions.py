"""The CLI's `emissions` sink: PREFIX.sr{rate}.w{W}.emissions and the printed records of the README's two chains against
engine.emissions_of of the plan's own norms (which a fresh Python process fetches: this one never opens the GPU; test_gpu_pool holds
those norms to the oracle); fused (qd_plan_emissions) and through the iterator chain (qd_emissions_fold, qd_emissions_finish) the same
bytes; -level, -levels FILE, -times, -min, -cells, -cap below found, -print with its seconds and Hz, -window bh; the grammar and the
-gpus message."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_cli_bands import CUPBOARD, FSK, README, ROOT, plan_norms
from test_cli_peaks import cli, run  # noqa: F401  (cli: fixture)
from test_emissions_cpu import EMISSION

F32 = np.float32

FETCH_BH = """
import sys
import numpy as np
sys.path.insert(0, %r)
import quadrs_amd as Q
path, rate, stages, W, S, out = %r
data = open(path, "rb").read()
kw = dict(stages=stages) if stages else {}
plan = Q.Plan(Q.FMT_CF32, rate, len(data) // 8, width=W, stride=S, windowing=Q.WINDOW_BH, **kw)
np.save(out, plan.run_host(data, n_windows=plan.complete_windows()))
"""


def printed(lst, k, rate, W, S):
    """the two lines of each of the first k records: the fields, then seconds and Hz worked out here from the record and the rates"""
    out = []
    for r in lst[:k]:
        out.append(b"%d %d %d %d %d %d %d %s %d" % (r["first"], r["last"], r["lo"], r["hi"], r["cells"], r["peak_at"], r["peak_bin"], b"%.9g" % r["peak"], r["flags"]))
        t0, t1 = int(r["first"]) * S / rate, (int(r["last"]) * S + W) / rate
        f0, f1 = (int(r["lo"]) - W / 2) * rate / W, (int(r["hi"]) + 1 - W / 2) * rate / W
        out.append(b"  %s s ... %s s, %s Hz ... %s Hz" % tuple(b"%.9g" % x for x in (t0, t1, f0, f1)))
    return out


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
@pytest.mark.parametrize("name", ["cupboard", "fsk"])
def test_readme_chains_fused_and_unfused(cli, engine, tmp_path, name):
    path, file_rate, chain, stages, rate, W, S = README[name]
    norms = plan_norms(tmp_path, name)
    n = norms.shape[0]
    assert n >= 20 and norms.shape[1] == W
    median = np.nanmedian(norms, axis=0).astype(F32)
    level = F32(np.quantile(norms.astype(np.float64), 0.9))
    floor_file = str(tmp_path / "floor.f32")
    median.tofile(floor_file)
    full = engine.emissions_of(norms, median * F32(1.5), 2, 3, cap=n * W)
    assert full[1] > 4
    small = full[1] - 2
    cases = {
        "level": (["-level", repr(float(level))], engine.emissions_of(norms, level, cap=n * W), 0),
        "levels": (["-levels", floor_file, "-times", "1.5", "-min", "2", "-cells", "3", "-print", "3"], full, 3),
        "cap": (["-levels", floor_file, "-times", "1.5", "-min", "2", "-cells", "3", "-cap", str(small), "-print", str(small + 5)],
                engine.emissions_of(norms, median * F32(1.5), 2, 3, cap=small), small),
        "count": (["-level", repr(float(level)), "-cap", "0", "-print", "2"], engine.emissions_of(norms, level, cap=0), 0),
    }
    for tag, (words, (lst, found), shown) in cases.items():
        assert found > 0, tag
        got = {}
        for how, env in (("fused", None), ("iter", {"QUADRS_HIP_NO_FUSE": "1"})):
            prefix = str(tmp_path / f"{tag}_{how}")
            r = run(cli, "from", path, *chain, "emissions", "-width", str(W), "-stride", str(S), *words, prefix, env=env)
            assert r.returncode == 0, (tag, how, r.stderr)
            lines = r.stdout.split(b"\n")
            min_len, min_cells = (2, 3) if "-min" in words else (1, 1)
            assert lines[0] == b"emissions width=%d stride=%d min=%d cells=%d windows=%d found=%d written=%d" % (W, S, min_len, min_cells, n, found, lst.size), lines[0]
            assert lines[1:] == printed(lst, shown, rate, W, S) + [b""], (tag, how, lines[1:5])
            got[how] = open(f"{prefix}.sr{rate}.w{W}.emissions", "rb").read()
            assert sorted(f for f in os.listdir(tmp_path) if f.startswith(f"{tag}_{how}.")) == [f"{tag}_{how}.sr{rate}.w{W}.emissions"]
        assert got["fused"] == lst.tobytes(), tag
        assert got["iter"] == got["fused"], tag
    assert cases["cap"][1][1] == full[1] and cases["cap"][1][0].tobytes() == full[0][:small].tobytes()
    kept = np.frombuffer(open(str(tmp_path / f"levels_fused.sr{rate}.w{W}.emissions"), "rb").read(), dtype=EMISSION)
    assert (kept["last"] - kept["first"] + 1).min() >= 2 and kept["cells"].min() >= 3
    # -window bh: the norms of the windowed plan
    out = str(tmp_path / "bh.npy")
    r = subprocess.run([sys.executable, "-c", FETCH_BH % (ROOT, (path, file_rate, stages, W, S, out))], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    bh = np.load(out)
    level_bh = F32(np.quantile(bh.astype(np.float64), 0.9))                # the window lowers every norm: a level of its own
    lst, found = engine.emissions_of(bh, level_bh, cap=n * W)
    assert found > 0 and lst.tobytes() != engine.emissions_of(norms, level_bh, cap=n * W)[0].tobytes()
    for how, env in (("fused", None), ("iter", {"QUADRS_HIP_NO_FUSE": "1"})):
        prefix = str(tmp_path / f"bh_{how}")
        r = run(cli, "from", path, *chain, "emissions", "-width", str(W), "-stride", str(S), "-level", repr(float(level_bh)), "-window", "bh", prefix, env=env)
        assert r.returncode == 0, (how, r.stderr)
        assert open(f"{prefix}.sr{rate}.w{W}.emissions", "rb").read() == lst.tobytes(), how
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", path, *chain, "emissions", "-width", str(W), "-stride", str(S), "-level", "1", str(tmp_path / "level_fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr
    # a thresholds file of another width
    r = run(cli, "from", path, *chain, "emissions", "-width", str(2 * W), "-levels", floor_file, str(tmp_path / "wrong"))
    assert r.returncode == 1 and b"exactly %d f32 values" % (2 * W) in r.stderr, r.stderr
    # an inadmissible threshold is the library's refusal
    r = run(cli, "from", path, *chain, "emissions", "-width", str(W), "-stride", str(S), "-level", "1", "-times", "-2", str(tmp_path / "neg"))
    assert r.returncode == 1 and b"threshold" in r.stderr and not os.path.exists(str(tmp_path / f"neg.sr{rate}.w{W}.emissions")), r.stderr


def test_emissions_grammar(cli):
    base = ("-parse-only", "from", FSK, "emissions")
    r = run(cli, *base, "-level", "0.25", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"emissions width=128 stride=128 level=0.25 times=1 min=1 cells=1 cap=1048576 print=0", r.stdout
    r = run(cli, *base, "-width", "64", "-stride", "16", "-levels", "floor.f32", "-times", "3", "-min", "4", "-cells", "9", "-cap", "10", "-print", "7", "-window", "bh", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1:3] == [b"emissions width=64 stride=16 levels=floor.f32 times=3 min=4 cells=9 cap=10 print=7", b"window=bh"], r.stdout
    assert run(cli, *base, "-level", "inf", "-cap", "0", "P").returncode == 0
    assert run(cli, *base, "P").returncode == 2                                       # -level or -levels
    assert run(cli, *base, "-level", "1").returncode == 2                             # the prefix
    assert run(cli, *base, "-level", "1", "-levels", "F", "P").returncode == 2
    assert run(cli, *base, "-level", "loud", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-times", "k", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-min", "0", "P").returncode == 2
    r = run(cli, *base, "-level", "1", "-cells", "0", "P")
    assert r.returncode == 2 and b"-cells takes a number of cells > 0" in r.stderr
    limit = (1 << 30) // 56
    r = run(cli, *base, "-level", "1", "-cap", str(limit + 1), "P")                   # a list workspace above 1 GiB
    assert r.returncode == 2 and b"-cap takes at most %d records" % limit in r.stderr
    assert run(cli, *base, "-level", "1", "-cap", str(limit), "P").returncode == 0
    assert run(cli, *base, "-level", "1", "-level", "2", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-window", "hann", "P").returncode == 2
    assert run(cli, *base, "-level", "1", "-floor", "yes", "P").returncode == 2
    assert run(cli, "-parse-only", "from", FSK, "bursts", "-level", "1", "-cells", "2", "P").returncode == 2      # -cells is the emissions verb's
    assert run(cli, "emissions", "-level", "1", "P").returncode == 1                  # no input
    u = run(cli)
    assert u.returncode == 2
    assert b"emissions [-width 128] [-stride =width] (-level X | -levels FILE) [-times K] [-min 1] [-cells 1] [-cap 1048576] [-print 0] FILENAME_PREFIX \\\n" in u.stderr
    assert b"emissions, bands, bursts and picture also take [-window bh|rect]" in u.stderr


def test_gpus_is_refused_before_any_device_is_touched(cli, tmp_path):
    for path in (CUPBOARD, FSK):
        r = run(cli, "-gpus", "2", "from", path, "emissions", "-width", "4", "-level", "1", str(tmp_path / "P"))
        assert r.returncode == 1 and b"an emission crosses the seam" in r.stderr and b"-gpus" in r.stderr, r.stderr
        assert os.listdir(tmp_path) == []
