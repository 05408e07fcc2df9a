"""The CLI's `levels` sink: fused (qd_plan_summarize) and through the iterator chain (qd_summary_fold) print the same bytes, and the
printed floats parse back to the summary of the oracle's norms."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CUPBOARD = os.path.join(GOLDEN, "cupboard-superdec.sr400.cf32")
FSK = os.path.join(GOLDEN, "fsk-example-head65536.sr21M.cf32")
FSK_CHAIN = ["shift", "280000", "lowpass", "-power", "200", "-decimate", "32", "200000"]      # the README's FSK example
F32 = np.float32


@pytest.fixture(scope="module")
def cli(engine):
    from quadrs_amd import build as B
    return B.build_cli()


def run(cli, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([cli, *args], capture_output=True, env=e, timeout=300)


def expected(engine, rate, W, S, norms):
    """the text `levels` prints for these norms rows, from the Python summary (floats as the shortest that parse back: compared as f32)"""
    s = engine.summary_fold(norms)
    out = {"head": f"levels sample_rate={rate} width={W} stride={S} windows={norms.shape[0]}", "min": (s.min,), "max": (s.max,), "nan": s.n_nan}
    for name, q in (("q50", 0.5), ("q90", 0.9), ("q99", 0.99), ("q99.9", 0.999)):
        out[name] = s.quantile(q)
    b = int(np.argmax(s.peak))                    # the lowest index on ties
    out["peak_bin"] = (b, s.peak[b])
    return out


def check(stdout, exp):
    lines = stdout.decode().split("\n")
    assert lines[0] == exp["head"] and lines[-1] == "" and len(lines) == 10
    got = {l.split()[0]: l.split()[1:] for l in lines[1:-1]}
    assert list(got) == ["min", "max", "nan", "q50", "q90", "q99", "q99.9", "peak_bin"]
    for k in ("min", "max", "q50", "q90", "q99", "q99.9"):
        assert tuple(F32(v) for v in got[k]) == tuple(F32(v) for v in exp[k]), k
    assert int(got["nan"][0]) == exp["nan"]
    assert int(got["peak_bin"][0]) == exp["peak_bin"][0] and F32(got["peak_bin"][1]) == exp["peak_bin"][1]


def test_levels_cupboard(cli, engine, oracle, cupboard):
    sink = ["levels", "-width", "4", "-stride", "2"]
    fused = run(cli, "from", CUPBOARD, *sink)
    slow = run(cli, "from", CUPBOARD, *sink, env={"QUADRS_HIP_NO_FUSE": "1"})
    assert fused.returncode == 0 and slow.returncode == 0, (fused.stderr, slow.stderr)
    assert fused.stdout == slow.stdout
    norms = oracle.Chain.from_bytes(cupboard, oracle.FMT_CF32, 400).spark_fft(4, 2, want_codes=False)[0]
    check(fused.stdout, expected(engine, 400, 4, 2, norms))
    two = run(cli, "-gpus", "2", "from", CUPBOARD, *sink)
    assert two.returncode == 0 and two.stdout == fused.stdout


def test_levels_readme_fsk_chain(cli, engine, oracle, fsk):
    sink = ["levels", "-width", "64", "-stride", "16"]
    fused = run(cli, "from", FSK, *FSK_CHAIN, *sink)
    slow = run(cli, "from", FSK, *FSK_CHAIN, *sink, env={"QUADRS_HIP_NO_FUSE": "1"})
    assert fused.returncode == 0 and slow.returncode == 0, (fused.stderr, slow.stderr)
    assert fused.stdout == slow.stdout
    ch = oracle.Chain.from_bytes(fsk, oracle.FMT_CF32, 21_000_000).shift(280000).lowpass(200000, 32, 400)
    check(fused.stdout, expected(engine, ch.sample_rate(), 64, 16, ch.spark_fft(64, 16, want_codes=False)[0]))
    two = run(cli, "-gpus", "2", "from", FSK, *FSK_CHAIN, *sink)
    assert two.returncode == 0 and two.stdout == fused.stdout


def test_levels_three_lowpasses_go_through_the_iterator(cli, engine, oracle, fsk):
    chain = ["lowpass", "-decimate", "4", "4M", "lowpass", "-decimate", "2", "1M", "lowpass", "-decimate", "2", "500k"]
    r = run(cli, "from", FSK, *chain, "levels", "-width", "16", "-stride", "8")
    assert r.returncode == 0, r.stderr
    ch = oracle.Chain.from_bytes(fsk, oracle.FMT_CF32, 21_000_000).lowpass(4_000_000, 4, 40).lowpass(1_000_000, 2, 40).lowpass(500_000, 2, 40)
    n = int(r.stdout.split(b"\n")[0].split(b"windows=")[1])
    assert n >= 1
    check(r.stdout, expected(engine, ch.sample_rate(), 16, 8, ch.spark_fft(16, 8, max_windows=n, want_codes=False)[0]))
    # the windows folded are the complete ones: the next one fails read_exact_at in the reference, or the loop ended
    total = (ch.len() - 16 - 1) // 8 + 1
    assert n <= total
    if n < total:
        with pytest.raises(RuntimeError):
            ch.spark_fft(16, 8, max_windows=n + 1, want_codes=False)


def test_levels_grammar(cli):
    r = run(cli, "-parse-only", "from", CUPBOARD, "levels", "-width", "4", "-stride", "2")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"levels width=4 stride=2"
    r = run(cli, "-parse-only", "from", CUPBOARD, "levels")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"levels width=128 stride=128"
    assert run(cli, "-parse-only", "from", CUPBOARD, "levels", "-range", "0:1").returncode == 2
    u = run(cli)
    assert u.returncode == 2 and b"  levels [-width 128] [-stride =width]" in u.stderr
