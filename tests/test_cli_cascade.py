"""The CLI on cascaded chains (a shift after the filter, two lowpasses): one fused cascade plan, the reference's bytes."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FSK = os.path.join(GOLDEN, "fsk-example-head65536.sr21M.cf32")


@pytest.fixture(scope="module")
def cli(engine):
    from quadrs_amd import build as B
    return B.build_cli()


def run(cli, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([cli, *args], capture_output=True, env=e, timeout=300)


def _nested(O, ch, stages):
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch


L1 = ["lowpass", "-decimate", "4", "2000000"]
L2 = ["lowpass", "-power", "100", "-decimate", "8", "200000"]
ST1, ST2 = ("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200))


@pytest.mark.parametrize("name,chain,stages", [
    ("LL", L1 + L2, [ST1, ST2]),
    ("SLL", ["shift", "280000"] + L1 + L2, [("shift", 280_000), ST1, ST2]),
    ("LLS", L1 + L2 + ["shift", "20000"], [ST1, ST2, ("shift", 20_000)]),
    ("LS", ["lowpass", "-power", "200", "-decimate", "16", "2000000", "shift", "20000"], [("lowpass", (2_000_000, 16, 400)), ("shift", 20_000)]),
])
def test_cascade_from_file(cli, oracle, fsk, name, chain, stages):
    ch = _nested(oracle, oracle.Chain.from_bytes(fsk, oracle.FMT_CF32, 21_000_000), stages)
    sink = ["sparkfft", "-width", "16", "-stride", "8", "-range", "0.002:0.2"]
    r = run(cli, "from", FSK, *chain, *sink)
    assert r.returncode == 0, r.stderr
    want = ch.spark_text(16, 8, (0.002, 0.2))
    got_lines, want_lines = r.stdout.split(b"\n"), want.split(b"\n")
    assert len(got_lines) == len(want_lines) > 20 and got_lines[0] == want_lines[0]
    same = sum(a == b for a, b in zip(got_lines, want_lines))
    if any(k == "shift" for k, _ in stages):
        assert same >= len(want_lines) - 1        # a 1-ulp NCO event may flip one glyph at a bin edge
    else:
        assert r.stdout == want
        slow = run(cli, "from", FSK, *chain, *sink, env={"QUADRS_HIP_NO_FUSE": "1"})
        assert slow.returncode == 0 and slow.stdout == r.stdout
    two = run(cli, "-gpus", "2", "from", FSK, *chain, *sink)
    assert two.returncode == 0 and two.stdout == r.stdout
    # bucket
    rb = run(cli, "from", FSK, *chain, "bucket", "-width", "16", "-by", "freq", "2")
    assert rb.returncode == 0, rb.stderr
    assert rb.stdout.decode().strip() == "".join(str(int(v)) for v in ch.freq_levels(16, 16))


def test_cascade_from_gen(cli, oracle):
    chain = ["gen", "-cos", "1000", "-cos", "-3k", "-cos", "7500", "-len", "0.25", "48k",
             "lowpass", "-power", "12", "-decimate", "2", "12000", "lowpass", "-power", "12", "-decimate", "2", "4000"]
    ch = oracle.Chain.gen([1000, -3000, 7500], 48000, 0.25).lowpass(12000, 2, 24).lowpass(4000, 2, 24)
    for sink in (["sparkfft", "-width", "16", "-stride", "8", "-range", "0.02:3"], ["bucket", "-width", "32", "-by", "freq", "2"]):
        fused = run(cli, *chain, *sink)
        slow = run(cli, *chain, *sink, env={"QUADRS_HIP_NO_FUSE": "1"})
        assert fused.returncode == 0 and slow.returncode == 0, (fused.stderr, slow.stderr)
        assert fused.stdout == slow.stdout and len(fused.stdout) > 50
    got = run(cli, *chain, "sparkfft", "-width", "16", "-stride", "8", "-range", "0.02:3").stdout
    assert got == ch.spark_text(16, 8, (0.02, 3.0))


def test_cascade_failing_tail(cli, oracle, tmp_path):
    """20 036 samples of the probe chain: the last window's read_exact_at fails.  The complete rows are printed, then the
    reference's error, exit 1."""
    n = 20_036
    rng = np.random.default_rng(23)
    data = (0.05 * rng.standard_normal((n, 2))).astype(np.float32).tobytes()
    f = tmp_path / "probe.sr1M.cf32"
    f.write_bytes(data)
    r = run(cli, "from", str(f), "lowpass", "-decimate", "4", "100000", "lowpass", "-power", "100", "-decimate", "8", "10000",
            "sparkfft", "-width", "4", "-range", "0.0001:0.01")
    ch = oracle.Chain.from_bytes(data, oracle.FMT_CF32, 1_000_000).lowpass(100_000, 4, 40).lowpass(10_000, 8, 200)
    total = oracle.lib().qo_spark_window_count(ch.len(), 4, 4)
    _, codes = ch.spark_fft(4, 4, rng=(0.0001, 0.01), max_windows=total - 1)
    want = oracle.render(ch.sample_rate(), codes)
    assert r.returncode == 1
    assert r.stdout == want
    assert r.stderr.decode().strip().endswith(f"Error: TODO: read-exact messed up: 4 (wanted) != 3 (read) at {(total - 1) * 4}")
