"""The CLI's `marks` sink on the README's OOK capture: fused and through the iterator chain, and -scan against a Python
restatement of bits::scan (tests/test_bits_scan_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

from test_bits_scan_cpu import scan

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CUPBOARD = os.path.join(GOLDEN, "cupboard-superdec.sr400.cf32")
SINK = ["marks", "-width", "4", "-stride", "2", "-min", "0.001"]


@pytest.fixture(scope="module")
def cli(engine):
    from quadrs_amd import build as B
    return B.build_cli()


def run(cli, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([cli, *args], capture_output=True, env=e, timeout=300)


def test_marks_fused_and_iterator(cli, engine, cupboard):
    fused = run(cli, "from", CUPBOARD, *SINK)
    slow = run(cli, "from", CUPBOARD, *SINK, env={"QUADRS_HIP_NO_FUSE": "1"})
    assert fused.returncode == 0 and slow.returncode == 0, (fused.stderr, slow.stderr)
    assert fused.stdout == slow.stdout
    marks = engine.Plan(0, 400, len(cupboard) // 8, width=4, stride=2, epilogue=engine.EPI_MARK_U8, rng=(0.001, 1.0)).run_host(cupboard)
    assert fused.stdout == "".join(str(int(m)) for m in marks).encode() + b"\n"
    assert 0 < marks.mean() < 1
    two = run(cli, "-gpus", "2", "from", CUPBOARD, *SINK)
    assert two.returncode == 0 and two.stdout == fused.stdout


def test_marks_scan(cli, engine, cupboard):
    marks = engine.Plan(0, 400, len(cupboard) // 8, width=4, stride=2, epilogue=engine.EPI_MARK_U8, rng=(0.001, 1.0)).run_host(cupboard)
    status, error, bits = scan(marks, 8.0)
    fused = run(cli, "from", CUPBOARD, *SINK, "-scan", "8")
    slow = run(cli, "from", CUPBOARD, *SINK, "-scan", "8", env={"QUADRS_HIP_NO_FUSE": "1"})
    assert fused.stdout == slow.stdout and fused.returncode == slow.returncode
    if status == "ok":
        assert fused.returncode == 0, fused.stderr
        lines = fused.stdout.split(b"\n")
        assert lines[0] == "".join(str(int(b)) for b in bits).encode()
        assert float(lines[1]) == error
    else:                                   # the reference's loop never terminates on this stream: exit 1, the library's message
        assert fused.returncode == 1 and b"src/bits.rs:9-15" in fused.stderr and fused.stdout == b""


def test_marks_grammar(cli):
    r = run(cli, "-parse-only", "from", CUPBOARD, "marks", "-width", "4", "-stride", "2", "-min", "0.001", "-scan", "8")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"marks width=4 stride=2 min=yes scan=yes"
    assert run(cli, "-parse-only", "from", CUPBOARD, "marks", "-scan", "0").returncode == 2
    assert run(cli, "-parse-only", "from", CUPBOARD, "marks", "-range", "0:1").returncode == 2
