"""The CLI's `cuts` sink: `emissions` then `cuts -list` on the burst stream of test_cuts_cpu, written to a cf32 file.  The file names, the
header, the printed cuts and every file's bytes against engine.cut_of_emission and engine.cuts_run (which a fresh Python process runs:
this one never opens the GPU); fused (one qd_cuts_run) and with QUADRS_HIP_NO_FUSE=1 (qd_unpack, qd_shift, qd_lowpass_block cut by cut)
the same files; -first-window; the grammar; the cascade and -gpus refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_cli_bands import ROOT
from test_cli_peaks import cli, run  # noqa: F401  (cli: fixture)
from test_cuts_cpu import BURST_SR, burst_stream, make_desc

W = S = 64

FETCH = """
import sys
import numpy as np
sys.path.insert(0, %r)
import quadrs_amd as Q
path, rate, cuts_file, out = %r
data = open(path, "rb").read()
cuts = np.fromfile(cuts_file, dtype=Q.CUT_DTYPE)
got = Q.cuts_run(Q.FMT_CF32, rate, len(data) // 8, data, cuts)
np.save(out, np.concatenate(got) if got else np.zeros((0, 2), np.float32))
"""


def cut_files(tmp_path, stem):
    return sorted(f for f in os.listdir(tmp_path) if f.startswith(stem + "."))


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_emissions_then_cuts(cli, engine, tmp_path):
    x = burst_stream()
    n = x.shape[0]
    path = str(tmp_path / "bursts.sr2M.cf32")
    x.tofile(path)
    r = run(cli, "from", path, "emissions", "-width", str(W), "-stride", str(S), "-level", "4", "-cells", "8", str(tmp_path / "E"))
    assert r.returncode == 0, r.stderr
    listed = str(tmp_path / f"E.sr{BURST_SR}.w{W}.emissions")
    records = np.fromfile(listed, dtype=engine.EMISSION_DTYPE)
    assert records.size == 5
    desc = make_desc(engine, BURST_SR, n, W, S)
    for fw, words in ((0, []), (3, ["-first-window", "3"])):
        cuts = np.array([engine.cut_of_emission(desc, fw, e, engine.cut_rule(1, 2, 1)) for e in records], dtype=engine.CUT_DTYPE)
        assert (cuts["count"] > 0).all() and (fw == 0 or (cuts["first"] != 0).all())
        cuts_file, out = str(tmp_path / f"cuts{fw}.bin"), str(tmp_path / f"want{fw}.npy")
        cuts.tofile(cuts_file)
        p = subprocess.run([sys.executable, "-c", FETCH % (ROOT, (path, BURST_SR, cuts_file, out))], capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr
        want = np.load(out)
        offs = np.concatenate([[0], np.cumsum(cuts["count"])]).astype(int)
        names = [f"%s.{k:06d}.sr{BURST_SR // int(c['decimate'])}.cf32" for k, c in enumerate(cuts)]
        got = {}
        for how, env in (("fused", None), ("fine", {"QUADRS_HIP_NO_FUSE": "1"})):
            stem = f"C{fw}_{how}"
            r = run(cli, "from", path, "cuts", "-width", str(W), "-stride", str(S), "-list", listed, "-guard", "1", "-oversample", "2", "-pad", "1", *words,
                    "-print", "3", str(tmp_path / stem), env=env)
            assert r.returncode == 0, (how, r.stderr)
            lines = r.stdout.split(b"\n")
            assert lines[0] == b"cuts width=%d stride=%d first_window=%d guard=1 oversample=2 taps=0 pad=1 records=5 files=5 samples=%d" % (W, S, fw, offs[-1]), lines[0]
            assert lines[1:] == [b"%d %d %d %d %d %d" % tuple(int(c[k]) for k in ("shift_hz", "lowpass_hz", "decimate", "taps", "first", "count")) for c in cuts[:3]] + [b""]
            assert cut_files(tmp_path, stem) == sorted(nm % stem for nm in names)
            got[how] = [open(str(tmp_path / (nm % stem)), "rb").read() for nm in names]
        for k in range(cuts.size):
            assert got["fused"][k] == want[offs[k]:offs[k + 1]].tobytes(), (fw, k)
            assert got["fine"][k] == got["fused"][k], (fw, k)
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", path, "cuts", "-width", str(W), "-list", listed, str(tmp_path / "C0_fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr
    # a list that is no list
    r = run(cli, "from", path, "cuts", "-width", str(W), "-list", path[:-5] + ".none", str(tmp_path / "X"))
    assert r.returncode == 1 and b"os error 2" in r.stderr, r.stderr
    open(str(tmp_path / "ragged.emissions"), "wb").write(records.tobytes()[:-3])
    r = run(cli, "from", path, "cuts", "-width", str(W), "-list", str(tmp_path / "ragged.emissions"), str(tmp_path / "X"))
    assert r.returncode == 1 and b"whole qd_emission records" in r.stderr and cut_files(tmp_path, "X") == [], r.stderr
    # a width the records do not fit is the library's refusal
    r = run(cli, "from", path, "cuts", "-width", "4", "-list", listed, str(tmp_path / "X"))
    assert r.returncode == 1 and b"record 0" in r.stderr and cut_files(tmp_path, "X") == [], r.stderr


def test_cuts_grammar_and_refusals(cli, tmp_path):
    path = str(tmp_path / "bursts.sr2M.cf32")
    burst_stream()[:4096].tofile(path)
    base = ("-parse-only", "from", path, "cuts")
    r = run(cli, *base, "-width", "64", "-list", "L", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"cuts width=64 stride=64 list=L first_window=0 guard=1 oversample=2 taps=0 pad=1 print=0", r.stdout
    r = run(cli, *base, "-width", "64", "-stride", "16", "-list", "L", "-first-window", "7", "-guard", "0", "-oversample", "4", "-taps", "80", "-pad", "9", "-print", "2", "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"cuts width=64 stride=16 list=L first_window=7 guard=0 oversample=4 taps=80 pad=9 print=2", r.stdout
    assert run(cli, *base, "-list", "L", "P").returncode == 2                             # -width
    assert run(cli, *base, "-width", "64", "P").returncode == 2                           # -list
    assert run(cli, *base, "-width", "64", "-list", "L").returncode == 2                  # the prefix
    assert run(cli, *base, "-width", "64", "-list", "L", "-oversample", "0", "P").returncode == 2
    assert run(cli, *base, "-width", "64", "-list", "L", "-taps", "1", "P").returncode == 2
    assert run(cli, *base, "-width", "64", "-list", "L", "-taps", "4097", "P").returncode == 2
    assert run(cli, *base, "-width", "64", "-list", "L", "-level", "1", "P").returncode == 2
    assert run(cli, "cuts", "-width", "64", "-list", "L", "P").returncode == 1            # no input
    u = run(cli)
    assert b"cuts -width W [-stride =width] -list FILE.emissions [-first-window 0] [-guard 1] [-oversample 2] [-taps 0] [-pad 1] [-print 0] FILENAME_PREFIX \\\n" in u.stderr
    # a cascade in front has no single shift and decimation; -gpus: one source, one device.  Both before any file or device is touched
    r = run(cli, "from", path, "lowpass", "-decimate", "2", "400k", "shift", "1000", "cuts", "-width", "64", "-list", "L", str(tmp_path / "P"))
    assert r.returncode == 1 and b"cascade" in r.stderr, r.stderr
    r = run(cli, "-gpus", "2", "from", path, "cuts", "-width", "64", "-list", "L", str(tmp_path / "P"))
    assert r.returncode == 1 and b"-gpus" in r.stderr and b"one device" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bursts.sr2M.cf32"]
