"""The CLI's `symbols` sink: `emissions` then `symbols -list` on the end-to-end capture of symbols_util (three 2-FSK packets with planted
bits).  The grammar, the dry-run echo and the refusals without a GPU; on the GPU the header, PREFIX.symbols line by line, the bits lines
against the planted bits, and fused (one qd_cuts_symbols) and with QUADRS_HIP_NO_FUSE=1 (qd_cuts_run and a plan, cut by cut) the same
file, for both sinks."""
import os

import numpy as np
import pytest

import symbols_util as U
from test_cli_peaks import cli, run  # noqa: F401  (cli: fixture)

W = U.E2E_W
USAGE = (b" symbols -width W [-stride =width] -list FILE.emissions [cuts' flags] -fft w [-step =w] -by freq|level [-range min] [-window bh|rect] \\\n"
         b"         [-scan SCALE] [-print 0] FILENAME_PREFIX \\\n")


def test_symbols_grammar_and_refusals(cli, tmp_path):
    path = str(tmp_path / "e2e.sr2M.cf32")
    U.e2e_stream()[:4096].tofile(path)
    base = ("-parse-only", "from", path, "symbols")
    need = ("-width", "64", "-list", "L", "-fft", "16", "-by", "freq")
    r = run(cli, *base, *need, "P")
    assert r.returncode == 0 and r.stdout.split(b"\n")[1] == b"symbols width=64 stride=64 list=L first_window=0 guard=1 oversample=2 taps=0 pad=1 fft=16 step=16 by=freq print=0", r.stdout
    r = run(cli, *base, "-width", "64", "-stride", "16", "-list", "L", "-first-window", "7", "-guard", "0", "-oversample", "4", "-taps", "80", "-pad", "9", "-fft", "32",
            "-step", "8", "-by", "level", "-range", "0.5", "-window", "bh", "-scan", "10.5", "-print", "2", "P")
    lines = r.stdout.split(b"\n")
    assert r.returncode == 0 and lines[1] == (b"symbols width=64 stride=16 list=L first_window=7 guard=0 oversample=4 taps=80 pad=9 fft=32 step=8 by=level range=0.5 "
                                              b"scan=10.5 print=2") and lines[2] == b"window=bh", r.stdout
    for missing in ("-width", "-list", "-fft", "-by"):
        words = list(need)
        at = words.index(missing)
        assert run(cli, *base, *(words[:at] + words[at + 2:]), "P").returncode == 2, missing
    assert run(cli, *base, *need).returncode == 2                                        # the prefix
    assert run(cli, *base, *need[:-1], "phase", "P").returncode == 2                     # -by freq|level
    assert run(cli, *base, *need, "-range", "0.5", "P").returncode == 2                  # -range is the mark sink's
    assert run(cli, *base, *need, "-scan", "0", "P").returncode == 2
    assert run(cli, *base, *need, "-window", "hann", "P").returncode == 2
    assert run(cli, *base, *need, "-taps", "1", "P").returncode == 2                     # cuts' flags, cuts' bounds
    assert run(cli, *base, *need, "-oversample", "0", "P").returncode == 2
    assert run(cli, *base, *need, "-level", "1", "P").returncode == 2
    assert run(cli, "symbols", *need, "P").returncode == 1                               # no input
    assert USAGE in run(cli).stderr
    # a cascade in front has no single shift and decimation; -gpus: one source, one device.  Both before any file or device is touched
    r = run(cli, "from", path, "lowpass", "-decimate", "2", "400k", "shift", "1000", "symbols", *need, str(tmp_path / "P"))
    assert r.returncode == 1 and b"cascade" in r.stderr, r.stderr
    r = run(cli, "-gpus", "2", "from", path, "symbols", *need, str(tmp_path / "P"))
    assert r.returncode == 1 and b"-gpus" in r.stderr and b"one device" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["e2e.sr2M.cf32"]


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_emissions_then_symbols(cli, engine, tmp_path):
    x = U.e2e_stream()
    path = str(tmp_path / "e2e.sr2M.cf32")
    x.tofile(path)
    r = run(cli, "from", path, "emissions", "-width", str(W), "-stride", str(W), "-level", str(U.E2E_LEVEL), "-cells", "8", str(tmp_path / "E"))
    assert r.returncode == 0, r.stderr
    listed = str(tmp_path / f"E.sr{U.E2E_SR}.w{W}.emissions")
    records = np.fromfile(listed, dtype=engine.EMISSION_DTYPE)
    assert records.size == len(U.E2E_BINS)
    from test_cuts_cpu import make_desc
    desc = make_desc(engine, U.E2E_SR, x.shape[0], W, W)
    cuts = [engine.cut_of_emission(desc, 0, e, engine.cut_rule(*U.E2E_RULE)) for e in records]
    scale = U.e2e_scale(cuts[0])
    assert all(U.e2e_scale(c) == scale for c in cuts)
    rule = ("-guard", str(U.E2E_RULE[0]), "-oversample", str(U.E2E_RULE[1]), "-pad", str(U.E2E_RULE[2]))
    F = U.E2E_SINK_W
    files = {}
    for by, more in (("freq", ("-scan", repr(scale))), ("level", ("-range", "4", "-step", "8"))):
        for how, env in (("fused", None), ("fine", {"QUADRS_HIP_NO_FUSE": "1"})):
            stem = str(tmp_path / f"S_{by}_{how}")
            r = run(cli, "from", path, "symbols", "-width", str(W), "-list", listed, *rule, "-fft", str(F), "-by", by, *more, "-print", "2", stem, env=env)
            assert r.returncode == 0, (by, how, r.stderr)
            text = open(stem + ".symbols", "rb").read()
            files[by, how] = text
            lines = text.split(b"\n")
            out = r.stdout.split(b"\n")
            step = F if by == "freq" else 8
            windows = [(int(c["count"]) - F) // step if by == "freq" else -(-(int(c["count"]) - F) // step) for c in cuts]
            head = b"symbols width=%d stride=%d first_window=0 guard=%d oversample=%d taps=0 pad=%d fft=%d step=%d by=%s window=rect records=%d windows=%d" % (
                W, W, U.E2E_RULE[0], U.E2E_RULE[1], U.E2E_RULE[2], F, step, by.encode(), len(cuts), sum(windows))
            if by == "freq":
                head += b" scan=%s stuck=0" % (b"%.9g" % scale)
            assert out[0] == head, (out[0], head)
            assert out[1:3] == lines[:2] and out[3] == b"", out[:4]                      # -print 2: the file's first two lines
            per = 2 if by == "freq" else 1
            assert len(lines) == per * len(cuts) + 1 and lines[-1] == b""
            for k, (c, nw) in enumerate(zip(cuts, windows)):
                num, rate, n, digits = lines[per * k].split(b" ")
                assert (num, int(rate), int(n)) == (b"%06d" % k, U.E2E_SR // int(c["decimate"]), nw) and len(digits) == nw and set(digits) <= set(b"01"), lines[per * k][:80]
                if by == "freq":
                    num, bits, err = lines[2 * k + 1].split(b" ")
                    assert num == b"%06d" % k and bits.decode() == "".join(str(b) for b in U.e2e_bits()[k]), (k, bits)
                    assert 0.0 <= float(err) < 4.0
                else:
                    assert 0 < digits.count(b"1") <= nw, (k, digits.count(b"1"), nw)        # the rows of the packet mark
        assert files[by, "fused"] == files[by, "fine"], by
    # an existing output file is refused, with the write sink's message
    r = run(cli, "from", path, "symbols", "-width", str(W), "-list", listed, "-fft", "16", "-by", "freq", str(tmp_path / "S_freq_fused"))
    assert r.returncode == 1 and b"os error 17" in r.stderr, r.stderr
