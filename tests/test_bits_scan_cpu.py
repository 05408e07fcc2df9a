"""qd_bits_scan against a Python restatement of bits::scan / run_of (src/bits.rs:3-55).  Host arithmetic only: no GPU."""
import ctypes as C
import math

import numpy as np
import pytest


def rust_round(x):
    """f64::round: to the nearest integer, halves away from zero (exact: floor(|x|) and the fraction are exact in f64)."""
    f = math.floor(abs(x))
    r = f + 1.0 if abs(x) - f >= 0.5 else f
    return math.copysign(r, x)


def run_of(data, scale, val):
    """src/bits.rs:40-55"""
    bad = 0
    for i, bit in enumerate(data):
        bad = bad + 1 if bit != val else 0
        if bad > scale:
            return i + 1 - bad
    return len(data)


def scan(data, scale):
    """src/bits.rs:3-38 -> (status, error, bits).  status "stuck": the reference's loop would never end — a run of at most `half`
    before the end of the data `continue`s without flipping `bit`, the next run_of returns 0, and so on (the no-progress guard
    below); error and bits are what had been emitted by then."""
    data = [bool(v) for v in data]
    i, half, bit, error, ret = 0, int(rust_round(scale / 2.0)), False, 0.0, []
    while i != len(data):
        found = run_of(data[i:], half, bit)
        i += found
        if found <= half:
            if i != len(data):
                # no progress is possible from here: the same `bit`, and data[i:] opens with more than `half` wrong values
                assert run_of(data[i:], half, bit) == 0
                return "stuck", error, ret
            continue
        bits = found / scale
        rounded = rust_round(bits)
        error += abs(bits - rounded)
        ret.extend([bit] * int(rounded))
        bit = not bit
    return "ok", error, ret


def parse(s):
    return [c == "1" for c in s if not c.isspace()]


def test_reference_run_of_vectors():
    """the reference's own unit test, src/bits.rs:60-69.  Pins the Python restatement, not the library: it passes without qd_bits_scan."""
    assert run_of(parse("0000"), 2, False) == 4                 # runs a whole buffer
    assert run_of(parse("00001000111"), 2, False) == 8          # doesn't trip over a single bit flip at 2


def test_rust_round_halves_away_from_zero():
    """pins the restatement's rounding, not the library"""
    assert [rust_round(v) for v in (0.5, 1.5, 2.5, 0.49999999999999994, 8.15, 1.25)] == [1.0, 2.0, 3.0, 0.0, 8.0, 1.0]


def _call(engine, marks, scale, cap):
    L = engine._ffi.lib()
    m = np.ascontiguousarray(marks, dtype=np.uint8)
    bits = np.full(max(cap, 0) + 8, 0xA5, dtype=np.uint8)       # guard bytes behind cap
    produced, error = C.c_size_t(12345), C.c_double(-1.0)
    rc = L.qd_bits_scan(m.ctypes.data_as(C.c_void_p), m.size, float(scale), bits.ctypes.data_as(C.c_void_p), cap,
                        C.byref(produced), C.byref(error))
    assert (bits[cap:] == 0xA5).all()
    return rc, produced.value, error.value, bits[:cap]


def test_reference_vectors_through_the_library(engine):
    """the run_of vectors seen through scan: at scale 4 (half 2) the first stream is one run of four 0s -> one 0 bit, error 0;
    the second is a run of eight (the lone 1 does not stop it) -> two 0 bits, then three 1s -> round(0.75) = one 1 bit."""
    for s, scale in (("0000", 4.0), ("00001000111", 4.0), ("", 4.0), ("1111", 4.0)):
        st, err, bits = scan(parse(s), scale)
        rc, produced, error, out = _call(engine, parse(s), scale, 64)
        assert rc == (engine._ffi.OK if st == "ok" else engine._ffi.ERR_PANIC), s
        assert produced == len(bits) and list(out[:produced]) == [int(b) for b in bits] and error == err
    assert scan(parse("0000"), 4.0) == ("ok", 0.0, [False])
    assert scan(parse("00001000111"), 4.0) == ("ok", 0.25, [False, False, True])
    assert scan(parse("1111"), 4.0)[0] == "stuck"            # opens with more than `half` 1s while 0 is expected: run_of returns 0


def _streams():
    """~2000 seeded mark streams: keyed runs around a multiple of the scale with jitter and isolated flips (mostly decodable), and
    plain random bits (mostly the non-terminating case)"""
    rng = np.random.default_rng(20260)
    for case in range(2000):
        scale = (1.0, 2.5, 8.0, 16.3)[case % 4]
        kind = (case // 4) % 3
        if kind == 0:
            n = int(rng.integers(0, 40))
            marks = rng.integers(0, 2, n).astype(np.uint8)
        else:
            parts, val = [], 0 if kind == 1 else int(rng.integers(0, 2))
            for _ in range(int(rng.integers(1, 9))):
                ln = max(1, int(round(scale * int(rng.integers(1, 4)) + rng.normal(0, scale * 0.15))))
                run = np.full(ln, val, dtype=np.uint8)
                if ln > 2 and rng.random() < 0.3:
                    run[int(rng.integers(1, ln - 1))] ^= 1      # an isolated flip inside the run
                parts.append(run)
                val ^= 1
            marks = np.concatenate(parts)
            if rng.random() < 0.5:
                marks = marks * int(rng.integers(1, 256))       # any non-zero byte is a mark
        yield case, scale, marks.astype(np.uint8)


def test_random_streams_match_the_restatement(engine):
    F = engine._ffi
    seen = {"ok": 0, "stuck": 0}
    for case, scale, marks in _streams():
        st, err, bits = scan(marks, scale)
        seen[st] += 1
        want = [int(b) for b in bits]
        rc, produced, error, out = _call(engine, marks, scale, len(bits))
        assert rc == (F.OK if st == "ok" else F.ERR_PANIC), (case, scale, marks.tolist())
        assert produced == len(bits) and list(out) == want, (case, scale, marks.tolist())
        assert np.float64(error).tobytes() == np.float64(err).tobytes(), (case, error, err)      # bit for bit
        if st == "stuck":
            assert b"src/bits.rs:9-15" in F.lib().qd_last_error()
        if bits:                                                # a cap one too small: QD_ERR_INVALID and the count needed
            rc, produced, error, out = _call(engine, marks, scale, len(bits) - 1)
            assert rc == F.ERR_INVALID and produced == len(bits) and list(out) == want[:-1]
    assert seen["ok"] > 300 and seen["stuck"] > 300, seen       # both outcomes are exercised


def test_empty_stream_and_bad_scale(engine):
    F = engine._ffi
    for scale in (1.0, 2.5, 8.0, 16.3):
        assert _call(engine, [], scale, 0)[:3] == (F.OK, 0, 0.0)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(engine, [0, 0, 1, 1], scale, 8)[0] == F.ERR_INVALID


def test_python_view(engine):
    err, bits = engine.bits_scan(parse("00001000111"), 4.0)
    assert err == 0.25 and bits.tolist() == [0, 0, 1]
    with pytest.raises(engine.QuadrsError) as e:
        engine.bits_scan(parse("1111"), 4.0)
    assert e.value.code == engine._ffi.ERR_PANIC
