"""Case tables, streams and references of the cut list's envelope tests (test_cuts_envelope_cpu.py, test_gpu_cuts_envelope.py; DESIGN.md
section 3.27).  Everything here is numpy, the planning header's text and the oracle alone; each table, stream and reference is built once,
shared and read-only.  The tables hold what the strict cuts of test_cuts_cpu.py do not reach: the corners of the tile geometry, every
16-byte load residue, every sample code, signed zeros and non-finite samples, both NCO orders in one list, hundreds of lane and tap
tables, and calls of more than one batch of tiles."""
import os
import re

import numpy as np

from test_cuts_cpu import ROOT, span_of, tile_outputs
from test_gpu_parity import _signal, _to_format
from util import FMT_BYTES, NCO_ABS_ERR, _two_prod_err, ambiguous_components, code_stream, nco_candidates, stream_codes, zero_runs

SR = 21_000_000
N_STREAM = 1 << 17
FLOOR = 60_000                                    # shifted spans lie in [FLOOR, N_STREAM): the +-1 Hz and +-(SR/2 - 1) shifts have ambiguous components below 59 392
CUT_DTYPE = np.dtype([("shift_hz", "<i8"), ("lowpass_hz", "<u8"), ("decimate", "<u8"), ("taps", "<u8"), ("first", "<u8"), ("count", "<u8")])      # engine.CUT_DTYPE
SPV = {0: 2, 1: 8, 2: 8, 3: 4}                    # samples per 16-byte load
_CACHE = {}


def header_constants():
    """every `constexpr uint32_t NAME = EXPR;` of quadrs_amd/csrc/qd_cuts_plan.h whose EXPR is integer arithmetic over earlier names"""
    if "header" not in _CACHE:
        text = open(os.path.join(ROOT, "quadrs_amd", "csrc", "qd_cuts_plan.h")).read()
        k = {}
        for name, expr in re.findall(r"constexpr uint32_t (\w+) = ([^;(]+);", text):
            try:
                k[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(k)))      # noqa: S307 - the project's own header
            except (NameError, SyntaxError):
                pass
        _CACHE["header"] = k
    return _CACHE["header"]


def _frozen(a):
    a.setflags(write=False)
    return a


def make_cuts(rows):
    return _frozen(np.array([tuple(int(v) for v in r) for r in rows], dtype=CUT_DTYPE).reshape(-1))


def first_read(cut):
    D, T = int(cut["decimate"]), int(cut["taps"])
    return int(cut["first"]) * D + T - T // 2


def tiles_of(cut):
    """[(first read, one past the last read)] of every tile of a cut, absolute samples: cut_tile_reads of qd_cuts.h"""
    D, T, first, count = (int(cut[k]) for k in ("decimate", "taps", "first", "count"))
    to, ctr, valid, out = tile_outputs(D, T), T - T // 2, count * D + T, []
    for o in range(0, count, to):
        n = min(to, count - o)
        out.append((first * D + o * D + ctr, first * D + min(valid, (o + n - 1) * D + ctr + T)))
    return out


def ragged_samples(cut, fmt):
    """the absolute samples of a cut that k_cuts loads one by one, in front of the first and behind the last whole 16-byte group of each
    tile, when sample 0 of the stream lies on a 16-byte boundary"""
    spv, out = SPV[fmt], []
    for lo, hi in tiles_of(cut):
        head = min((-lo) % spv, hi - lo)
        tail = lo + head + (hi - lo - head) // spv * spv
        out += list(range(lo, lo + head)) + list(range(tail, hi))
    return out


# ------------------------------------------------------------------ the envelope table

ENV_SHAPES = ((1, 4096), (20, 4096), (1024, 2), (1023, 4096), (255, 4096), (36, 36), (35, 256), (33, 64), (64, 512), (3, 2), (2, 4094))
ENV_SHIFTS = (0, 999_983, -3_000_017, 1, -1, 10_499_999, -10_499_999)
ROW_SHAPE = (20, 4096)                            # the longest tile span of all admissible shapes (test_cuts_envelope_cpu.py holds that)
ALIGN_SHIFT = 999_983
ENV_AT, ENV_STEP = 6, 1021                         # the placements: ones at which every broken rule of the twin shows in every case marked for it


def env_counts(D, T):
    tile = tile_outputs(D, T)
    return (1, tile - 1, tile, tile + 1, 2 * tile + 3)


def row_edge_first():
    """`first` of the planted ROW_SHAPE cut: the first cut behind FLOOR whose first read has the largest residue modulo the NCO row that the
    shape reaches at all (first D + T - T/2 is a multiple of 4 there, so 508 of 512 and not 511)"""
    D, T = ROW_SHAPE
    row = header_constants()["kCutsNcoRow"]
    f0 = -(-FLOOR // D)
    res = [(f * D + T - T // 2) % row for f in range(f0, f0 + row)]
    return f0 + int(np.argmax(res))


def envelope_cuts():
    """Every shape of ENV_SHAPES with its five counts; the shape's shifts are 0 (at count index si % 5) and four of the six others, rotated;
    spans start behind FLOOR at odd offsets and overlap their neighbours'.  Last: the shifted ROW_SHAPE cut of row_edge_first(), whose first
    tile is the longest tile there is and starts at the end of an NCO row."""
    if "env" not in _CACHE:
        rows, i = [], 0
        for si, (D, T) in enumerate(ENV_SHAPES):
            shifts = [ENV_SHIFTS[1 + (si + k) % 6] for k in range(4)]
            shifts.insert(si % 5, 0)
            for count, s in zip(env_counts(D, T), shifts):
                first = -(-(FLOOR + 1 + (ENV_AT + ENV_STEP * i) % 45_000) // D)
                rows.append((s, 150_000 + 20_011 * (i % 5), D, T, first, count))
                i += 1
        rows.append((999_983, 190_022, ROW_SHAPE[0], ROW_SHAPE[1], row_edge_first(), 2 * tile_outputs(*ROW_SHAPE) + 3))      # (a shorter cut's block ends inside its first tile's reach)
        _CACHE["env"] = make_cuts(rows)
        assert all(span_of(c)[1] + int(c["taps"]) <= N_STREAM for c in _CACHE["env"])
    return _CACHE["env"]


def align_cuts():
    """The alignment table, one list for all formats (residues modulo 8 samples hold those modulo 4 and 2).  Shift-free and with ALIGN_SHIFT:
      * (1, 2): every residue of the first read crossed with every residue of the span's end, 64 cuts of 24 ... 31 outputs;
      * (4, 40): the pairs that shape reaches (its first read and its end are multiples of 4);
      * (1, 2), one output: a tile of 2 samples at every residue - behind a ragged head of up to 7 in the 8-bit formats;
      * the cuts that end on the stream's last sample, (1, 2) and (4, 40);
    and shift-free only: the cuts with first == 0."""
    if "align" not in _CACHE:
        rows = []
        for s in (0, ALIGN_SHIFT):
            at = FLOOR + 1000
            for h in range(8):
                for e in range(8):
                    first = at + (h - 1 - at) % 8                              # first + 1 = h (mod 8)
                    count = 24 + (e - (first + 24 + 2)) % 8                    # first + count + 2 = e (mod 8)
                    rows.append((s, 2_000_000, 1, 2, first, count))
                    at += 173
            for h in (0, 1):
                for e in (0, 1):
                    first = 18_001 + 2 * len(rows) + (h - 18_001 - 5) % 2      # 4 first + 20 = 4 h (mod 8)
                    count = 300 + (e - (first + 300 + 10)) % 2                 # 4 (first + count) + 40 = 4 e (mod 8)
                    rows.append((s, 900_000, 4, 40, first, count))
            rows += [(s, 2_000_000, 1, 2, FLOOR + 40_000 + 11 * h, 1) for h in range(8)]
            rows += [(s, 2_000_000, 1, 2, N_STREAM - 2 - 37, 37), (s, 900_000, 4, 40, (N_STREAM - 40) // 4 - 261, 261)]
        rows += [(0, 2_000_000, 1, 2, 0, 37), (0, 900_000, 4, 40, 0, 9)]
        _CACHE["align"] = make_cuts(rows)
    return _CACHE["align"]


def signal_stream(fmt):
    """the 2^17-sample stream of a format: test_gpu_parity's signal in that format's codes (read-only uint8)"""
    key = ("signal", fmt)
    if key not in _CACHE:
        _CACHE[key] = _frozen(np.frombuffer(_to_format(_signal(np.random.default_rng(20261021), N_STREAM), fmt), dtype=np.uint8).copy())
    return _CACHE[key]


def oracle_cut(oracle, data, fmt, sr, cut, first=None, mults=None):
    """the reference's read_at(first, count) of  from -> [shift] -> lowpass  over `data`; mults = (c, s): f32 multipliers of every sample of
    `data`, planted through override_shift"""
    ch = oracle.Chain.from_bytes(data, fmt, sr)
    if int(cut["shift_hz"]):
        ch = ch.shift(int(cut["shift_hz"]))
        if mults is not None:
            ch.override_shift(0, np.arange(len(mults[0]), dtype=np.uint64), mults[0], mults[1])
    ch = ch.lowpass(int(cut["lowpass_hz"]), int(cut["decimate"]), int(cut["taps"]))
    got, y = ch.read_at(int(cut["first"]) if first is None else first, int(cut["count"]))
    assert got == int(cut["count"]), (got, cut)
    return _frozen(y)


def oracle_refs(oracle, key, data, fmt, cuts, sr=SR):
    """[the reference's bytes of cut k], cached under key"""
    key = ("refs", key, fmt)
    if key not in _CACHE:
        data = np.ascontiguousarray(data)
        last, chain = None, None
        out = []
        for c in cuts:                                                          # neighbours with one (shift, lowpass, D, T) share a chain: the stream is copied once
            k = (int(c["shift_hz"]), int(c["lowpass_hz"]), int(c["decimate"]), int(c["taps"]))
            if k != last:
                chain = oracle.Chain.from_bytes(data, fmt, sr)
                if k[0]:
                    chain = chain.shift(k[0])
                last, chain = k, chain.lowpass(k[1], k[2], k[3])
            got, y = chain.read_at(int(c["first"]), int(c["count"]))
            assert got == int(c["count"]), (got, c)
            out.append(_frozen(y))
        _CACHE[key] = out
    return _CACHE[key]


def clean(oracle, cut, sr=SR):
    """no ambiguous NCO multiplier component in the cut's span (shift-free cuts have no multiplier at all)"""
    if not int(cut["shift_hz"]):
        return True
    a, b = span_of(cut)
    return ambiguous_components(oracle.shift_ratio(int(cut["shift_hz"]), sr), a, b) == []


# ------------------------------------------------------------------ the twin with switchable rules

def twin_cut(oracle, x, cut, sr=SR, truncate=True, ascending=True, fused=False):
    """The header's definition in numpy over x, the (shifted) cf32 stream (n, 2): out[i] = sum_{j < jmax(i)} x[first D + i D + c + j] taps[j]
    in f32, ascending j, separately rounded products.  Each switch breaks one rule: no tail truncation (the filter runs on past the cut's
    block), descending tap order, a fused multiply-add (product and sum in f64, rounded once)."""
    D, T, first, count = (int(cut[k]) for k in ("decimate", "taps", "first", "count"))
    h = oracle.taps(int(cut["lowpass_hz"]), sr, T)
    c, valid = T - T // 2, count * D + T
    base = first * D + np.arange(count, dtype=np.int64) * D + c
    jmax = np.minimum(T, valid - (np.arange(count, dtype=np.int64) * D + c)) if truncate else np.full(count, T)
    acc = np.zeros((count, 2), dtype=np.float32)
    for j in (range(T) if ascending else range(T - 1, -1, -1)):
        live = j < jmax
        if not live.any():
            continue
        v = x[np.minimum(base + j, x.shape[0] - 1)]
        if fused:
            new = (acc.astype(np.float64) + v.astype(np.float64) * np.float64(h[j])).astype(np.float32)
        else:
            new = acc + v * h[j]
        acc = np.where(live[:, None], new, acc)
    return acc


def shifted_stream(oracle, shift):
    """the cf32 signal stream behind the reference's Shift (or as it is), (N_STREAM, 2) float32"""
    key = ("shifted", shift)
    if key not in _CACHE:
        ch = oracle.Chain.from_bytes(signal_stream(0), 0, SR)
        if shift:
            ch = ch.shift(shift)
        got, y = ch.read_at(0, N_STREAM)
        assert got == N_STREAM
        _CACHE[key] = _frozen(y)
    return _CACHE[key]


# ------------------------------------------------------------------ value streams

VALUE_N = {1: 1 << 14, 2: 1 << 14, 3: 300_000}
VALUE_SHIFT = 999_983
VALUE_T = 4
EDGE_CODES = {1: (0x00, 0x7F, 0x80, 0xFF), 2: (0x00, 0x7F, 0x80, 0xFF), 3: (0x0000, 0x7FFF, 0x8000, 0xFFFF)}


def value_stream(fmt):
    """util.code_stream of the format behind one 16-byte group (a copy of the stream's last), so that every sample of the code stream keeps
    its load position and can be read by a cut: sample 0 of a stream never is (the first read of a cut is first D + T - T/2 >= 1)"""
    key = ("codes", fmt)
    if key not in _CACHE:
        s = code_stream(fmt, VALUE_N[fmt], 7 + fmt)
        _CACHE[key] = _frozen(np.concatenate([s[-16:], s]))
    return _CACHE[key]


def value_cuts(fmt):
    """(1, VALUE_T) cuts over value_stream(fmt), shift-free and with VALUE_SHIFT: one per load position, cut k with its first read at position
    k, each handing over to the next, together every sample of the code stream; and for every edge code and component a one-output (1, 2)
    cut, all per-sample loads, that reads a sample with it"""
    key = ("value_cuts", fmt)
    if key not in _CACHE:
        spv, n = SPV[fmt], VALUE_N[fmt] + 16 // FMT_BYTES[fmt]
        codes = stream_codes(fmt, value_stream(fmt))
        rows = []
        for s in (0, VALUE_SHIFT):
            piece = n // spv
            for k in range(spv):
                first = k * piece + (k - k * piece - VALUE_T // 2) % spv       # first + T - T/2 = k (mod spv); cut 0 reads from the code stream's first sample on
                end = n - VALUE_T if k == spv - 1 else (k + 1) * piece + spv
                rows.append((s, 2_000_000, 1, VALUE_T, first, end - first))
            for code in EDGE_CODES[fmt]:
                for comp in range(2):
                    at = np.flatnonzero(codes[spv + 8:n - 8, comp] == code)
                    rows.append((s, 2_000_000, 1, 2, int(at[len(at) // 2]) + spv + 8 - 1, 1))
        _CACHE[key] = make_cuts(rows)
    return _CACHE[key]


ZERO_LONG, ZERO_SPAN = 2400, 600
NAN_AT, INF_AT = 70_001, 100_003
_SPECIAL_SHAPE = (900_000, 4, 40)


def zero_stream():
    """util.zero_runs over the cf32 signal: (read-only bytes, mask of the samples with a zero component)"""
    if "zeros" not in _CACHE:
        x, mask = zero_runs(_signal(np.random.default_rng(20261021), N_STREAM), ZERO_LONG, ZERO_SPAN, 11)
        _CACHE["zeros"] = (_frozen(x.view(np.uint8).reshape(-1)), _frozen(mask))
    return _CACHE["zeros"]


def zero_cuts():
    """(4, 40) and (1, 8) cuts, shift-free and shifted, over the long run of signed zeros (all four quarters) and over short runs behind FLOOR"""
    a = N_STREAM // 3
    rows = []
    for s in (0, VALUE_SHIFT, -3_000_017):
        rows += [(s, 900_000, 4, 40, (a - 300) // 4, (ZERO_LONG + 600) // 4), (s, 2_000_000, 1, 8, a - 51, ZERO_LONG + 102),
                 (s, 900_000, 4, 40, (FLOOR + 3) // 4, 4000), (s, 2_000_000, 1, 8, FLOOR + 20_001, 5000)]
    return make_cuts(rows)


def special_stream(planted=True):
    """the cf32 signal with ONE NaN real part at NAN_AT and ONE +Inf imaginary part at INF_AT (planted=False: the clean signal), read-only bytes"""
    key = ("special", planted)
    if key not in _CACHE:
        x = _signal(np.random.default_rng(20261021), N_STREAM)
        if planted:
            x[NAN_AT, 0] = np.nan
            x[INF_AT, 1] = np.inf
        _CACHE[key] = _frozen(x.view(np.uint8).reshape(-1))
    return _CACHE[key]


def special_cuts():
    """(4, 40) and (1, 2) cuts around each planted sample, shift-free and shifted: each starts well ahead of it and ends well behind"""
    rows = []
    for s in (0, VALUE_SHIFT):
        for at in (NAN_AT, INF_AT):
            rows += [(s,) + _SPECIAL_SHAPE + (at // 4 - 150, 300), (s, 2_000_000, 1, 2, at - 40, 80)]
    return make_cuts(rows)


def reaches(cut, at):
    """mask of the outputs of a cut whose T-sample reach [first D + i D + c, + T) holds sample `at`"""
    D, T, first, count = (int(cut[k]) for k in ("decimate", "taps", "first", "count"))
    lo = first * D + np.arange(count) * D + T - T // 2
    return (lo <= at) & (at < lo + T)


# ------------------------------------------------------------------ both NCO orders in one list

SENSITIVE_CASES = (                               # (sensitive shift, rate, sample, companion first-order shift): tests/test_gpu_parity.py SENSITIVE
    (-1_234_567, 21_000_000, 11_625_090_444, 1000),
    (49_999_999, 100_000_000, 1_346_889_343, 1000),
    (49_999_999, 100_000_000, 1_347_894_995, 1000),
    (-7_777_777, 21_000_000, 1_842_962_899, 1000),
)
SENS_HALF = 400                                   # the slab is samples [base, base + 2 SENS_HALF) around the sensitive sample
SENS_D, SENS_T, SENS_COUNT = 2, 40, 300
SECOND_ORDER_ABOVE = 268435456.0                  # include/quadrs_hip.h: the second-order form iff fabs(ratio) (first D + valid) exceeds it


def sensitive_case(k):
    """(sr, n_samples, base, slab bytes (cf32: a unit impulse at the sensitive sample over noise of sigma 0.001), cuts [shift-free, companion
    shift, sensitive shift] over the slab, absolute `first`)"""
    key = ("sens", k)
    if key not in _CACHE:
        shift, sr, n, companion = SENSITIVE_CASES[k]
        base = (n - SENS_HALF) // SENS_D * SENS_D
        m = 2 * SENS_HALF
        x = (np.random.default_rng(20261021 + k).standard_normal((m, 2)) * 0.001).astype(np.float32)
        x[n - base] = (1.0, 0.0)
        first = (base + 60) // SENS_D
        cuts = make_cuts([(s, 2_000_000, SENS_D, SENS_T, first, SENS_COUNT) for s in (0, companion, shift)])
        a, b = span_of(cuts[2])
        assert base <= a and a + SENS_T < n < b - SENS_T and b <= base + m
        _CACHE[key] = (sr, n + (1 << 20), base, _frozen(x.view(np.uint8).reshape(-1)), cuts)
    return _CACHE[key]


def sensitive_mults(oracle, k, shift, first_order_at=None):
    """the reference's f32 multipliers (c, s) of the slab's absolute indices for `shift`; first_order_at = n: the sensitive component of
    sample n replaced by the neighbouring f32 that an NCO without the second-order term lands on (util.nco_sensitive_samples' condition)"""
    sr, _, base, slab, _ = sensitive_case(k)
    ratio = oracle.shift_ratio(shift, sr)
    c64, s64 = oracle.shift_multipliers_f64(ratio, base, slab.size // 8)
    c, s = c64.astype(np.float32), s64.astype(np.float32)
    moved = 0
    if first_order_at is not None:
        i = first_order_at - base
        r = float(_two_prod_err(np.float64(first_order_at), np.float64(ratio)))
        for arr, v in ((c, c64[i]), (s, s64[i])):
            lo, hi = nco_candidates(np.array([v]))
            f = np.float32(v)
            nb = np.nextafter(f, np.float32(-np.inf) if v < 0 else np.float32(np.inf))
            dist = abs((float(f) + float(nb)) / 2) - abs(v)
            if lo[0] == hi[0] and 2 * NCO_ABS_ERR < dist < abs(v) * 0.5 * r * r - 2 * NCO_ABS_ERR:
                arr[i] = nb
                moved += 1
    return c, s, moved


def sensitive_refs(oracle, k):
    """the reference's bytes of the case's three cuts, the shifted ones with the multipliers of the absolute indices planted"""
    key = ("sens_refs", k)
    if key not in _CACHE:
        sr, _, base, slab, cuts = sensitive_case(k)
        out = []
        for c in cuts:
            mults = sensitive_mults(oracle, k, int(c["shift_hz"]))[:2] if int(c["shift_hz"]) else None
            out.append(oracle_cut(oracle, slab, 0, sr, c, first=int(c["first"]) - base // SENS_D, mults=mults))
        _CACHE[key] = out
    return _CACHE[key]


# ------------------------------------------------------------------ many tables, many tiles

MANY_N = 600


def many_cuts():
    """600 short cuts behind FLOOR, shuffled: 300 distinct shifts and their negatives - among them +-1 Hz and +-(SR/2 - 1) -, 150 distinct
    (lowpass_hz, taps) pairs with T = 2 ... 4096, D = 1 ... 64, 1 ... 9 outputs"""
    if "many" not in _CACHE:
        rng = np.random.default_rng(20261021)
        fixed = np.array([1, SR // 2 - 1, 999_983, 3_000_017])
        shifts = np.concatenate([fixed, rng.permutation(np.setdiff1d(rng.integers(2, SR // 2 - 1, 400), fixed))[:300 - fixed.size]])
        shifts = np.concatenate([shifts, -shifts])
        fixed = np.array([2, 4, 40, 4094, 4096])
        ts = np.concatenate([fixed, rng.permutation(np.setdiff1d(2 * rng.integers(1, 2049, 300), fixed))[:150 - fixed.size]])
        pairs = [(100_000 + 13_001 * i, int(t)) for i, t in enumerate(ts)]
        assert len(set(shifts.tolist())) == MANY_N and len({t for _, t in pairs}) == 150
        rows = []
        for i in rng.permutation(MANY_N):
            lp, T = pairs[i % 150]
            D = int(rng.choice([1, 2, 3, 4, 7, 16, 33, 64]))
            count = int(rng.integers(1, 10))
            first = -(-(FLOOR + 1 + int(rng.integers(0, N_STREAM - FLOOR - (count + 1) * D - T - 2))) // D)
            rows.append((int(shifts[i]), lp, D, T, first, count))
        _CACHE["many"] = make_cuts(rows)
    return _CACHE["many"]


def many_clean(oracle):
    """mask of many_cuts(): the spans without an ambiguous multiplier component"""
    if "many_clean" not in _CACHE:
        _CACHE["many_clean"] = _frozen(np.array([clean(oracle, c) for c in many_cuts()]))
    return _CACHE["many_clean"]


CAP_SHAPE = (999_983, 300_000, 4, 40)
CAP_ONES = 17_000


def cap_ones():
    """17 000 shifted cuts of one output, a tile each: more than kCutsBatchTiles tiles in one call"""
    if "ones" not in _CACHE:
        a = np.zeros(CAP_ONES, dtype=CUT_DTYPE)
        a["shift_hz"], a["lowpass_hz"], a["decimate"], a["taps"], a["count"] = CAP_SHAPE + (1,)
        a["first"] = FLOOR // 4 + 1 + np.arange(CAP_ONES)
        _CACHE["ones"] = _frozen(a)
    return _CACHE["ones"]


def cap_long():
    """(cu8 stream of random bytes, the shift-free (1, 2) cut of kCutsBatchTiles tiles and 300 outputs more over it)"""
    if "long" not in _CACHE:
        count = header_constants()["kCutsBatchTiles"] * tile_outputs(1, 2) + 300
        n = 5 + count + 2 + 9
        data = np.random.default_rng(20261021).integers(0, 256, 2 * n, dtype=np.uint8)
        _CACHE["long"] = (_frozen(data), make_cuts([(0, 2_000_000, 1, 2, 5, count)]))
    return _CACHE["long"]
