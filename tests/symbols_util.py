"""Streams, segment lists and references of the symbol list's tests (test_symbols_cpu.py, test_gpu_symbols.py, test_cli_symbols.py).
Everything here is computed by numpy and the oracle alone; each stream and reference is built once, shared and read-only."""
import numpy as np

from util import balanced_real_stream

SR = 2_000_000
N_BUF = 1 << 16
REGION = N_BUF // 4
WIDTHS = (2, 4, 8, 16, 64, 256, 1024, 4096)
BALANCED_WIDTHS = (16, 64, 256)
N_BALANCED = 12
NAN_AT = 2 * REGION + 4_001
BUCKET, MARK = 2, 4                               # QD_EPI_BUCKET2_U8, QD_EPI_MARK_U8
_CACHE = {}


def strides(W):
    return sorted({1, max(W // 2, 1), W, W + 3})


def mark_min(W):
    """the mark sink's range_min of the tests: |X| of a tone of amplitude 0.05 that sits on a bin"""
    return float(np.float32(0.05 * W))


def balanced_at(W):
    """(first, count) of the tie-balanced stream of width W (stride W) inside the buffer: at odd elements at the end of the last region"""
    at = N_BUF - 1
    for w in sorted(BALANCED_WIDTHS, reverse=True):
        at -= 16 * w + 2
        if w == W:
            return at | 1, 16 * w
    raise KeyError(W)


def buffer(oracle):
    """The 2^16-sample cf32 buffer (float32 (n, 2), read-only), four regions of 2^14 samples:
      0  keyed +-tone FSK, amplitude 0.5, tones at +-1/8 cycle a sample, symbols of 48 ... 3000 samples;
      1  on / off keying of a tone at 1/16 cycle a sample in symbols of 256 ... 6000 samples, amplitudes 0, 0.2 and 0.03 / 0.05 / 0.07:
         around mark_min(W) = 0.05 W for every width that has the tone on a bin;
      2  complex noise of sigma 0.3, with ONE NaN real part at NAN_AT;
      3  complex noise of sigma 0.002 (blank rows), and behind it the tie-balanced real streams of BALANCED_WIDTHS (util.balanced_real_stream).
    Noise of sigma 0.002 lies under regions 0 and 1 too."""
    if "buffer" not in _CACHE:
        rng = np.random.default_rng(20261021)
        z = 0.002 * (rng.standard_normal(N_BUF) + 1j * rng.standard_normal(N_BUF))
        t = np.arange(N_BUF)
        at = 0
        while at < REGION:
            n = int(rng.choice([48, 96, 200, 640, 3000]))
            sign = 1 if rng.integers(2) else -1
            z[at:min(at + n, REGION)] += 0.5 * np.exp(sign * 2j * np.pi * t[at:min(at + n, REGION)] / 8)
            at += n
        at, k = REGION, 0
        levels = (0.0, 0.2, 0.03, 0.0, 0.05, 0.07, 0.2, 0.0)
        lengths = (256, 700, 6000, 5000, 256, 1024, 300, 2848)
        while at < 2 * REGION:
            n = lengths[k % 8]
            z[at:min(at + n, 2 * REGION)] += levels[k % 8] * np.exp(2j * np.pi * t[at:min(at + n, 2 * REGION)] / 16)
            at += n
            k += 1
        z[2 * REGION:3 * REGION] += 0.3 * (rng.standard_normal(REGION) + 1j * rng.standard_normal(REGION))
        x = np.stack([z.real, z.imag], axis=1).astype(np.float32)
        for W in BALANCED_WIDTHS:
            first, count = balanced_at(W)
            b, bal = balanced_real_stream(oracle, [], W, W, N_BALANCED, 20261021 + W, SR)
            assert b.shape[0] == count and list(bal) == list(range(N_BALANCED)), (W, b.shape, bal)
            x[first:first + count] = b
        x[NAN_AT, 0] = np.nan
        x.setflags(write=False)
        _CACHE["buffer"] = x
    return _CACHE["buffer"]


def lengths(W, S):
    """the issue's lengths; with S == 1 a length is capped so that a case stays under about 20 000 windows (and the widest under 2000)"""
    ls = [0, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 3 * W + 5, 1000, 4099]
    cap = W + min(1200, max(40, (1 << 19) // W)) if S == 1 else N_BUF
    return [min(v, cap) for v in ls], cap


def segments(W, S):
    """The case's list, a (first, count) uint64 structured array: 40 segments - every length of lengths(W, S) once in each region, at odd
    elements -, one across the NaN sample, and the three tie-balanced streams (balanced at their own width with S == W)."""
    key = ("segments", W, S)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * W + S)
        ls, cap = lengths(W, S)
        rows = []
        for region in range(4):
            for n in ls:
                lo, hi = region * REGION, (region + 1) * REGION
                first = int(rng.integers(lo, max(lo + 1, min(hi, N_BUF - n)))) | 1
                rows.append((min(first, N_BUF - n), n))
        n = min(3 * W + 5, cap)
        rows.append((NAN_AT - 2 * (W // 4), n))                                # (an odd element: window 0 sees the NaN sample whatever the stride)
        for w in BALANCED_WIDTHS:
            first, count = balanced_at(w)
            rows.append((first, min(count, cap)))
        a = np.array(rows, dtype=[("first", "<u8"), ("count", "<u8")])
        assert all(int(f) + int(c) <= N_BUF for f, c in rows)
        a.setflags(write=False)
        _CACHE[key] = a
    return _CACHE[key]


def oracle_bytes(oracle, x, epi, W, S, sr=SR, rmin=None):
    """the reference's bytes of the stream x (float32 (n, 2)): freq_levels digits, or sparkfft's rows as blank / not blank; a stream of at
    most W samples has none (the symbol list's stated departure: the reference underflows there)"""
    if x.shape[0] <= W:
        return np.zeros(0, dtype=np.uint8)
    ch = oracle.Chain.from_bytes(np.ascontiguousarray(x).tobytes(), 0, sr)
    if epi == BUCKET:
        return ch.freq_levels(W, S).copy()
    _, codes = ch.spark_fft(W, S, rng=(mark_min(W) if rmin is None else rmin, 1.0), want_norms=False)
    return (codes != 0).any(axis=1).astype(np.uint8)


def references(oracle, epi, W, S):
    """[bytes of segment k] of the case, from the oracle (read-only)"""
    key = ("refs", epi, W, S)
    if key not in _CACHE:
        x = buffer(oracle)
        out = []
        for f, c in segments(W, S):
            r = oracle_bytes(oracle, x[int(f):int(f) + int(c)], epi, W, S)
            r.setflags(write=False)
            out.append(r)
        _CACHE[key] = out
    return _CACHE[key]


def windows_of(epi, count, W, S):
    """the two counting rules (src/fft.rs:86; src/fft.rs:28,65), and none for a segment of at most W samples"""
    if count <= W:
        return 0
    return (count - W) // S if epi == BUCKET else -(-(count - W) // S)


# ------------------------------------------------------------------ the end-to-end capture

E2E_SR = 2_000_000
E2E_W = 64                                        # the emission plan's width and stride
E2E_LEVEL = 10.0
E2E_SYMBOL = 1024                                 # source samples a bit
E2E_BINS = (42, 18, 36)                           # fftshifted centre bins of the three packets
E2E_GAP = 8192
E2E_SINK_W = 16                                   # the symbol sink's width and stride over a cut
E2E_RULE = (1, 2, 1)                              # guard_bins, oversample, pad


def e2e_bits():
    """the planted bits: 20 a packet, the first a 0 (bits::scan starts on a run of zeros), runs of at most 3"""
    if "e2e_bits" not in _CACHE:
        rng = np.random.default_rng(5)
        out = []
        for _ in E2E_BINS:
            bits, v = [], 0
            while len(bits) < 20:
                bits += [v] * min(int(rng.integers(1, 4)), 20 - len(bits))
                v = 1 - v
            out.append(np.array(bits, dtype=np.uint8))
        _CACHE["e2e_bits"] = out
    return _CACHE["e2e_bits"]


def e2e_stream():
    """A capture at 2 MHz (float32 (n, 2), read-only): silence (complex noise of sigma 0.01) and three 2-FSK packets of amplitude 0.5,
    each on the centre of an emission bin with a deviation of half a bin, so that a 0 lights the bins b - 1 and b and a 1 the bins b and
    b + 1 of every window it fills: one 4-connected emission a packet, symmetric about its centre.  Packets start on a window."""
    if "e2e" not in _CACHE:
        rng = np.random.default_rng(20261022)
        n = len(E2E_BINS) * (E2E_GAP + 20 * E2E_SYMBOL) + E2E_GAP
        z = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        at = E2E_GAP
        for b, bits in zip(E2E_BINS, e2e_bits()):
            fc, dev = (b - E2E_W // 2) / E2E_W, 0.5 / E2E_W
            phase = 0.0
            for bit in bits:
                f = fc + (dev if bit else -dev)
                k = np.arange(E2E_SYMBOL)
                z[at:at + E2E_SYMBOL] += 0.5 * np.exp(2j * np.pi * (phase + f * k))
                phase = (phase + f * E2E_SYMBOL) % 1.0
                at += E2E_SYMBOL
            at += E2E_GAP
        x = np.stack([z.real, z.imag], axis=1).astype(np.float32)
        x.setflags(write=False)
        _CACHE["e2e"] = x
    return _CACHE["e2e"]


def e2e_scale(cut):
    """bucket windows a bit over a cut: the symbol's length at the cut's rate over the sink's stride"""
    return E2E_SYMBOL / int(cut["decimate"]) / E2E_SINK_W
