import numpy as np

import os

# the reference's README.md:167, copied verbatim as an expected-output fixture
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readme_ook_line167.txt")) as _f:
    README_OOK = _f.read().strip()


def ook_pipeline(text):
    """The README's sed/tr pipeline (README.md:122-167) over spark_fft's stdout bytes."""
    import re
    bits = []
    for line in text.decode("utf-8").split("\n")[:-1]:
        line = re.sub(r"^.    .$", ".", line)
        line = re.sub(r"....*", "X", line)
        bits.append(line)
    s = "".join(bits).replace(".", "o")     # the README writes '.' in one step and 'o' in the next
    return re.sub(r"o{5,10}", "B", re.sub(r"X{6,10}", "A", s))


def ulp_diff(a, b):
    """distance in units of f32 representable steps (sign-magnitude ordered)"""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def ulp_of(x):
    """spacing of f32 at |x|"""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.spacing(np.maximum(x, np.float32(1e-45)))


def complex_ulp_err(ref, got):
    """|got - ref| per component in units of ulp(max(|re|,|im|)) of the reference sample —
    the cf32 tolerance unit used throughout (north_star: 'within 1 ulp on cf32')."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 2)
    got = np.asarray(got, dtype=np.float32).reshape(-1, 2)
    scale = ulp_of(np.max(np.abs(ref), axis=1)).astype(np.float64)
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=1)
    return d / scale


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def fuzz_chain_shapes(Q, n_shapes, seed, log=None, oracle=None, variants_only=False, auto_only=False, stats=None):
    """Random chain shapes through the plan-time compiler (QD_JIT=1; a quarter of them with a QD_TUNE tiling that
    exercises the register-tiled FIR / 16-byte LDS rows / wide workgroups) against the generic kernel (QD_JIT=0),
    bit for bit; with `oracle` (tests only) the first windows are also checked against the CPU oracle: bit-exact without
    a shift stage, within 1 ulp of the window maximum with one.  Returns (checked, mismatching descriptions).
    Q is the quadrs_amd package."""
    import os
    rng = np.random.default_rng(seed)
    checked, bad = 0, []
    saved = {k: os.environ.get(k) for k in ("QD_TUNE", "QD_JIT")}
    try:
        for _ in range(n_shapes):
            fmt = int(rng.integers(0, 4))
            W = 1 << int(rng.integers(2, 11))
            S = int(rng.choice([W, W, max(1, W // 2), max(1, W // 4), int(rng.integers(1, 2 * W + 1))]))
            D = int(rng.choice([1, 2, 3, 4, 7, 8, 12, 16, 32, 64]))
            T = int(rng.choice([2, 8, 9, 16, 40, 48, 64, 100, 128, 200, 256, 400, 512, 800]))
            if auto_only:                           # the families the plan-time variant selection serves, NO hint: the library chooses
                W = int(rng.choice([64, 128, 256, 512, 1024]))
                S = W
                D = int(rng.choice([4, 8, 16, 32]))
                T = int(rng.choice([64, 72, 96, 128, 160, 192, 200, 256, 384, 400, 512]))
                fmt = int(rng.choice([0, 0, 1, 3]))
                if rng.random() < 0.3:                 # overlapping windows with a long filter: the three-stage kernel's family
                    W = int(rng.choice([64, 128]))
                    S = int(rng.choice([16, W // 4, W // 2]))
                    D = int(rng.choice([8, 16, 32]))
                    T = int(rng.choice([t for t in (128, 200, 256, 400, 512) if t >= 8 * D]))
            if variants_only:                       # geometries the FLAGS_ variants apply to, every shape with a variant tiling
                D = int(rng.choice([8, 16, 32, 64]))
                T = int(rng.choice([32, 40, 48, 64, 96, 128, 200, 256, 400, 512, 800]))
                if rng.random() < 0.5:
                    S = W
            if (W * D + T) * 8 * 1.2 > 150 * 1024:
                continue
            shift = None if rng.random() < 0.25 else int(rng.integers(-3_000_000, 3_000_000))
            N = (int(rng.integers(3, 400)) * S + W) * D + T + int(rng.integers(0, D + 1))
            bps = {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
            data = rng.integers(0, 256, N * bps, dtype=np.uint8)
            if fmt == 0:
                data = (rng.standard_normal((N, 2)).astype(np.float32) * 0.05).view(np.uint8).reshape(-1)
            tune = None
            if auto_only:
                pass
            elif not variants_only and rng.random() < 0.25 and D % 8 == 0 and T % 16 == 0:
                tune = "%d:%d:%d:8:%d:%d" % (rng.integers(1, 4), rng.choice([256, 512, 1024]), rng.choice([1, 2]), rng.choice([2, 4]),
                                            rng.choice([1, 2]))
            elif (variants_only or rng.random() < 0.35) and D % 8 == 0 and T % 8 == 0 and T >= 32:
                # the FLAGS_ variants of the built-in kernels on shapes of the fuzzer's choosing: packed pair FIR (4), row-aligned
                # phase 1 (8), deferred FFT (64, two slots), straight-line shared FIR (32), packed two-output tile (128)
                flags, batch = [(4, 1), (12, 1), (68, 2), (76, 2), (32, 1), (128, 1), (192, 2), (4, 2)][int(rng.integers(0, 8))]
                tune = "%d:%d:%d:4:4:2:%d:0" % (rng.integers(1, 3), rng.choice([256, 512, 1024]), 2 if flags & 128 else 1, batch | (flags << 8))
            epi = int(rng.choice([0, 0, 1, 2]))             # f32 norms / glyph codes / bucket digits
            outs, info = {}, {}
            for mode in ("0", "1"):
                os.environ.pop("QD_TUNE", None)
                os.environ["QD_JIT"] = mode
                if mode == "1" and tune:
                    os.environ["QD_TUNE"] = tune
                try:
                    try:
                        p = Q.Plan(fmt, 21_000_000, N, shift_hz=shift, lowpass=(1_000_000, D, T), width=W, stride=S, epilogue=epi)
                    except Q.QuadrsError as e:
                        if "tile_hint" not in str(e) or "QD_TUNE" not in os.environ:
                            raise
                        os.environ.pop("QD_TUNE")            # a tiling this shape cannot take (LDS, geometry): the library's own choice
                        tune = None
                        p = Q.Plan(fmt, 21_000_000, N, shift_hz=shift, lowpass=(1_000_000, D, T), width=W, stride=S, epilogue=epi)
                    outs[mode] = p.run_host(data)
                    info[mode] = (p.info.kernel_kind, p.info.tile_windows, p.info.threads, p.info.kernel_flags)
                    if stats is not None and mode == "1":
                        stats.append((int(p.info.kernel_kind), int(p.info.kernel_flags)))
                except Q.QuadrsError as e:
                    outs[mode] = str(e)
            a, b = outs["0"], outs["1"]
            ok = (isinstance(a, str) and isinstance(b, str)) or (
                not isinstance(a, str) and not isinstance(b, str) and a.shape == b.shape and a.tobytes() == b.tobytes())
            if ok and epi == 0 and oracle is not None and not isinstance(a, str) and a.shape[0] > 0:
                ch = oracle.Chain.from_bytes(data.tobytes(), fmt, 21_000_000)
                if shift is not None:
                    ch = ch.shift(shift)
                ref, _ = ch.lowpass(1_000_000, D, T).spark_fft(W, S, max_windows=24)
                got = a[:ref.shape[0]]
                if shift is None:
                    ok = bits_equal(ref, got)
                else:
                    # odd tap counts put a 0/0 in the middle of the reference's windowed sinc: NaN spectra, on both sides
                    both_nan = np.isnan(ref) & np.isnan(got)
                    with np.errstate(invalid="ignore"):
                        scale = ulp_of(np.nanmax(np.where(np.isnan(ref), -np.inf, ref), axis=-1, keepdims=True)).astype(np.float64)
                        close = np.abs(ref.astype(np.float64) - got.astype(np.float64)) <= 1.0 * scale
                    ok = bool((close | both_nan).all()) and not explain_check(
                        ([("shift", shift), ("lowpass", (1_000_000, D, T))], W, S, 21_000_000), ref, got)
            if ok and epi != 0 and oracle is not None and not isinstance(a, str) and a.shape[0] > 0:
                # glyph cells / bucket digits against the oracle's: equal, except (with a shift) in windows the NCO rule explains
                ch = oracle.Chain.from_bytes(data.tobytes(), fmt, 21_000_000)
                if shift is not None:
                    ch = ch.shift(shift)
                ch = ch.lowpass(1_000_000, D, T)
                if epi == 1:
                    ref = ch.spark_fft(W, S, max_windows=24, want_norms=False)[1]
                else:
                    ref = ch.freq_levels(W, S, max_windows=24)
                got = a[:ref.shape[0]]
                n_ = ref.shape[0]
                chain = (([("shift", shift)] if shift is not None else []) + [("lowpass", (1_000_000, D, T))], W, S, 21_000_000)
                ok = got.shape == ref.shape and not explain_check(chain, ref.reshape(n_, -1), got.reshape(n_, -1))
            desc = f"fmt={fmt} W={W} S={S} D={D} T={T} shift={shift} N={N} epi={epi} tune={tune} kinds={info}"
            if log:
                log(("ok  " if ok else "BAD ") + desc)
            checked += 1
            if not ok:
                bad.append(desc)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return checked, bad


def fuzz_nofir_shapes(Q, n_shapes, seed, log=None, oracle=None, stats=None):
    """Random chains WITHOUT a lowpass (`from F [shift] sparkfft -width W -stride S`): the plan-time builds of the wave-local kernel family
    (k_spark swizzled, k_spark2, k_spark0, interleaved launches; QD_KERNEL_SPECIALISE) against the generic chain kernel, bit for bit
    without a shift and where the NCO row grids agree (cf32), within the NCO's tolerance otherwise — whole streams and a random window
    sub-range each; with `oracle` (tests only) also against the CPU oracle: bit-exact without a shift, 1 ulp of the window maximum with.
    Returns (checked, mismatching descriptions)."""
    from quadrs_amd import _ffi
    rng = np.random.default_rng(seed)
    checked, bad = 0, []
    for _ in range(n_shapes):
        fmt = int(rng.integers(0, 4))
        W = 1 << int(rng.integers(0, 11))
        S = int(rng.choice([W, W, max(1, W // 2), max(1, W // 4), int(rng.integers(1, W + 1)), int(rng.integers(1, 2 * W + 1))]))
        shift = None if rng.random() < 0.55 else int(rng.integers(-3_000_000, 3_000_000))
        epi = int(rng.choice([0, 0, 1, 2]))
        if epi == 2 and W < 2:
            epi = 0
        bps = {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
        N = int(rng.integers(2, 600)) * S + W + int(rng.integers(0, max(2, S)))
        N = min(N, 300_000)
        data = rng.integers(0, 256, N * bps, dtype=np.uint8)
        if fmt == 0:
            data = (rng.standard_normal((N, 2)).astype(np.float32) * 0.05).view(np.uint8).reshape(-1)
        raw = data.tobytes()
        kw = dict(shift_hz=shift, width=W, stride=S, epilogue=epi, rng=(0.01, 0.5) if fmt == 0 else (0.3, 30.0))
        desc = f"fmt={fmt} W={W} S={S} shift={shift} N={N} epi={epi}"
        try:
            j = Q.Plan(fmt, 21_000_000, N, kernel_policy=_ffi.KERNEL_SPECIALISE, **kw)
            g = Q.Plan(fmt, 21_000_000, N, kernel_policy=_ffi.KERNEL_GENERIC, **kw)
        except Q.QuadrsError as e:
            if log:
                log("skip " + desc + ": " + str(e)[:80])
            continue
        a, b = j.run_host(raw), g.run_host(raw)
        desc += f" kind={j.info.kernel_kind} flags={j.info.kernel_flags}"
        if stats is not None:
            stats.append((int(j.info.kernel_kind), int(j.info.kernel_flags)))

        # bit for bit where the two kernels tile the NCO alike (no shift; cf32 with windows side by side); within the NCO's tolerance where
        # they do not (8-bit formats and cs16: rows of 512 against 1024 samples; overlapping windows behind a shift: a row grid per
        # interleaved launch) — DESIGN section 4.  Sinks that quantise then differ in a cell next to a threshold at most.
        exact = shift is None or (fmt == 0 and S >= W)

        chain = ([("shift", shift)] if shift is not None else [], W, S, 21_000_000)

        def same(x, y, w0=0):
            if x.shape != y.shape:
                return False
            if exact:
                return x.tobytes() == y.tobytes()
            # both within NCO_ABS_ERR of the truth: they may differ only in windows that read an ambiguous multiplier
            if explain_check(chain, y.reshape(y.shape[0], -1), x.reshape(x.shape[0], -1), w0):
                return False
            if x.dtype != np.float32:
                return float((x != y).mean()) <= 5e-3
            scale = ulp_of(np.maximum(np.abs(y).max(axis=-1, keepdims=True), 1e-30)).astype(np.float64)
            return bool((np.abs(x.astype(np.float64) - y.astype(np.float64)) <= scale).all())
        ok = same(a, b)
        nw = j.n_windows
        if ok and nw > 2:
            w0 = int(rng.integers(1, nw))
            cnt = int(rng.integers(1, nw - w0 + 1))
            first, count = j.src_range(w0, cnt)
            sub = j.run_host(raw[first * bps:(first + count) * bps], w0, cnt, src_first=first)
            ok = same(sub, a[w0:w0 + cnt], w0)
            if not ok:
                desc += f" SUB-RANGE w0={w0} cnt={cnt}"
        if ok and epi == 0 and oracle is not None and nw > 0:
            ch = oracle.Chain.from_bytes(raw, fmt, 21_000_000)
            if shift is not None:
                ch = ch.shift(shift)
            ref, _ = ch.spark_fft(W, S, max_windows=32)
            got = a[:ref.shape[0]]
            if shift is None:
                ok = bits_equal(ref, got)
            else:
                scale = ulp_of(np.maximum(np.abs(ref).max(axis=-1, keepdims=True), 1e-30)).astype(np.float64)
                ok = bool((np.abs(ref.astype(np.float64) - got.astype(np.float64)) <= scale).all()) and not explain_check(chain, ref, got)
            if not ok:
                desc += " ORACLE"
        j.close(); g.close()
        if log:
            log(("ok  " if ok else "BAD ") + desc)
        checked += 1
        if not ok:
            bad.append(desc)
    return checked, bad


def full_size_census(Q, O, bench, name):
    """EVERY window of BASELINE workload `name` at its full size: HIP chain kernel against the CPU oracle in its cheapest exact
    form (FIR at the decimated positions only, same products, same order) on all host cores, same input bytes, absolute sample
    indices.  Returns (n_windows, kernel_kind, windows_differing, bins_differing, worst deviation in ulp of the window maximum,
    every differing window as a dict (index, explained by the NCO rule, its replay and the flips the replay found), seconds
    on the GPU side, seconds in the oracle (the comparison pass), threads)."""
    import concurrent.futures as cf
    import os
    import time
    import torch
    dev = torch.device("cuda", 0)
    cores = max(1, min(len(os.sched_getaffinity(0)), 32))
    cfg = bench.WORKLOADS[name]
    t0 = time.perf_counter()
    if name == "cfg4":
        src = torch.empty(cfg["n"], 2, dtype=torch.float32, device=dev)
        tones = [(k - 32) * 1_562_500 + 390_625 for k in range(64)]
        for a in range(0, cfg["n"], 1 << 28):
            Q.gen_device(tones, cfg["sr"], a, src[a:a + (1 << 28)])
    else:
        src = bench.synth_slab(torch, cfg["fmt"], 0, cfg["n"], 0x5EED0002, dev)
    p = Q.Plan(cfg["fmt"], cfg["sr"], cfg["n"], shift_hz=cfg["shift"], lowpass=cfg["lp"], width=cfg["W"], stride=cfg["S"])
    out = torch.empty(p.n_windows, cfg["W"], dtype=torch.float32, device=dev)
    p.run_device(src, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    host = src.view(torch.uint8).reshape(-1).cpu().numpy()
    del src, out
    torch.cuda.empty_cache()
    t_gpu = time.perf_counter() - t0
    # the oracle on the very same bytes; no copy of the slab (the C side reads through the pointer)
    ch = O.Chain()
    ch._node = O.lib().qo_source_mem(O._p(host), host.size, cfg["fmt"], cfg["sr"])
    ch._keep.append(host)
    if cfg["shift"] is not None:
        ch = ch.shift(cfg["shift"])
    ch = ch.lowpass(*cfg["lp"])
    total = O.lib().qo_spark_window_count(ch.len(), cfg["W"], cfg["S"])
    assert total == p.n_windows, (total, p.n_windows)
    piece = 8192
    jobs = [(a, min(piece, total - a)) for a in range(0, total, piece)]

    def work(job):
        a, n = job
        ref, _ = ch.spark_fft(cfg["W"], cfg["S"], first_window=a, max_windows=n, want_codes=False)
        g = got[a:a + n]
        ne = ref.view(np.uint32) != g.view(np.uint32)
        if not ne.any():
            return 0, 0, 0.0, None
        scale = np.spacing(np.abs(ref).max(axis=1, keepdims=True).astype(np.float32)).astype(np.float64)
        err = (np.abs(ref.astype(np.float64) - g.astype(np.float64)) / scale).max()
        rows = np.nonzero(ne.any(axis=1))[0]
        return len(rows), int(ne.sum()), float(err), [int(a + r) for r in rows]

    nw = nb = 0
    worst, diff = 0.0, []
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(cores) as ex:
        for a, b, err, f in ex.map(work, jobs):
            nw += a; nb += b; worst = max(worst, err)
            if f:
                diff += f
    t_cpu = time.perf_counter() - t0
    # every differing window under the NCO rule, and its replay through the oracle's override hook
    stages = ([("shift", cfg["shift"])] if cfg["shift"] is not None else []) + [("lowpass", tuple(cfg["lp"]))]
    desc = (stages, cfg["W"], cfg["S"], cfg["sr"])
    windows = []
    for w in diff:
        ref, _ = ch.spark_fft(cfg["W"], cfg["S"], first_window=w, max_windows=1, want_codes=False)
        detail = {}
        bad = unexplained_windows(ref, got[w:w + 1], lambda v: shift_spans(desc, v), shift_ratios(desc), w, detail)
        combo = replay_window(ch, w, detail.get(w, []), got[w], cfg["W"], cfg["S"]) if not bad else None
        rec = dict(window=w, explained=not bad, ambiguous=len(detail.get(w, [])), replay=combo)
        if combo:
            # what flipped: sample, component, distance of the f64 value to its f32 rounding boundary in f32 ulp
            rec["flips"] = []
            for k, n, comp, v in combo:
                c, s_ = O.shift_multipliers_f64(shift_ratios(desc)[k], n, 1)
                v64 = (c, s_)[comp][0]
                if np.float32(v64) != np.float32(v):
                    mid = (float(np.float32(v64)) + float(np.float32(v))) / 2
                    rec["flips"].append(dict(stage=k, sample=n, comp="cos" if comp == 0 else "sin",
                                             boundary_distance_ulp=abs(v64 - mid) / abs(float(np.spacing(np.float32(v64))))))
        windows.append(rec)
    return total, int(p.info.kernel_kind), nw, nb, worst, windows, t_gpu, t_cpu, cores


def casc_fir_class(D):
    """the FIR class of a cascade decimation (qd_cascade.h casc_fir_class): 0 odd D, 2, 4, 8 a multiple of 8, -1 any other even D"""
    return 0 if D & 1 else (2 if D == 2 else (4 if D == 4 else (8 if D % 8 == 0 else -1)))


def codes_edge_ok(ref_codes, got_codes, ref_norms, rmin, rmax, k_ulp=4):
    """glyph codes (src/fft.rs:54-60) equal the oracle's except where the oracle's own norm lies within k ulp of one of the nine
    decision thresholds min + i*(max-min)/7.  Returns (ok, differing cells, of them near a threshold)."""
    diff = ref_codes != got_codes
    step = (np.float32(rmax) - np.float32(rmin)) / np.float32(7.0)
    edges = np.array([np.float32(rmin) + np.float32(i) * step for i in range(8)] + [np.float32(rmax)], dtype=np.float32)
    nd = ref_norms[diff].astype(np.float64)
    near = np.zeros(nd.shape, dtype=bool)
    for e in edges:
        near |= np.abs(nd - float(e)) <= k_ulp * float(np.spacing(np.float32(e)))
    return bool(near.all()), int(diff.sum()), int(near.sum())


def bucket_digits_ok(ref_norms, got_digits):
    """bucket digits (src/fft.rs:95-97: two sequential f32 half sums of the norms in natural bin order) against the oracle's norms
    of the same windows; a digit may differ only where the two sums tie within 8 ulp

    What the excuse is for: chains with a shift stage, where an NCO multiplier next to an f32 rounding boundary moves a norm by an
    ulp and with it a near-tie (the NCO rule).  It says nothing about the ORDER of the sums — on streams whose halves tie it accepts
    the digits of a pairwise summation (test_bucket_order_cpu.py asserts that).  Exactness of the sum order and of the tie rule is
    held by test_gpu_bucket_order.py, on shift-free chains, without any excuse."""
    W = ref_norms.shape[1]
    nat = np.roll(ref_norms, W // 2, axis=1)                       # the sparkfft rows' fftshift undone
    first = np.cumsum(nat[:, : W // 2], axis=1, dtype=np.float32)[:, -1] if W > 1 else np.zeros(len(nat), np.float32)
    second = np.cumsum(nat[:, W // 2:], axis=1, dtype=np.float32)[:, -1]
    want = np.where(first < second, 0, 1).astype(np.uint8)
    tie = np.abs(first.astype(np.float64) - second) <= 8 * np.spacing(np.maximum(first, second)).astype(np.float64)
    return not ((want != got_digits) & ~tie).any()


def fuzz_cascade_shapes(Q, n_shapes, seed, oracle, log=None, cov=None, observed=None):
    """Random cascaded stage lists (qd_plan_create_stages, k_cascade: every fused shape [S] L [S] [L [S]], every format and sink,
    D 1 ... 32 of every FIR class, T not a multiple of 8, W 1 ... 8192 up to the n2 <= 8192 envelope, any stride, sample rates the
    decimations do not divide, shifts of 0 and +-(rate/2 - 1) at each stage's rate) against the CPU oracle's nested Samples on the
    first and the last 16 complete windows: norms bit-exact without a shift, within 1 ulp of the window maximum with one (the
    aggregate bit-exact fraction goes to `observed`); glyph codes edge-aware, bucket digits up to ties.  Each shape also runs a
    window sub-range from an offset slab and a 64 KiB-chunk host run, which must give the whole run's bytes.
    `cov` (a dict) collects the FIR classes, T % 8 != 0, the sub-tile sizes (M, min(n2, 512)) and the shapes reached.  Returns (checked, mismatching descriptions)."""
    import re
    rng = np.random.default_rng(seed)
    checked, bad = 0, []
    cov = {} if cov is None else cov
    for key in ("cls1", "cls2", "t1_mod8", "t2_mod8", "M", "shapes", "short"):
        cov.setdefault(key, set() if key != "short" else 0)
    observed = {} if observed is None else observed
    observed.setdefault("bins", 0)
    observed.setdefault("exact", 0)
    observed.setdefault("worst_ulp", 0.0)
    DS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 24, 32]
    TS = [2, 4, 6, 10, 16, 22, 40, 42, 64, 90, 100, 128, 200, 258, 400]
    for _ in range(n_shapes):
        fmt = int(rng.integers(0, 4))
        epi = int(rng.choice([0, 0, 1, 2]))
        l2 = rng.random() < 0.6
        s0, s1 = rng.random() < 0.5, rng.random() < 0.5 or not l2
        s2 = l2 and rng.random() < 0.5
        D1, T1 = int(rng.choice(DS)), int(rng.choice(TS))
        D2, T2 = (int(rng.choice(DS)), int(rng.choice(TS))) if l2 else (1, 0)
        if rng.random() < 0.15:                       # long first stages: with D1 large, the sub-tile halves below 512 outputs
            T1, D1 = int(rng.choice([1000, 2050, 4096])), int(rng.choice([6, 10, 16, 24, 32]))
        lim = 8192 if rng.random() < 0.15 else 1024
        W = 1 << int(rng.integers(0, 14))
        while W > 1 and ((W * D2 + T2 if l2 else W) > lim or (W * D2 + T2 if l2 else W) * T1 > 3_000_000):
            W //= 2
        n2 = W * D2 + T2 if l2 else W
        if n2 > 8192:
            continue
        S = int(rng.choice([W, max(1, W // 4), 2 * W, int(rng.integers(1, 2 * W + 1))]))
        sr = int(rng.integers(1_000_000, 30_000_000))
        r1 = sr // D1
        r2 = r1 // D2
        if r2 < 4:
            continue

        def shift_at(rate):
            lim2 = rate // 2
            return int(rng.choice([0, lim2 - 1, -(lim2 - 1), int(rng.integers(-(lim2 - 1), lim2))]))
        stages = []
        if s0:
            stages.append(("shift", shift_at(sr)))
        stages.append(("lowpass", (int(rng.integers(1, sr // 2)), D1, T1)))
        if s1:
            stages.append(("shift", shift_at(r1)))
        if l2:
            stages.append(("lowpass", (int(rng.integers(1, r1 // 2)), D2, T2)))
            if s2:
                stages.append(("shift", shift_at(r2)))
        span, step = n2 * D1 + T1, S * D2 * D1
        N = span + int(rng.integers(20, 80)) * step + int(rng.integers(0, 2 * D1 * D2 + 1))
        bps = {0: 8, 1: 2, 2: 2, 3: 4}[fmt]
        data = rng.integers(0, 256, N * bps, dtype=np.uint8)
        if fmt == 0:
            data = (rng.standard_normal((N, 2)).astype(np.float32) * 0.05).view(np.uint8).reshape(-1)
        raw = data.tobytes()
        u_w0, u_cnt = rng.random(), rng.random()      # the sub-range, drawn up front: what a shape draws never depends on a result
        shape = "".join(k[0].upper() for k, _ in stages)
        shifted = any(k == "shift" and a != 0 for k, a in stages)
        desc = f"fmt={fmt} epi={epi} {shape} stages={stages} sr={sr} W={W} S={S} N={N}"
        done = total = 0
        try:
            ch = oracle.Chain.from_bytes(raw, fmt, sr)
            for kind, arg in stages:
                ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
            p0 = Q.Plan(fmt, sr, N, stages=stages, width=W, stride=S, epilogue=2 if epi == 2 else 0)
            done, total = p0.complete_windows(), p0.n_windows          # the bucket sink's loop is one window shorter or equal
            # the windows compared with the oracle: the first and the last 16 complete ones
            heads = [(0, min(16, done))] + ([(max(16, done - 16), done - max(16, done - 16))] if done > 16 else [])
            refs = [ch.spark_fft(W, S, first_window=a, max_windows=c, want_codes=False)[0] for a, c in heads]
            rng_g = None
            if epi == 1:
                allr = np.concatenate(refs).ravel()
                lo, hi = np.percentile(allr, [20, 90])
                rng_g = (float(lo), float(max(hi, lo * 1.5 + 1e-6)))
            p = p0 if epi != 1 else Q.Plan(fmt, sr, N, stages=stages, width=W, stride=S, epilogue=epi, rng=rng_g)
            M = int(re.search(r"M (\d+)\)", p.kernel_name()).group(1))
            whole = p.run_host(raw, n_windows=done)
            ok = whole.shape[0] == done
            for (a, c), ref in zip(heads, refs):
                if not ok or c == 0:
                    break
                got = whole[a:a + c]
                if epi == 0:
                    ex = ref.view(np.uint32) == got.view(np.uint32)
                    scale = ulp_of(ref.max(axis=-1, keepdims=True)).astype(np.float64)
                    worst = float((np.abs(ref.astype(np.float64) - got.astype(np.float64)) / scale).max())
                    observed["bins"] += int(ex.size)
                    observed["exact"] += int(ex.sum())
                    observed["worst_ulp"] = max(observed["worst_ulp"], worst)
                    ok = bool(ex.all()) if not shifted else (worst <= 1.0 and not explain_check((stages, W, S, sr), ref, got, a))
                elif epi == 1:
                    rn, rc = ch.spark_fft(W, S, rng=rng_g, first_window=a, max_windows=c)
                    ok = codes_edge_ok(rc, got, rn, *rng_g)[0]
                    # a differing cell is also in a window the NCO rule explains (shift-free: no cell differs)
                    ok = ok and not explain_check((stages, W, S, sr), rc, got, a)
                else:
                    ok = bucket_digits_ok(ref, got)
                    lv = ch.freq_levels(W, S, max_windows=a + c)[a:a + c]
                    ok = ok and lv.shape == got.shape and not explain_check((stages, W, S, sr), lv.reshape(c, 1), got.reshape(c, 1), a)
                if not ok:
                    desc += f" ORACLE windows [{a}, +{c})"
            if ok and done > 1:
                w0 = 1 + int(u_w0 * (done - 1))
                cnt = 1 + int(u_cnt * (done - w0))
                first, count = p.src_range(w0, cnt)
                sub = p.run_host(raw[first * bps:(first + count) * bps], w0, cnt, src_first=first)
                ok = sub.tobytes() == whole[w0:w0 + cnt].tobytes()
                if not ok:
                    desc += f" SUB-RANGE w0={w0} cnt={cnt}"
            if ok:
                small = Q.Plan(fmt, sr, N, stages=stages, width=W, stride=S, epilogue=epi, rng=rng_g, chunk_bytes=1 << 16)
                ok = small.run_host(raw, n_windows=done).tobytes() == whole.tobytes()
                small.close()
                if not ok:
                    desc += " CHUNKED"
            if p is not p0:
                p.close()
            p0.close()
        except (Q.QuadrsError, RuntimeError) as e:
            ok, M = False, None
            desc += f" ERROR {e}"
        cov["cls1"].add(casc_fir_class(D1))
        if l2:
            cov["cls2"].add(casc_fir_class(D2))
            cov["t2_mod8"].add(T2 % 8 != 0)
        cov["t1_mod8"].add(T1 % 8 != 0)
        cov["M"].add((M, min(n2, 512)))                # the sub-tile against the one it starts from: below it, cascade_init halved
        cov["shapes"].add(shape)
        cov["short"] += ok and done < total
        if log:
            log(("ok  " if ok else "BAD ") + desc + f" M={M} complete={done}/{total}")
        checked += 1
        if not ok:
            bad.append(desc)
    return checked, bad


# ------------------------------------------------------------------ the NCO rule
#
# A shifted result may differ from the oracle only where the NCO explains it: in a window that reads a sample whose reference
# multiplier component is ambiguous, i.e. whose glibc f64 value lies within NCO_ABS_ERR of an f32 rounding boundary.

NCO_ABS_ERR = 2e-15
"""Absolute bound on |device f64 multiplier component - glibc f64 cos/sin(place)| before the f32 casts (qd_device.h, nco_*).
Every value involved has magnitude <= 1, where 1 ulp of f64 is <= 2^-53 = 1.1e-16 and a rounding costs <= 0.56e-16.
  * table entries (nco_table_entry): the device sincos of the rounded product, <= 2 ulp = 2.2e-16, plus the final rounding of
    the lo-correction, 0.56e-16 (its dropped lo^4/24 is < 1e-23 for |lo| <= 2^-18): <= 2.8e-16 per entry;
  * rotation (nco_mul: C = rb.c lr.c - rb.s lr.s, S alike): the entries' errors weighted by |lr.c| + |lr.s| <= sqrt 2 and
    |rb.c| + |rb.s| <= sqrt 2, 2 sqrt 2 * 2.8e-16 = 7.9e-16, plus the product's and the fma's roundings, 1.1e-16: <= 9.0e-16;
  * residual correction (c = C + r S - ...): at most two roundings, 1.1e-16; r times the rotation's error is < 1e-21;
  * the dropped term: r^2/2 <= 1.1e-16 on the first-order form (|place| <= 2^28 rad, |r| <= 2^-26); r^3/6 < 1e-17 on the
    second-order form (|place| < 2^36 rad, |r| <= 2^-18: every 2^34-sample stream at any shift);
  * glibc's own cos/sin, < 1 ulp: 1.1e-16.
Sum 1.23e-15; the bound keeps a margin of 1.6x.  The rule's mutation tests need it below 1e-14: never raise it to pass a test."""


def _f32_round_exact(t, e):
    """f32 round-to-nearest-even of the exact reals t + e (t float64, e the exact residual of t with |e| <= ulp(t)/2)"""
    f = t.astype(np.float32)
    f64 = f.astype(np.float64)
    up = np.nextafter(f, np.float32(np.inf))
    dn = np.nextafter(f, np.float32(-np.inf))
    mid_up = (f64 + up.astype(np.float64)) * 0.5            # exact in f64
    mid_dn = (f64 + dn.astype(np.float64)) * 0.5
    # t lies exactly on a midpoint: the residual's sign decides; otherwise t + e rounds like t (a midpoint is >= 1 f64 ulp away)
    f = np.where((t == mid_up) & (e > 0), up, f)
    f = np.where((t == mid_dn) & (e < 0), dn, f)
    return f


def nco_candidates(v64, eps=NCO_ABS_ERR):
    """(lo32, hi32): the smallest and the largest f32 that round-to-nearest gives for any real x in [v - eps, v + eps], per
    element of the f64 array v64.  Every f32 in [lo32, hi32] is such a value (rounding is monotone).  A component is
    ambiguous where lo32 != hi32."""
    v = np.asarray(v64, dtype=np.float64)
    out = []
    for b in (-eps, eps):
        t = v + b                                            # TwoSum: v + b == t + e exactly
        bb = t - v
        e = (v - (t - bb)) + (b - bb)
        out.append(_f32_round_exact(t, e))
    return out[0], out[1]


def _chain_of(desc):
    """(stages, W, S, sample_rate) of a Plan, or of a tuple (stages, W, S[, sample_rate])"""
    if isinstance(desc, tuple):
        stages, W, S = desc[0], desc[1], desc[2]
        return list(stages), int(W), int(S), (int(desc[3]) if len(desc) > 3 else None)
    d = desc.desc
    stages = desc.stages
    if stages is None:
        stages = ([("shift", int(d.shift_hz))] if d.has_shift else []) + \
                 ([("lowpass", (int(d.lowpass_hz), int(d.decimate), int(d.taps)))] if d.has_lowpass else [])
    return list(stages), int(d.width), int(d.stride), int(d.sample_rate)


def shift_ratios(desc):
    """the ratio of each shift stage, source to sink: TAU * f / (that stage's input rate) (src/shift.rs:28)"""
    import math
    stages, _, _, sr = _chain_of(desc)
    out = []
    for kind, arg in stages:
        if kind == "shift":
            out.append(math.tau * float(arg) / float(sr))
        else:
            sr //= int(arg[1])
    return out


def shift_spans(desc, window):
    """For each shift stage (source to sink): the half-open range [lo, hi) of absolute indices, at that stage's rate, that
    sink window `window` (an int or an int array) reads — window w reads [w S, w S + W) of the last stage (spark_fft, and the
    write sink's blocks with S = W = B).  A lowpass (D, T) serves a read of outputs [b0, b1) with ONE block read [b0 D, b1 D + T)
    of its input, and output k of it reads inputs k D + c ... k D + c + T - 1 (c = T - T/2, src/filter.rs:68-83,
    complex_convolve's kept outputs) that lie inside that block.  So the block and the dependency range [lo, hi) are carried
    separately: lo' = lo D + c, hi' = min((hi - 1) D + c + T, b1 D + T), block' = [b0 D, b1 D + T).  Exact, up to the tail
    truncation of a block, which only removes samples: never inward, outward by less than one FIR length per stage.  With a
    Plan the source-rate spans are checked to lie in its src_range."""
    stages, W, S, _ = _chain_of(desc)
    w = np.asarray(window, dtype=np.int64)
    lo, hi = w * S, w * S + W
    b0, b1 = lo, hi                                          # the block read at this stage's rate
    spans = []
    for kind, arg in reversed(stages):
        if kind == "shift":
            spans.append((lo, hi))
        else:
            D, T = int(arg[1]), int(arg[2])
            c = T - T // 2
            lo, hi = lo * D + c, np.minimum((hi - 1) * D + c + T, b1 * D + T)
            b0, b1 = b0 * D, b1 * D + T
    spans.reverse()
    if not isinstance(desc, tuple) and np.ndim(window) == 0 and stages and stages[0][0] == "shift":
        a, n = desc.src_range(int(window), 1)
        assert a <= int(spans[0][0]) and int(spans[0][1]) <= a + n, (spans[0], a, n)
    if np.ndim(window) == 0:
        spans = [(int(a), int(b)) for a, b in spans]
    return spans


def ambiguous_components(ratio, lo, hi, eps=NCO_ABS_ERR):
    """the ambiguous multiplier components of samples [lo, hi) of a shift with `ratio`: a list of (n, comp, candidates),
    comp 0 = cos / 1 = sin, candidates the f32 values round-to-nearest may give (float32 array; None past 64 of them)"""
    from oracle import oracle as O
    out = []
    if hi <= lo:
        return out
    c, s = O.shift_multipliers_f64(ratio, lo, hi - lo)
    for comp, v in ((0, c), (1, s)):
        a, b = nco_candidates(v, eps)
        for i in np.nonzero(a != b)[0]:
            ia, ib = int(a[i:i + 1].view(np.int32)[0]), int(b[i:i + 1].view(np.int32)[0])
            cand = None                                      # a zero crossing, or too many values to enumerate
            if (a[i] > 0 or b[i] < 0) and abs(ib - ia) <= 64:
                cand = np.arange(min(ia, ib), max(ia, ib) + 1, dtype=np.int64).astype(np.int32).view(np.float32)
            out.append((int(lo + i), comp, cand))
    return out


def ambiguous_windows(desc, windows):
    """how many of the sink windows `windows` (absolute indices, any order) of a Plan or (stages, W, S, sample_rate) read an ambiguous
    multiplier component of some shift stage: the windows in which the NCO rule would excuse a difference"""
    w = np.asarray(windows, dtype=np.int64).reshape(-1)
    hit = np.zeros(w.size, dtype=bool)
    if w.size == 0:
        return 0
    d = desc if isinstance(desc, tuple) else _chain_of(desc)
    for (lo, hi), ratio in zip(shift_spans(tuple(d), w), shift_ratios(desc)):
        at = np.array(sorted({n for n, _, _ in ambiguous_components(ratio, int(lo.min()), int(hi.max()))}), dtype=np.int64)
        # window i reads an ambiguous sample iff one lies in [lo_i, hi_i)
        hit |= np.searchsorted(at, hi, side="left") > np.searchsorted(at, lo, side="left")
    return int(hit.sum())


REAL_TIE_GAP = 1e-13
"""A multiplier component is a REAL tie where its nco_candidates pair (lo32, hi32) lies further apart than this.  The bound of the
Bluestein rows (2 ulp_f32 of the reference norm + 1e-12 of the row's l1 norm) holds without any excuse as long as the rows read no
real tie: a component that moves by g moves a bin by at most g |x| <= g l1, a tenth of the bound's l1 term at g = 1e-13.  Zero
crossings (|v| < 3e-8, where the f32 grid is finer than 2 NCO_ABS_ERR) are ambiguous but 1e-19 ... 1e-14 apart: no real ties."""


def real_ties(ratio, lo, n, gap=REAL_TIE_GAP, eps=NCO_ABS_ERR):
    """(number of ambiguous multiplier components, the real ties among them as [(sample, comp, lo32, hi32), ...]) of samples
    [lo, lo + n) of a shift with `ratio`; comp 0 = cos / 1 = sin"""
    from oracle import oracle as O
    ambiguous, ties = 0, []
    if n <= 0:
        return ambiguous, ties
    for comp, v in enumerate(O.shift_multipliers_f64(ratio, int(lo), int(n))):
        a, b = nco_candidates(v, eps)
        ambiguous += int((a != b).sum())
        far = np.nonzero(b.astype(np.float64) - a.astype(np.float64) > gap)[0]
        ties += [(int(lo) + int(i), comp, float(a[i]), float(b[i])) for i in far]
    return ambiguous, ties


def differing_windows(ref, got):
    """rows (windows) whose bytes differ, NaN-aware: a NaN against a NaN is no difference"""
    ref = np.ascontiguousarray(ref)
    got = np.ascontiguousarray(got)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    n = ref.shape[0]
    a = ref.reshape(n, -1)
    b = got.reshape(n, -1)
    ne = a.view(np.uint8).reshape(n, -1) != b.view(np.uint8).reshape(n, -1)
    if a.dtype.kind == "f":
        ne = (a.view(np.uint32 if a.itemsize == 4 else np.uint64) != b.view(np.uint32 if a.itemsize == 4 else np.uint64)) & \
             ~(np.isnan(a) & np.isnan(b))
    return np.nonzero(ne.any(axis=1))[0]


def unexplained_windows(ref, got, spans_fn, ratios, first_window=0, detail=None, eps=NCO_ABS_ERR):
    """The NCO rule.  The windows (absolute indices first_window + row) in which ref and got differ at all (bytes, NaN-aware) but
    whose spans_fn(w) (one [lo, hi) per shift stage, see shift_spans) hold no ambiguous multiplier component of that stage's
    ratio.  Ambiguity is computed over the differing windows' spans only.  With `detail` (a dict) every differing window maps
    to its ambiguous components [(stage, n, comp, candidates), ...]."""
    bad = []
    for r in differing_windows(ref, got):
        w = first_window + int(r)
        amb = []
        for k, ((lo, hi), ratio) in enumerate(zip(spans_fn(w), ratios)):
            amb += [(k,) + a for a in ambiguous_components(ratio, int(lo), int(hi), eps)]
        if detail is not None:
            detail[w] = amb
        if not amb:
            bad.append(w)
    return bad


def explain_check(desc, ref, got, first_window=0, detail=None):
    """unexplained_windows for a Plan (or (stages, W, S, sample_rate)) whose windows first_window ... are ref / got"""
    return unexplained_windows(ref, got, lambda w: shift_spans(desc, w), shift_ratios(desc), first_window, detail)


def _window_eval(chain, w, width, stride, sink):
    if sink == "blocks":
        n, out = chain.read_at(w * width, width)
        return out if n == width else None
    return chain.spark_fft(width, stride, first_window=w, max_windows=1, want_codes=False)[0]


def replay_window(chain, w, ambiguous, got_w, width, stride=None, sink="norms", limit=256):
    """Replay window w of the oracle Chain through the shift override hook with other candidate values of its ambiguous
    components (as unexplained_windows reports them in `detail`): first every single component changed to each of its other
    candidates, then every pair, the components of largest magnitude first, at most `limit` replays.  Components with too
    many candidates to enumerate (zero crossings) keep the reference's value.  Returns the combination
    [(stage, n, comp, value), ...] of every enumerated component whose output equals got_w bit for bit (NaN-aware), or
    None.  The hook is cleared on return."""
    import itertools
    from oracle import oracle as O
    stride = width if stride is None else stride
    amb = sorted((a for a in ambiguous if a[3] is not None), key=lambda a: -float(np.abs(a[3]).max()))
    if not amb:
        return None
    got_w = np.asarray(got_w).reshape(1, -1)
    base = {}
    for k, n, comp, cand in amb:
        if (k, n) not in base:
            c, s = O.shift_multipliers_f64(chain.shift_ratios[k], n, 1)
            base[(k, n)] = [np.float32(c[0]), np.float32(s[0])]
    alts = [[v for v in a[3] if v != base[(a[0], a[1])][a[2]]] for a in amb]

    def combos():
        for r in (1, 2):
            for idx in itertools.combinations(range(len(amb)), r):
                for vals in itertools.product(*[alts[i] for i in idx]):
                    yield dict(zip(idx, vals))
    try:
        for tried, change in enumerate(combos()):
            if tried >= limit:
                return None
            mults = {key: list(v) for key, v in base.items()}
            for i, val in change.items():
                k, n, comp, _ = amb[i]
                mults[(k, n)][comp] = val
            for k in {key[0] for key in mults}:
                ns = [n for (kk, n) in mults if kk == k]
                chain.override_shift(k, ns, [mults[(k, n)][0] for n in ns], [mults[(k, n)][1] for n in ns])
            out = _window_eval(chain, w, width, stride, sink)
            if out is not None and len(differing_windows(np.asarray(out).reshape(1, -1), got_w)) == 0:
                return [(a[0], a[1], a[2], float(change.get(i, base[(a[0], a[1])][a[2]]))) for i, a in enumerate(amb)]
    finally:
        for k in range(len(chain.shift_nodes)):
            chain.override_shift(k, [], [], [])
    return None


def _two_prod_err(a, b):
    """the exact rounding error of the f64 product a*b (Dekker): a*b == fl(a*b) + err"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    al = a - ah
    bh = cb - (cb - b)
    bl = b - bh
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


def nco_sensitive_samples(ratio, n0, count, chunk=1 << 22, eps=NCO_ABS_ERR):
    """Samples n in [n0, n0 + count) with a component that is NOT ambiguous and yet lies closer to its f32 rounding boundary
    than the second-order term r^2/2 |v| of the reference's residual r = n ratio - fl(n ratio): an NCO that drops that term
    rounds it the other way, a correct one must give the reference's bits.  Returns the sorted indices (numpy int64)."""
    from oracle import oracle as O
    found = []
    for a in range(n0, n0 + count, chunk):
        n = np.arange(a, min(a + chunk, n0 + count), dtype=np.float64)
        r = _two_prod_err(n, np.float64(ratio))
        place = n * ratio
        d = 0.5 * r * r                                      # relative size of the dropped term
        keep = d > 4 * eps
        n, place, d = n[keep], place[keep], d[keep]
        for v in (np.cos(place), np.sin(place)):            # a pre-selection; the survivors are re-checked on glibc's values
            f = v.astype(np.float32)
            out = np.nextafter(f, np.where(v < 0, np.float32(-np.inf), np.float32(np.inf)).astype(np.float32))
            dist = np.abs((f.astype(np.float64) + out.astype(np.float64)) / 2) - np.abs(v)
            sel = (dist > 3 * eps) & (dist < np.abs(v) * d - 3 * eps)
            found += [int(x) for x in n[sel]]
    out = []
    for k in sorted(set(found)):
        c, s = O.shift_multipliers_f64(ratio, k, 1)
        r = float(_two_prod_err(np.float64(k), np.float64(ratio)))
        for v in (c[0], s[0]):
            lo, hi = nco_candidates(np.array([v]), eps)
            f = np.float32(v)
            nb = np.nextafter(f, np.float32(-np.inf) if v < 0 else np.float32(np.inf))
            dist = abs((float(f) + float(nb)) / 2) - abs(v)
            if lo[0] == hi[0] and 2 * eps < dist < abs(v) * 0.5 * r * r - 2 * eps:
                out.append(k)
                break
    return np.array(out, dtype=np.int64)


# ------------------------------------------------------------------ footprints: which memory a run reads and writes
#
# A run of windows [w0, w0 + n) may read source samples src_range(w0, n) and nothing else, and write n * out_bytes_per_window
# bytes and nothing else (include/quadrs_hip.h).  The source slab and the output are laid INSIDE one allocation each, between
# frames the test owns:  [front frame | slab | back frame]  and  [guard | payload | guard].  Source frames hold a poison
# pattern, and every case runs twice, once per pattern: cf32 frames are 0x7FC00000 words (a quiet NaN, which survives a
# multiplication by a zero tap) and then 0x7F7FFFFF words (the largest finite f32).  The integer formats have no NaN: their
# frames are 0x80 bytes and then 0x7F bytes, and an influence of the frames shows ONLY as a difference between the two runs.
# Output guards and the payload itself are pre-filled with 0xA5, so a window that was never written does not look like zeros.
# Reads whose values are discarded cannot be seen by this method.

POISON_WORDS = (0x7FC00000, 0x7F7FFFFF)        # cf32 frames
POISON_BYTES = (0x80, 0x7F)                    # cs8 / cu8 / cs16 frames
GUARD_BYTE = 0xA5
FMT_BYTES = {0: 8, 1: 2, 2: 2, 3: 4}


def poison(fmt, nbytes, which):
    """nbytes (a multiple of 4) of source poison pattern `which` (0 / 1) for sample format fmt, as a uint8 array"""
    assert nbytes % 4 == 0
    if fmt == 0:
        return np.full(nbytes // 4, POISON_WORDS[which], dtype="<u4").view(np.uint8)
    return np.full(nbytes, POISON_BYTES[which], dtype=np.uint8)


def _round_up(x, q):
    return (int(x) + q - 1) // q * q


def src_frame_bytes(info, fmt):
    """the least size of a source frame: max(1 MiB, 4 x the plan's source span of one tile), kept a multiple of 4 KiB so that
    the slab keeps the allocation's alignment.  A condition, not a measurement."""
    tile_span = (max(int(info.tile_windows), 1) - 1) * int(info.raw_step) + int(info.raw_per_window)
    return _round_up(max(1 << 20, 4 * tile_span * FMT_BYTES[fmt]), 4096)


def out_guard_bytes(info):
    """the least size of an output guard: max(64 KiB, 4 tiles of output), a multiple of 4 KiB"""
    return _round_up(max(64 << 10, 4 * max(int(info.tile_windows), 1) * int(info.out_bytes_per_window)), 4096)


class Framed:
    """[front | body | back] in ONE allocation of device ("device": a torch uint8 tensor), pageable host ("host": numpy) or
    pinned host ("pinned": a PinnedBuffer of `engine`) memory.  `body` is what a run is handed (a view that starts at the body's
    first byte); `uploaded` the bytes the buffer was created with; snapshot() its bytes now."""

    def __init__(self, kind, front, body, back, engine=None):
        parts = [np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in (front, body, back)]
        self.kind = kind
        self.lo = parts[0].size
        self.hi = self.lo + parts[1].size
        self.uploaded = np.concatenate(parts)
        if kind == "device":
            import torch
            self._buf = torch.from_numpy(self.uploaded.copy()).cuda()
        elif kind == "pinned":
            self._pin = engine.PinnedBuffer(self.uploaded.size)
            self._buf = self._pin.array
            self._buf[:] = self.uploaded
        else:
            assert kind == "host", kind
            self._buf = self.uploaded.copy()
        self.body = self._buf[self.lo:self.hi]

    def snapshot(self):
        if self.kind == "device":
            import torch
            torch.cuda.synchronize()
            return self._buf.cpu().numpy()
        return np.array(self._buf, copy=True)

    def close(self):
        self.body = self._buf = None
        if self.kind == "pinned":
            self._pin.close()


def framed(kind, fmt, which, front_bytes, slab, back_bytes, engine=None):
    """a source slab (bytes / uint8 array) between frames of poison pattern `which`"""
    slab = np.frombuffer(slab, dtype=np.uint8) if not isinstance(slab, np.ndarray) else slab
    return Framed(kind, poison(fmt, front_bytes, which), slab, poison(fmt, back_bytes, which), engine)


def framed_out(kind, guard_bytes, payload_bytes, engine=None, fill=GUARD_BYTE):
    """an output of payload_bytes between two guards, all three filled with `fill` (GUARD_BYTE)"""
    g = np.full(guard_bytes, fill, dtype=np.uint8)
    return Framed(kind, g, np.full(payload_bytes, fill, dtype=np.uint8), g, engine)


class FootprintRun:
    """what one framed run left behind: the output buffer's bytes (guards and payload) and, where the source lives in memory a
    kernel could write (device, pinned), the source buffer's bytes against what was uploaded"""

    def __init__(self, out, src=None):
        snap = out.snapshot()
        self.front, self.payload, self.back = snap[:out.lo], snap[out.lo:out.hi], snap[out.hi:]
        self.src_uploaded = self.src_now = None
        if src is not None and src.kind != "host":
            self.src_uploaded, self.src_now = src.uploaded, src.snapshot()


def footprint_violations(runs, ref, rule=None, unit=4):
    """The footprint checker.  runs: the FootprintRun of each poison pattern (two), same windows, same true slab.  ref: the
    ORACLE's payload for those windows on the true stream (an array whose bytes are laid out like the payload).  rule(got
    payload bytes) -> a list of complaints holds the payload to the chain's rule against the oracle; None means bit for bit.
    unit: bytes per output element (4: f32 words, 1: glyph cells / bucket digits).  Returns the violated conditions:
      1. "poison": the two patterns' payloads differ (memory outside the slab reached an output byte);
      2. "oracle": the payload breaks the rule;
      3. "unwritten": an output element still holds the pre-fill where the oracle's value is something else;
      4. "guard": a byte of an output guard changed;
      5. "source": a byte of the source buffer (frames or slab) changed."""
    bad = []
    ref_b = np.ascontiguousarray(ref).view(np.uint8).reshape(-1)
    if len(runs) != len(POISON_WORDS):
        bad.append(f"poison: {len(runs)} runs, one per pattern is {len(POISON_WORDS)}")
    for r in runs[1:]:
        if r.payload.size != runs[0].payload.size or not np.array_equal(r.payload, runs[0].payload):
            d = np.flatnonzero(r.payload != runs[0].payload) if r.payload.size == runs[0].payload.size else []
            bad.append(f"poison: payloads of the two fills differ in {len(d)} bytes, first at byte {int(d[0]) if len(d) else -1}")
    for k, r in enumerate(runs):
        if r.payload.size != ref_b.size:
            bad.append(f"oracle: fill {k}: payload of {r.payload.size} bytes, the oracle's has {ref_b.size}")
            continue
        if rule is None:
            d = np.flatnonzero(r.payload != ref_b)
            if d.size:
                bad.append(f"oracle: fill {k}: {d.size} bytes differ from the oracle, first at byte {int(d[0])}")
        else:
            bad += [f"oracle: fill {k}: {c}" for c in rule(r.payload)]
        fill = np.uint8(GUARD_BYTE) if unit == 1 else np.uint32(0x01010101 * GUARD_BYTE)
        dt = np.uint8 if unit == 1 else np.uint32
        stale = np.flatnonzero((r.payload.view(dt) == fill) & (ref_b.view(dt) != fill))
        if stale.size:
            bad.append(f"unwritten: fill {k}: {stale.size} output elements still hold the pre-fill, first element {int(stale[0])}")
        for name, g in (("front", r.front), ("back", r.back)):
            d = np.flatnonzero(g != GUARD_BYTE)
            if d.size:
                where = int(d[0]) if name == "back" else int(d[-1]) - g.size
                bad.append(f"guard: fill {k}: {d.size} bytes of the {name} guard were written, nearest at {where:+d} bytes from the payload")
        if r.src_now is not None and not np.array_equal(r.src_now, r.src_uploaded):
            d = np.flatnonzero(r.src_now != r.src_uploaded)
            bad.append(f"source: fill {k}: {d.size} bytes of the source buffer changed, first at byte {int(d[0])}")
    return bad


def footprint_reference(oracle_chain, stages, sr, W, S, epi, rng, n_total):
    """The oracle's outputs of windows [0, n_total) of a chain on the TRUE stream and the rule a run of any sub-range is held to:
    returns expect(w0, n) -> (ref, rule, unit) for footprint_violations.  Norms (epi 0) and write blocks (3) are bit for bit
    without a shift stage and obey the NCO rule (explain_check) within 1 ulp of the window maximum / the sample's magnitude
    with one; glyph cells (1) obey codes_edge_ok, bucket digits (2) bucket_digits_ok, both also the NCO rule behind a shift."""
    shifted = any(k == "shift" and a != 0 for k, a in stages)
    desc = (list(stages), W, S, sr)
    if epi == 3:
        rows = []
        for b in range(n_total):
            got, blk = oracle_chain.read_at(b * W, W)
            assert got == W, (b, got)
            rows.append(blk.reshape(-1))
        ref_all = np.stack(rows) if rows else np.zeros((0, 2 * W), np.float32)
        norms_all = None
    else:
        norms_all, codes_all = oracle_chain.spark_fft(W, S, rng=rng if epi == 1 else None, max_windows=n_total, want_codes=(epi == 1))
        assert norms_all.shape[0] == n_total, (norms_all.shape, n_total)
        ref_all = norms_all if epi == 0 else codes_all if epi == 1 else oracle_chain.freq_levels(W, S, max_windows=n_total).reshape(-1, 1)
        assert ref_all.shape[0] == n_total, (ref_all.shape, n_total)

    def expect(w0, n):
        ref = np.ascontiguousarray(ref_all[w0:w0 + n])

        def rule(payload):
            got = payload.view(ref.dtype).reshape(ref.shape)
            out = []
            if epi == 0:
                scale = ulp_of(np.maximum(np.abs(ref).max(axis=-1, keepdims=True), 1e-30)).astype(np.float64)
                with np.errstate(invalid="ignore"):
                    worst = np.abs(ref.astype(np.float64) - got.astype(np.float64)) / scale
                if not (worst <= 1.0).all():
                    out.append(f"norms further than 1 ulp of the window maximum (or NaN), first window {w0 + int(np.nonzero(~(worst <= 1.0))[0][0])}")
            elif epi == 3:
                with np.errstate(invalid="ignore"):
                    err = complex_ulp_err(ref, got)
                if not (err <= 1.0).all():
                    out.append(f"block samples further than 1 ulp, first sample {w0 * W + int(np.nonzero(~(err <= 1.0))[0][0])}")
            elif epi == 1:
                ok, differing, near = codes_edge_ok(ref, got, norms_all[w0:w0 + n], rng[0], rng[1])
                if not ok:
                    out.append(f"{differing - near} glyph cells differ away from any threshold")
            else:
                if not bucket_digits_ok(norms_all[w0:w0 + n], got.reshape(-1)):
                    out.append("a bucket digit differs where the half sums do not tie")
            if shifted:
                bad = explain_check(desc, ref, got, w0)
                if bad:
                    out.append(f"{len(bad)} differing windows read no ambiguous NCO multiplier, first {bad[:5]}")
            elif epi in (0, 3) and not np.array_equal(payload, ref.view(np.uint8).reshape(-1)):
                out.append("differs from the oracle, and the chain has no shift stage")
            return out

        exact = not shifted and epi in (0, 3)
        return ref, (None if exact else rule), (1 if epi in (1, 2) else 4)
    return expect


# ------------------------------------------------------------------ the fold sinks' footprint (tests/test_gpu_fold_footprint.py)
#
# A fold (qd_plan_summarize, _pool, _mean, _power, _spread, _density, _bands, _picture) leaves SEVERAL output planes.  Each sits in a
# framed_out allocation of its own, and everything is byte for byte: the planes' expected bytes are the CPU twins' over the plan's norms.
# The payload pre-fill is the run's own: 0xA5 in the first run and 0x5A in the second.  As f32 / f64 the 0xA5 pattern is negative and as
# u32 above the 2^31 count limit, so no fold ever writes it; in a u8 plane (pick_rows, pixels, the summary struct's bytes) either byte
# is a value a fold may write, and an unwritten element shows in the run whose pre-fill the expected byte is not.

FOLD_FILLS = (GUARD_BYTE, 0x5A)                # the output pre-fill of run 0 / run 1


def fold_guard_bytes(row_bytes):
    """the least size of a fold plane's guard: max(64 KiB, four output rows), a multiple of 4 KiB.  A condition, not a measurement."""
    return _round_up(max(64 << 10, 4 * int(row_bytes)), 4096)


def fold_plane(kind, row_bytes, payload_bytes, fill=GUARD_BYTE, skew=0, engine=None):
    """one output plane of a fold between guards of fold_guard_bytes(row_bytes) + skew bytes: skew (a multiple of the element size that
    is no multiple of 16) moves the payload off the allocation's own alignment"""
    return framed_out(kind, fold_guard_bytes(row_bytes) + int(skew), int(payload_bytes), engine, fill)


class FoldRun:
    """what one framed fold run left behind: per plane name its FootprintRun (guards and payload) and the bytes of an output row, the
    run's pre-fill byte, and the source buffer's bytes where a kernel could write it (device, pinned)"""

    def __init__(self, planes, row_bytes, fill=GUARD_BYTE, src=None):
        self.fill = int(fill)
        self.row_bytes = {name: int(b) for name, b in row_bytes.items()}
        self.planes = {name: FootprintRun(out) for name, out in planes.items()}
        self.src_uploaded = self.src_now = None
        if src is not None and src.kind != "host":
            self.src_uploaded, self.src_now = src.uploaded, src.snapshot()


def fold_footprint_violations(runs, refs):
    """The footprint checker of the fold sinks.  runs: the FoldRun of each poison pattern (two; run k pre-filled with FOLD_FILLS[k]),
    same windows, same true slab.  refs: plane name -> the expected bytes (an array laid out like the payload; its dtype gives the
    element size).  Byte for byte.  Returns the violated conditions, each naming its plane; every wrong payload byte falls into exactly
    one of the first three classes:
      1. "unwritten": an output element still holds its run's pre-fill where the expected value is something else;
      2. "poison": the runs' payloads differ elsewhere (memory outside the slab, or a stale workspace, reached an output byte);
      3. "oracle": a byte on which the runs agree is not the expected one;
      4. "guard": a byte of a plane's guard changed, or a guard is smaller than fold_guard_bytes (64 KiB, four output rows);
      5. "source": a byte of the source buffer (frames or slab) changed."""
    bad = []
    if len(runs) != len(POISON_WORDS):
        bad.append(f"poison: {len(runs)} runs, one per pattern is {len(POISON_WORDS)}")
    for name, ref in refs.items():
        ref = np.ascontiguousarray(ref)
        unit = ref.dtype.itemsize
        ref_b = ref.view(np.uint8).reshape(-1)
        rs = [r.planes.get(name) for r in runs]
        if any(r is None for r in rs):
            bad.append(f"oracle: plane {name}: a run left no such plane")
            continue
        if unit == 1 and len({r.fill for r in runs}) < 2:
            bad.append(f"unwritten: plane {name}: a u8 plane needs a run with each pre-fill of {FOLD_FILLS}")
        sizes = [r.payload.size for r in rs]
        if any(s != ref_b.size for s in sizes):
            bad.append(f"oracle: plane {name}: payloads of {sizes} bytes, the expected plane has {ref_b.size}")
            continue
        stale = np.zeros(ref_b.size // unit, dtype=bool)
        for run, r in zip(runs, rs):
            fill = np.full(unit, run.fill, dtype=np.uint8)
            held = (r.payload.reshape(-1, unit) == fill).all(axis=1)
            stale |= held & ~(ref_b.reshape(-1, unit) == fill).all(axis=1)
        if stale.any():
            bad.append(f"unwritten: plane {name}: {int(stale.sum())} output elements still hold the pre-fill, first element {int(np.flatnonzero(stale)[0])}")
        live = ~np.repeat(stale, unit)
        apart = np.zeros(ref_b.size, dtype=bool)
        for r in rs[1:]:
            apart |= r.payload != rs[0].payload
        apart &= live
        if apart.any():
            bad.append(f"poison: plane {name}: payloads of the two fills differ in {int(apart.sum())} bytes, first at byte {int(np.flatnonzero(apart)[0])}")
        off = np.zeros(ref_b.size, dtype=bool)
        for r in rs:
            off |= r.payload != ref_b
        off &= live & ~apart
        if off.any():
            bad.append(f"oracle: plane {name}: {int(off.sum())} bytes differ from the expected plane, first at byte {int(np.flatnonzero(off)[0])}")
        for k, (run, r) in enumerate(zip(runs, rs)):
            need = fold_guard_bytes(run.row_bytes.get(name, 0))
            if min(r.front.size, r.back.size) < need:
                bad.append(f"guard: plane {name}: fill {k}: guards of {r.front.size} / {r.back.size} bytes, the condition is {need}")
            for side, g in (("front", r.front), ("back", r.back)):
                d = np.flatnonzero(g != run.fill)
                if d.size:
                    where = int(d[0]) if side == "back" else int(d[-1]) - g.size
                    bad.append(f"guard: plane {name}: fill {k}: {d.size} bytes of the {side} guard were written, nearest at {where:+d} bytes from the payload")
    for k, run in enumerate(runs):
        if run.src_now is not None and not np.array_equal(run.src_now, run.src_uploaded):
            d = np.flatnonzero(run.src_now != run.src_uploaded)
            bad.append(f"source: fill {k}: {d.size} bytes of the source buffer changed, first at byte {int(d[0])}")
    return bad


# ------------------------------------------------------------------ value-domain streams (tests/test_gpu_values.py)
#
# Streams chosen for their VALUES, not their shape: every sample code of an integer format at every load position
# (code_stream), power-of-two scaled cf32 (exact while nothing leaves the normal range: slow_bins says which bins the |X| range
# switch of qd_device.h norm_fast hands to the IEEE form), and runs of exact zeros (zero_runs).  Finite normal-range values and
# exact zeros only.  tests/test_value_streams_cpu.py holds the builders to their conditions on the oracle alone.

SLOW_LO, SLOW_HI = 2.0 ** -96, 2.0 ** 96       # norm_fast keeps s = x^2 + y^2 in [2^-96, 2^96); everything else is norm_ieee's
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def code_count(fmt):
    return {1: 256, 2: 256, 3: 65536}[fmt]


def cs8_grades():
    """the 256 cs8 codes (as bytes) in 8 grades by the binade of |value|: {0}, {+-1}, {+-2, +-3}, ... {+-64 ... +-127, -128}.
    All values of a grade but the last share one ulp, so a one-ulp error on any of them is not absorbed by its neighbours."""
    v = np.arange(-128, 128)
    grade = np.where(v == 0, 0, np.minimum(np.floor(np.log2(np.maximum(np.abs(v), 1))).astype(int) + 1, 7))
    return [v[grade == g].astype(np.int8).view(np.uint8) for g in range(8)]


CS16_COMB = sorted(set(range(0, 65536, 127)) | {0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF})
"""cs16 codes that code_stream repeats behind the first 4 * 65536 samples: the edge codes and every 127th.  A cs16 sample is
-32767.5 + h / 65535, so a one-ulp error (2^-9) on ONE sample moves a FIR output of magnitude ~32767 by tap * 2^-9, less than
its ulp: it shows only as a flipped rounding, with a chance of about |tap| / 2 per output.  With the 4 occurrences per
component that 65536 codes leave room for, a lowpass (/4, 40 taps) + W = 32 misses such an error for 52 % of the codes (12 %
at /1); with the ~70 further occurrences of a 3e5-sample stream's tail it misses 3 of the comb's 1046 (code, component)
pairs at /4 and none at /1, the control's chain (tests/test_value_streams_cpu.py).  Without a lowpass the FFT's first
differences are exact and every occurrence shows."""


def code_stream(fmt, n, seed):
    """n samples of integer format fmt (cs8 1 / cu8 2 / cs16 3) as a uint8 array, holding EVERY code of the format in the I and
    in the Q component at every byte offset modulo 16 of the stream (sample index modulo 8 for the 8-bit formats, modulo 4 for
    cs16).  By construction, not by chance: the slots of one component at one offset are filled with whole random permutations
    of the codes, the first permutation first.  cs8 comes in 8 magnitude-graded segments of n // 8 samples (cs8_grades): each
    segment holds its grade's codes only, small codes among small codes, so a window inside a segment sums values of one
    binade.  cu8 and cs16 values all sit near -127 / -32767.5 (src/lib.rs:246-255) and need no grading; cs16 needs
    n >= 4 * 65536 for one occurrence per offset, and the samples behind those repeat the codes of CS16_COMB."""
    rng = np.random.default_rng(seed)
    phases = 8 if fmt in (1, 2) else 4
    codes = np.zeros((n, 2), dtype=np.uint8 if fmt in (1, 2) else "<u2")
    if fmt == 1:
        seg = n // 8
        parts = [(g * seg, n if g == 7 else (g + 1) * seg, gc) for g, gc in enumerate(cs8_grades())]
    elif fmt == 2:
        parts = [(0, n, np.arange(256, dtype=np.uint8))]
    else:
        assert n >= 4 * 65536, n
        parts = [(0, 4 * 65536, np.arange(65536).astype("<u2")), (4 * 65536, n, np.array(CS16_COMB, dtype="<u2"))]
    for a, b, gc in parts:
        for comp in range(2):
            for ph in range(phases):
                slots = np.arange(a + (ph - a) % phases, b, phases)
                reps = -(-slots.size // gc.size)
                codes[slots, comp] = rng.permuted(np.tile(gc, (reps, 1)), axis=1).reshape(-1)[:slots.size]
    return codes.view(np.uint8).reshape(-1)


def stream_codes(fmt, data):
    """(n, 2) integer codes (the raw bytes / little-endian halfwords) of an integer-format stream"""
    return np.ascontiguousarray(data).view(np.uint8).view(np.uint8 if fmt in (1, 2) else "<u2").reshape(-1, 2).astype(np.int64)


def code_coverage(fmt, data, first, count):
    """occurrences[component, load position, code] inside samples [first, first + count) of the stream: load position = the
    sample's byte offset modulo 16 in units of one sample (index modulo 8 / modulo 4)"""
    phases = 8 if fmt in (1, 2) else 4
    c = stream_codes(fmt, data)[first:first + count]
    ph = (np.arange(first, first + c.shape[0]) % phases).astype(np.int64)
    nc = code_count(fmt)
    return np.stack([np.bincount(ph * nc + c[:, comp], minlength=phases * nc).reshape(phases, nc) for comp in range(2)])


def perturb_code(fmt, data, unpacked, code, comp, sign=1):
    """`unpacked` (oracle.unpack of `data`) with every occurrence of `code` in component comp moved by one ulp (nextafter towards
    sign * inf); cs8 code 0 unpacks to 0.0, which no ulp moves, and becomes sign * 2^-24 instead, a wrong quotient of plausible
    size.  Returns (the perturbed copy, the sample indices changed)."""
    at = np.flatnonzero(stream_codes(fmt, data)[:, comp] == code)
    x = unpacked.copy()
    v = x[at, comp]
    x[at, comp] = np.where(v == 0, np.float32(sign * 2.0 ** -24), np.nextafter(v, np.float32(sign * np.inf)))
    assert (x[at, comp] != v).all()
    return x, at


def source_block(stages, W, S, w0, n=1):
    """[lo, hi): the source samples the reference fetches for sink windows [w0, w0 + n): window w reads [w S, w S + W) of the
    last stage, and a lowpass (D, T) serves outputs [a, b) with one block read [a D, b D + T) of its input (src/filter.rs:68-71)"""
    lo, hi = w0 * S, (w0 + n - 1) * S + W
    for kind, arg in reversed(list(stages)):
        if kind == "lowpass":
            lo, hi = lo * int(arg[1]), hi * int(arg[1]) + int(arg[2])
    return lo, hi


def windows_reading(stages, W, S, samples, n_windows):
    """the sorted sink windows < n_windows whose source_block holds one of `samples`"""
    step = source_block(stages, W, S, 1)[0]
    span = source_block(stages, W, S, 0)[1]
    out = set()
    for s in np.unique(np.asarray(samples, dtype=np.int64)):
        out.update(range(max(0, -(-(int(s) - span + 1) // step)), min(n_windows, int(s) // step + 1)))
    return sorted(out)


def contiguous_runs(ws):
    """[(first, count), ...] of a sorted list of integers"""
    runs = []
    for w in ws:
        if runs and runs[-1][0] + runs[-1][1] == w:
            runs[-1][1] += 1
        else:
            runs.append([w, 1])
    return [tuple(r) for r in runs]


def slow_bins(norms):
    """bins of reference norms whose x^2 + y^2 lies outside [2^-96, 2^96): norm_fast (qd_device.h) hands exactly those to the IEEE
    form for their range (zeros included).  Judged on the norm: norm^2 is x^2 + y^2 to 2^-23, so bins within that of a limit
    are counted as neither (returned as the second array)."""
    s = np.asarray(norms, dtype=np.float64) ** 2
    edge = (np.abs(s / SLOW_LO - 1) < 2.0 ** -20) | (np.abs(s / SLOW_HI - 1) < 2.0 ** -20)
    return ((s < SLOW_LO) | (s >= SLOW_HI)) & ~edge, edge


def normal_or_zero(a):
    """every element finite and either 0 or of normal-range magnitude (no subnormal)"""
    a = np.abs(np.asarray(a, dtype=np.float32))
    return bool((np.isfinite(a) & ((a == 0) | (a >= np.float32(F32_MIN_NORMAL)))).all())


def zero_runs(x, long_run, window_span, seed):
    """a copy of the cf32 stream x (n, 2) with runs of exact zeros: ONE run of long_run samples from n // 3 on, in four quarters
    (+0, +0), (-0, +0), (+0, -0), (-0, -0); and short runs of window_span // 3 + 1 samples every 2.5 window spans outside it,
    which therefore start and end inside a window: in turn both components, I only, Q only, signs alternating.  Returns
    (stream, mask of the samples with a zero component).  Through _to_format the zeros become cs8 code 0."""
    rng = np.random.default_rng(seed)
    n = x.shape[0]
    x = x.copy()
    pz, nz = np.float32(0.0), np.float32(-0.0)
    a = n // 3
    assert long_run > 0 and a + long_run + 3 * window_span < n, (n, long_run, window_span)
    q = -(-long_run // 4)
    for k, (si, sq) in enumerate(((pz, pz), (nz, pz), (pz, nz), (nz, nz))):
        lo, hi = a + k * q, min(a + (k + 1) * q, a + long_run)
        x[lo:hi, 0], x[lo:hi, 1] = si, sq
    short = window_span // 3 + 1
    step = (5 * window_span) // 2 + int(rng.integers(1, 8))
    k = 0
    for s in list(range(window_span // 2, a - window_span - short, step)) + list(range(a + long_run + window_span, n - short, step)):
        z = nz if k % 2 else pz
        if k % 3 != 2:
            x[s:s + short, 0] = z
        if k % 3 != 1:
            x[s:s + short, 1] = z
        k += 1
    return x, (x[:, 0] == 0) | (x[:, 1] == 0)


def mixed_scale(norms, side=1):
    """(k, windows): the power of two (k > 0 with side = 1, k < 0 with side = -1) that puts slow and fast bins (slow_bins) inside
    the same window in the most windows of the reference norms `norms` (n_windows, W), and that count.  Chosen from the
    reference alone."""
    base = np.asarray(norms, dtype=np.float64)
    best = (side * 48, -1)
    for k in range(30, 70):
        slow, edge = slow_bins(base * 2.0 ** (side * k))
        both = int((slow.any(axis=1) & (~slow & ~edge).any(axis=1)).sum())
        if both > best[1]:
            best = (side * k, both)
    return best


# ------------------------------------------------------------------ the bucket sink's half-sum order (test_bucket_order_cpu.py)
#
# freq_levels reduces a window to first < second ? 0 : 1 with two sequential f32 sums of |X| over the natural bins 0 ... W/2-1 and
# W/2 ... W-1 (src/fft.rs:95-97).  On a real-valued stream |X[k]| = |X[W-k]|: `second` is `first`'s multiset with |X[W/2]| in place
# of |X[0]|, summed in the opposite order.  Where the window's odd-indexed samples sum to zero, X[0] and X[W/2] agree up to the
# FFT's own rounding, and only the summation order and the tie rule decide the digit.  The builders below make such windows.

SUM_ORDERS = ("sequential", "pairwise", "f64", "reversed", "shifted_halves")


def _oracle_chain(oracle, data, fmt, sr, stages):
    ch = oracle.Chain.from_bytes(data, fmt, sr)
    for kind, arg in stages:
        ch = ch.shift(arg) if kind == "shift" else ch.lowpass(*arg)
    return ch


def balanced_geometry(stages, W, S):
    """(span, step, q) of a list of lowpass triples, composed source to sink: the source samples one window reads
    ((W D2 + T2) D1 + T1), the source samples between window starts (S D1 D2), and q = ceil(span / step): windows 0, q, 2q, ...
    read disjoint source spans."""
    span, step = int(W), int(S)
    for _, D, T in reversed(list(stages)):
        span, step = span * int(D) + int(T), step * int(D)
    return span, step, -(-span // step)


def balanced_real_stream(oracle, stages, W, S, n_balanced, seed, sr):
    """A cf32 stream with zero imaginary part (real part ~ 0.25 N(0, 1)) in which windows 0, q, 2q, ... (n_balanced of them) of the
    chain  lowpass* | width W stride S  have odd-indexed samples that sum to zero up to f32 rounding.  `stages`: lowpass triples
    (frequency, decimate, size), possibly none; no shift.  Each balanced window owns one source sample n0 at an odd offset near
    the middle of its span; the chain is linear, so with L the f64 sum of the window's odd outputs (oracle read_at: what the sink
    reads, tail truncation included) and G the same sum for a unit impulse at n0, x[n0] - L / G balances the window.  Only the
    oracle computes here.  Returns (x float32 (n, 2), the balanced windows' indices)."""
    stages = [tuple(int(v) for v in lp) for lp in stages]
    span, step, q = balanced_geometry(stages, W, S)
    balanced = np.arange(n_balanced, dtype=np.int64) * q
    n = (int(balanced[-1]) + 3) * step + span + step
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 2), dtype=np.float32)
    x[:, 0] = (0.25 * rng.standard_normal(n)).astype(np.float32)
    lps = [("lowpass", lp) for lp in stages]
    # the offset of n0 in its span: odd, near the middle, and the phase (of the 2 prod(D) a pair of outputs spans) at which a unit
    # impulse reaches the window's odd outputs with the largest gain |G|; found on window 0 of a probe stream
    period = 2 * (step // int(S))
    cands = [((span // 2) | 1) + 2 * j for j in range(period // 2) if ((span // 2) | 1) + 2 * j < span]
    probe = np.zeros((span + step, 2), dtype=np.float32)
    gains = []
    for c in cands:
        probe[c, 0] = 1.0
        ng, g = _oracle_chain(oracle, probe, 0, sr, lps).read_at(0, W)
        assert ng == W, (c, ng)
        gains.append(abs(float(g[1::2, 0].astype(np.float64).sum())))
        probe[c, 0] = 0.0
    off = cands[int(np.argmax(gains))]
    n0 = balanced * step + off
    e = np.zeros((n, 2), dtype=np.float32)
    e[n0, 0] = 1.0
    cx, ce = _oracle_chain(oracle, x, 0, sr, lps), _oracle_chain(oracle, e, 0, sr, lps)
    for w, at in zip(balanced, n0):
        (ny, y), (ng, g) = cx.read_at(int(w) * S, W), ce.read_at(int(w) * S, W)
        assert ny == W and ng == W, (int(w), ny, ng)
        L = float(y[1::2, 0].astype(np.float64).sum())
        G = float(g[1::2, 0].astype(np.float64).sum())
        assert abs(G) >= 0.999 * max(gains) > 0.0, (int(w), G, max(gains))      # every balanced window sees the probe's gain
        x[at, 0] = np.float32(float(x[at, 0]) - L / G)
    return x, balanced


def balanced_cs8_stream(n, seed):
    """cs8 codes (n, 2) int8, n a multiple of 4, with x[4m+1] = a_m, x[4m+3] = -a_m and imaginary codes 0: cs8 unpacks as
    code / 127 (odd-symmetric, 0 -> 0), so every window of 4k samples that starts at an even sample is balanced exactly."""
    assert n % 4 == 0
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 2), dtype=np.int8)
    x[0::2, 0] = rng.integers(-128, 128, n // 2)
    a = rng.integers(-127, 128, n // 4)
    x[1::4, 0], x[3::4, 0] = a, -a
    return x


def _half_sums(half, order):
    """f32 (f64 for "f64") sums of the rows of `half` (n, m) in the given order"""
    if half.shape[1] == 0:
        return np.zeros(half.shape[0], np.float64 if order == "f64" else np.float32)
    if order == "f64":
        return half.astype(np.float64).sum(axis=1)
    if order == "reversed":
        half = half[:, ::-1]
    if order == "pairwise":
        h = half.astype(np.float32)
        while h.shape[1] > 1:
            h = h[:, 0::2] + h[:, 1::2]                     # float32 + float32: one rounding per node of the tree
        return h[:, 0]
    return np.cumsum(half, axis=1, dtype=np.float32)[:, -1]


def digits_from_norms(norms, order):
    """freq_levels digits from the oracle's sparkfft norms (n_windows, W) (the rows' fftshift undone, as in bucket_digits_ok),
    with the two half sums formed in `order`:
      "sequential"      ascending over the natural bins, f32 (src/fft.rs:95-97; what the engine must do)
      "pairwise"        a balanced f32 tree over adjacent bins (a wave reduction)
      "f64"             f64 sums, compared in f64
      "reversed"        descending over the natural bins, f32
      "shifted_halves"  sequential over the halves of the fftshifted row: the two sums change places
    first < second gives 0, anything else (a tie included) 1."""
    assert order in SUM_ORDERS, order
    norms = np.asarray(norms, dtype=np.float32)
    W = norms.shape[1]
    nat = norms if order == "shifted_halves" else np.roll(norms, W // 2, axis=1)
    first, second = _half_sums(nat[:, : W // 2], order), _half_sums(nat[:, W // 2:], order)
    return np.where(first < second, 0, 1).astype(np.uint8)


def exact_ties(norms):
    """windows of the oracle's sparkfft norms whose two sequential f32 half sums are equal"""
    norms = np.asarray(norms, dtype=np.float32)
    W = norms.shape[1]
    nat = np.roll(norms, W // 2, axis=1)
    return _half_sums(nat[:, : W // 2], "sequential") == _half_sums(nat[:, W // 2:], "sequential")


class BucketOrderCase:
    """one chain of test_gpu_bucket_order.py / test_bucket_order_cpu.py: the balanced stream it runs on and the plan it must come
    out as.  shift: None, or 0 — a `shift 0` stage multiplies by exactly (1, 0), so the stream stays real and the chain exact; it is
    how the built-in kernels of the shapes that exist only with a shift stage are reached.  policy: "auto" / "generic" /
    "specialise" / "builtin" (QD_KERNEL_NO_PLAN_TIME: the built-in kernel whatever the code-object cache holds); family(info, kernel name) says whether the plan is the intended kernel."""

    def __init__(self, name, stages, W, S, n_balanced, family, fmt=0, sr=21_000_000, shift=None, policy="auto", tile_hint=None, paths=False,
                 seed=20261018):
        self.name, self.stages, self.W, self.S, self.n_balanced, self.family = name, [tuple(lp) for lp in stages], W, S, n_balanced, family
        self.fmt, self.sr, self.shift, self.policy, self.tile_hint, self.paths, self.seed = fmt, sr, shift, policy, tile_hint, paths, seed

    def __repr__(self):
        return self.name

    def stream_key(self):
        return (self.fmt, self.sr, tuple(self.stages), self.W, self.S, self.n_balanced, self.seed)

    def chain_stages(self):
        return ([("shift", self.shift)] if self.shift is not None else []) + [("lowpass", lp) for lp in self.stages]


_BUCKET_STREAMS = {}


def bucket_order_stream(oracle, case):
    """(the stream's bytes as a uint8 array, the balanced windows' indices) of a BucketOrderCase; built once per stream_key"""
    key = case.stream_key()
    if key not in _BUCKET_STREAMS:
        if case.fmt == 0:
            x, bal = balanced_real_stream(oracle, case.stages, case.W, case.S, case.n_balanced, case.seed, case.sr)
        else:
            assert case.fmt == 1 and not case.stages and case.W % 4 == 0 and case.S % 2 == 0, case
            x = balanced_cs8_stream((case.n_balanced + 1) * case.S + case.W, case.seed)
            bal = np.arange(case.n_balanced, dtype=np.int64)
        raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        raw.setflags(write=False)
        _BUCKET_STREAMS[key] = (raw, bal)
    return _BUCKET_STREAMS[key]


def _fam(kind=None, kernel=None, flags=0, no_flags=0, eq_flags=None, part=None, threads=None):
    def ok(info, name):
        return ((threads is None or int(info.threads) == threads) and (kind is None or int(info.kernel_kind) == kind) and (kernel is None or name.startswith(f"qd::{kernel}<"))
                and (int(info.kernel_flags) & flags) == flags and not (int(info.kernel_flags) & no_flags)
                and (eq_flags is None or int(info.kernel_flags) == eq_flags) and (part is None or part in name))
    return ok


_CFG2, _CFG3P, _CFG3, _CFG4, _D12 = (2_000_000, 16, 40), (200_000, 32, 200), (200_000, 32, 400), (5_000_000, 8, 512), (1_500_000, 12, 48)
_CASC = [(200_000, 4, 40), (30_000, 4, 64)]
_SPARK, _SPARK2, _SPARK0 = 524288, 1048576, 2097152
_GENERIC = _fam(kind=0, part="DynGeo")

# Every place that forms the bucket digit, on the smallest shape that selects it ("the order contract").
BUCKET_ORDER_CASES = [
    # built-in FixedGeo kernels.  cfg2, cfg3' and the 64 / 16 FSK chain are built in with a shift stage only: `shift 0` reaches them
    BucketOrderCase("builtin-cfg2", [_CFG2], 128, 128, 100, _fam(kind=1, kernel="k_chain", eq_flags=65800), shift=0, policy="builtin"),
    BucketOrderCase("builtin-cfg3p-deferred-fft", [_CFG3P], 128, 128, 100, _fam(kind=1, kernel="k_chain", eq_flags=65868), shift=0, paths=True, policy="builtin"),
    BucketOrderCase("builtin-cfg4", [_CFG4], 1024, 1024, 40, _fam(kind=1, kernel="k_chain", eq_flags=8392), sr=100_000_000, policy="builtin"),
    BucketOrderCase("builtin-cfg3-streaming", [_CFG3], 64, 16, 100, _fam(kind=1, kernel="k_chain_pipe3s", eq_flags=164128), shift=0, policy="builtin"),
    # the streaming three-stage kernel as the plan-time build of the same shape without a shift stage
    BucketOrderCase("cfg3-streaming", [_CFG3], 64, 16, 100, _fam(kind=2, kernel="k_chain_pipe3s", flags=32768 | 131072), policy="specialise"),
    # policies: runtime geometry (k_chain phase 4) and plan-time builds; a shape without a built-in kernel
    BucketOrderCase("cfg2-generic", [_CFG2], 128, 128, 100, _GENERIC, policy="generic"),
    BucketOrderCase("cfg2-specialise", [_CFG2], 128, 128, 100, _fam(kind=2, kernel="k_chain"), policy="specialise"),
    BucketOrderCase("cfg3p-generic", [_CFG3P], 128, 128, 100, _GENERIC, policy="generic"),
    BucketOrderCase("cfg3p-specialise", [_CFG3P], 128, 128, 100, _fam(kind=2, kernel="k_chain", flags=4 | 64), policy="specialise"),
    BucketOrderCase("d12-specialise", [_D12], 256, 256, 100, _fam(kind=2, kernel="k_chain"), policy="specialise"),
    # wave-local kernels without a lowpass: the built-in runtime-width k_spark, its plan-time builds (the lean path from W = 8), k_spark2
    BucketOrderCase("spark-w8", [], 8, 8, 300, _fam(kind=1, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="builtin"),
    BucketOrderCase("spark-w16", [], 16, 16, 300, _fam(kind=1, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="builtin"),
    BucketOrderCase("spark-w64", [], 64, 64, 300, _fam(kind=1, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="builtin"),
    BucketOrderCase("spark-w128", [], 128, 128, 300, _fam(kind=1, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="builtin"),
    BucketOrderCase("spark-w1024", [], 1024, 1024, 100, _fam(kind=1, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="builtin"),
    BucketOrderCase("spark-w8-lean", [], 8, 8, 300, _fam(kind=2, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="specialise"),
    BucketOrderCase("spark-w16-lean", [], 16, 16, 300, _fam(kind=2, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="specialise"),
    BucketOrderCase("spark-w64-lean", [], 64, 64, 300, _fam(kind=2, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), policy="specialise"),
    BucketOrderCase("spark2-w128", [], 128, 128, 300, _fam(kind=2, kernel="k_spark2", flags=_SPARK | _SPARK2), policy="specialise"),
    BucketOrderCase("spark2-w1024", [], 1024, 1024, 100, _fam(kind=2, kernel="k_spark2", flags=_SPARK | _SPARK2), policy="specialise"),
    BucketOrderCase("spark-cs8-w128", [], 128, 128, 300, _fam(kind=1, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0), fmt=1, policy="builtin"),
    BucketOrderCase("spark2-cs8-w128", [], 128, 128, 300, _fam(kind=2, kernel="k_spark2", flags=_SPARK | _SPARK2), fmt=1, policy="specialise"),
    # overlapping windows without a lowpass: a window per lane (k_spark0); k_spark2 built for the stride; W = 64 / S = 16, which the
    # interleaved launches serve for the norms and glyph sinks only (chain_candidates): the bucket sink runs it on the chain kernel
    BucketOrderCase("spark0-w4-s2", [], 4, 2, 300, _fam(kind=2, kernel="k_spark0", flags=_SPARK | _SPARK0), policy="specialise"),
    BucketOrderCase("spark0-w8-s2", [], 8, 2, 300, _fam(kind=2, kernel="k_spark0", flags=_SPARK | _SPARK0), policy="specialise"),
    BucketOrderCase("spark2-w128-s32", [], 128, 32, 300, _fam(kind=2, kernel="k_spark2", flags=_SPARK | _SPARK2), policy="specialise"),
    BucketOrderCase("overlap-w64-s16-specialise", [], 64, 16, 300, _fam(kind=2, kernel="k_chain", no_flags=_SPARK), policy="specialise", paths=True),
    BucketOrderCase("overlap-w64-s16-generic", [], 64, 16, 300, _GENERIC, policy="generic"),
    # the cascade kernel (lane 0 sums) and the two-stage plan (a window past the LDS tile: the sink is its second stage's)
    BucketOrderCase("cascade-w16-s8", _CASC, 16, 8, 200, _fam(part="qd::k_cascade<0>"), sr=2_000_000),
    BucketOrderCase("cascade-w128", _CASC, 128, 128, 100, _fam(part="qd::k_cascade<0>"), sr=2_000_000),
    BucketOrderCase("two-stage-w1024", [_CFG3P], 1024, 1024, 40, _fam(part="two stages:"), seed=20261019),      # (the table's seed: no exact tie in 40 windows)
]


# ------------------------------------------------------------------ planted-value streams (test_planted_streams_cpu.py, test_gpu_planted.py)
#
# A cf32 window whose first sample is (a, 0) and whose other samples are +0 has the norm |a| in every bin, bit for bit (the transform adds
# and multiplies zeros only).  A stream of such windows lets a test choose the f32 pattern that every bin's cell of a fold receives, window
# by window; a "cell case" is a run of `depth` consecutive windows folded with pool = depth, so every bin of output row c holds case c.

PLANT_NAN, PLANT_INF, PLANT_MAX = 0x7FC00000, 0x7F800000, 0x7F7FFFFF
PLANTED_WIDTHS = (1, 4, 128, 256, 2048)          # where pool_geometry / power_geometry change V, lanes per window, pieces per workgroup, slabs
PLANTED_DEPTHS = (4, 16, 64, 4096)               # pool == depth; 4096 at W <= 4 only
PLANTED_CAP = 32 << 20                           # bytes a planted stream stays below (its norms are half of it)
PLANTED_SMALL_CHUNK = 1 << 16                    # chunk_bytes of the second plan
PLANTED_SR = 21_000_000


def impulse_stream(bits, W):
    """The cf32 bytes of len(bits) + 1 windows of W samples: window i is ((f32 of bits[i]), 0) followed by +0 samples, so that its norms
    are that pattern in all W bins; the trailing window is zeros (the sink's loop is `while i < len - W`).  A NaN pattern plants a NaN
    window (every bin NaN).  Signs are not planted: a norm is never negative, so what the folds do with a sign bit (or with a NaN's
    payload) stays a matter of the CPU twins' tests."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    assert ((bits <= PLANT_INF) | (bits == PLANT_NAN)).all(), "an impulse plants non-negative values, +inf and the quiet NaN only"
    x = np.zeros((bits.size + 1, int(W), 2), dtype=np.uint32)
    x[:-1, 0, 0] = bits
    return x.tobytes()


def cases_stream(cases, depth, W):
    """(bytes, uint32[len(cases), depth]) of the impulse stream whose windows [c depth, (c + 1) depth) hold the values of cases[c] followed
    by NaN windows (a NaN adds nothing to any fold)"""
    m = np.full((len(cases), int(depth)), PLANT_NAN, dtype=np.uint32)
    for c, vals in enumerate(cases):
        assert len(vals) <= depth
        m[c, :len(vals)] = vals
    return impulse_stream(m, W), m


def plantable(cell):
    """whether an impulse stream can hold the cell: no sign bit and no NaN other than the quiet one"""
    return all(b <= PLANT_INF or b == PLANT_NAN for b in cell)


def exponent_sweep():
    """for every biased exponent e = 0 ... 254 the cells [e<<23 | 1], [e<<23 | 0x7FFFFF] * 3 and a pair one exponent apart — an addend in
    every limb at every shift s & 31 (2 s & 31 for the squares), pairs that straddle a limb boundary included — and cells that mix the
    exponents 0 / 1 with 254: bits in the first and in the last limb of one cell"""
    cells = []
    for e in range(255):
        lo, hi = (e << 23) | 1, (e << 23) | 0x7FFFFF
        cells += [[lo], [hi] * 3, [hi, (min(e + 1, 254) << 23) | 1]]
    top = 254 << 23
    cells += [[1, top | 1], [0x7FFFFF, top | 0x7FFFFF, 1], [(1 << 23) | 1, top | 0x7FFFFF], [top | 0x7FFFFF, 1, (1 << 23) | 0x7FFFFF, 3]]
    return cells


def bucket_sweep():
    """for every bucket k = 0 ... 2040 of the summary's scale (bits >> 20) its two ends k << 20 and (k << 20) | 0xFFFFF; bucket 2040 holds
    +inf alone.  uint32[4081], ascending"""
    k = np.arange(2040, dtype=np.uint32) << 20
    return np.concatenate([np.stack([k, k | np.uint32(0xFFFFF)], axis=1).reshape(-1), np.array([PLANT_INF], np.uint32)])


_PLANTED = {}


def planted_cells():
    """(discriminating, rest): the cell cases of the GPU's planted streams.  `discriminating` are the planted rounding cases of the three
    CPU fold tests, in their order (power's, its ties, the mean's, the spread's); `rest` is exponent_sweep() and the random cells of the
    CPU generators (2000 of test_power_cpu's, 400 of test_spread_cpu's, their seeds).  Left out, because an impulse cannot plant a sign bit
    or a NaN payload: the mean's [nan, -nan, nan], [-0.0], [-1.0, 1.0]; the power's [nan, -nan], [-0.0], [-1.0, 1.0]; the spread's
    [-0.0, 0], [-1, 1, -2], [nan, 1, 0xFFC00001, 2], [-inf], [nan, -nan] (0x80000000, 0xBF800000, 0xC0000000, 0xFF800000, 0xFFC00000,
    0xFFC00001).  The all-NaN group stays: the spread's empty cell is NaN windows only."""
    if "cells" not in _PLANTED:
        import test_mean_cpu as M
        import test_power_cpu as P
        import test_spread_cpu as S
        first = P.PLANTED_CASES + P.PLANTED_TIES + [c[0] for c in M.PLANTED_CASES] + S.PLANTED_CASES + S.PLANTED_EQUAL + S.PLANTED_OTHERS
        first = [list(c) for c in first if plantable(c)]
        rest = exponent_sweep() + P.random_cells(2000) + S.random_cells(400)
        assert all(plantable(c) for c in rest)
        _PLANTED["cells"] = (first, rest)
    return _PLANTED["cells"]


def planted_depths(W):
    return [d for d in PLANTED_DEPTHS if d <= 64 or W <= 4]


def planted_case_set(W, depth):
    """The cells of the stream (W, depth), as many as PLANTED_CAP holds: every discriminating cell of at most `depth` values first, then
    the other cells whose smallest depth this is, then those that a smaller depth holds too; where one of the two groups has to be cut,
    its members are taken at even distances (the sweep keeps its span of exponents)."""
    key = (W, depth)
    if key not in _PLANTED:
        first, rest = planted_cells()
        below = max([d for d in PLANTED_DEPTHS if d < depth] + [0])
        room = (PLANTED_CAP // (8 * W) - 1) // depth
        cells = [c for c in first if len(c) <= depth][:room]
        for group in ([c for c in rest if below < len(c) <= depth], [c for c in rest if len(c) <= below]):
            m = min(len(group), room - len(cells))
            cells += [group[i * len(group) // m] for i in range(m)]
        _PLANTED[key] = cells
    return _PLANTED[key]


def planted_small_batch(W):
    """windows in a batch of a host-source fold of a cf32 plan of width W = stride with chunk_bytes = PLANTED_SMALL_CHUNK: quadrs_hip.hip,
    Fold::host gives walk_host bytes_per_window = max(S D 8, W 4) = 8 W, and chunk_windows divides chunk_bytes by it (a whole number of
    the kernel's tiles of `tile_windows`, which the GPU tests check divides it)"""
    return PLANTED_SMALL_CHUNK // (8 * W)


PLANTED_GRIDS = [(0, 256), (1000, 64), (2041 - 256, 256), (1500, 1)]        # (level0, L) of the density tests


def bucket_sweep_parts(W):
    """bucket_sweep() in as few consecutive parts as PLANTED_CAP allows at width W, each but the last of an even number of windows, so
    that pool = 2 keeps the two ends of a bucket in one row"""
    b = bucket_sweep()
    room = (PLANTED_CAP // (8 * W) - 1) // 2 * 2
    return [b[at:at + room] for at in range(0, b.size, room)]


def density_pair_buckets(level0, L, W):
    """the buckets whose two ends a pool = 2 density test plants at width W on the grid (level0, L): two on either side of both grid
    edges (so both clamps are hit where the scale has buckets outside the grid) and interior ones at even distances, as many rows as keep
    the counts [rows, W, L] within 16 MiB (at least 8)"""
    rows = min(max(8, (16 << 20) // (W * L * 4)), L + 4)
    edge = [k for k in (level0 - 2, level0 - 1, level0, level0 + 1, level0 + L - 2, level0 + L - 1, level0 + L, level0 + L + 1) if 0 <= k <= 2040]
    inner = [level0 + 2 + i * max(L - 4, 0) // max(rows - 8, 1) for i in range(max(rows - 8, 0))]
    return sorted(set(edge) | {k for k in inner if level0 <= k < level0 + L and k <= 2040})


# ------------------------------------------------------------------ deep slabs (test_deep_slabs_cpu.py, test_gpu_deep_slabs.py)
#
# A run of windows [w0, w0 + n) deep in a long stream reads source samples from base = w0 S D_eff on (D_eff the product of the chain's
# decimations).  The referee is an oracle chain over the SLAB alone, samples [base, base + count) of the described stream: base is a
# multiple of every stage's decimation, so the slab's window j is the stream's window w0 + j, every FIR centre falls where it does in the
# whole stream, and shift stage k (whose input runs at the source rate over the decimations before it) gets the reference's own f32
# multipliers of the absolute indices base_k + i planted through override_shift, base_k = base / (those decimations).  Everything the
# oracle makes of a chain is then available deep in the stream: norms, glyph codes, freq_levels digits, marks and read_at blocks.
# The slabs are chosen (a condition on the inputs, held by test_deep_slabs_cpu.py on the reference alone) so that NO multiplier component
# of any shift stage is ambiguous in them: the NCO rule then excuses nothing and the comparison is byte for byte.

DEEP_N = (1 << 34) + 12_345                      # the described stream: 2^34 samples and an odd tail
DEEP_MAX_WINDOWS = 64
DEEP_SLAB_CAP = 1 << 20
_DEEP_EPI = {"norms": 0, "glyph": 1, "bucket": 2, "blocks": 3, "mark": 4}
DEEP_GLYPH_RNG = (0.001, 0.5)
DEEP_DEPTHS = ("x32", "x33", "end")


def deep_run_windows(tile):
    """windows per run: 3 tiles + 5, or as many whole tiles + 5 as DEEP_MAX_WINDOWS holds (one tile + 5 where the tile itself is that
    large): a run that starts on a tile ends in a ragged one and can hold a sample strictly inside"""
    return min(3 * tile + 5, 5 + tile * ((max(DEEP_MAX_WINDOWS, tile + 5) - 5) // tile))


class DeepCase:
    """one chain of the deep-slab tests.  stages: [("shift", hz) | ("lowpass", (hz, D, T)), ...] source to sink; sink: norms / glyph /
    bucket / mark / blocks (the write sink: W is the block length, S is ignored); policy: "builtin" (QD_KERNEL_NO_PLAN_TIME) / "generic" /
    "specialise", never auto — a described 2^34-sample stream makes the auto policy compile; family(info, kernel name) says whether the
    plan is the intended kernel; tile: the plan's tile_windows (the GPU test holds the plan to it), which aligns the runs and sizes
    them: 3 tiles + 5 windows, a ragged last tile, see deep_run_windows; N: the described length; paths: also through 64 KiB chunks.
    Every case has three runs (DEEP_DEPTHS): "x32" / "x33" contain source sample 2^32 / 2^33 strictly inside, "end" is the stream's
    last windows."""

    def __init__(self, name, fmt, stages, W, S, family, sink="norms", policy="builtin", sr=21_000_000, tile=1, tile_hint=None,
                 N=DEEP_N, paths=False):
        self.name, self.fmt, self.stages, self.W, self.S, self.family = name, fmt, list(stages), W, (W if sink == "blocks" else S), family
        self.sink, self.policy, self.sr, self.tile, self.tile_hint, self.N = sink, policy, sr, tile, tile_hint, N
        self.n, self.paths = deep_run_windows(tile), paths

    def __repr__(self):
        return self.name

    epilogue = property(lambda self: _DEEP_EPI[self.sink])
    shifted = property(lambda self: any(k == "shift" for k, _ in self.stages))
    lowpasses = property(lambda self: [a for k, a in self.stages if k == "lowpass"])
    chain = property(lambda self: (self.stages, self.W, self.S, self.sr))

    def step(self):
        """source samples between window starts, S D_eff"""
        return source_block(self.stages, self.W, self.S, 1)[0]

    def span(self, n):
        """source samples windows [0, n) read"""
        return source_block(self.stages, self.W, self.S, 0, n)[1]

    def seed(self):
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) + 20261019

    def runs(self, total_windows):
        """[(depth, w0, n), ...] of a stream of total_windows windows (the plan's n_windows): w0 a multiple of the tile"""
        out = []
        for depth in DEEP_DEPTHS:
            if depth == "end":
                w0 = -(-(total_windows - self.n) // self.tile) * self.tile
                n = total_windows - w0
            else:
                mark = (1 << 32) if depth == "x32" else (1 << 33)
                w0 = (mark // self.step() - 1 - (self.n - self.tile) // 2) // self.tile * self.tile      # the mark's window is inside the run
                n = self.n
            out.append((depth, w0, n if depth != "end" else total_windows - w0))
        return out


def deep_geometry(engine, case):
    """(n_windows, complete windows, raw_step, raw_per_window) of the case's described stream from host arithmetic alone:
    qd_stages_geometry, and for the one-stage write sink, which it leaves to the plan, the header's floor((n - T) / (B D)) full blocks"""
    if case.sink == "blocks" and len(case.lowpasses) == 1:
        _, D, T = case.lowpasses[0]
        n = (case.N - T) // (case.W * D)
        return n, n, case.W * D, case.W * D + T
    info, done = engine.stages_geometry(case.fmt, case.sr, case.N, case.stages, case.W, case.S, case.epilogue)
    return int(info.n_windows), int(done), int(info.raw_step), int(info.raw_per_window)


def deep_slab_range(case, depth, w0, n):
    """(base, count): the slab of a run — from the first sample of window w0 to the end of window w0 + n (one window more than the run:
    the sink's loop is `while i < len - W`; the write sink's blocks need none), or, for the "end" run, to the end of the stream"""
    base = w0 * case.step()
    return base, (case.N - base if depth == "end" else case.span(n + (case.sink != "blocks")))


def deep_shift_bases(case, base):
    """[(ratio, base_k, decimation before stage k), ...] of the shift stages, source to sink"""
    out, dec = [], 1
    ratios = iter(shift_ratios(case.chain))
    for kind, arg in case.stages:
        if kind == "shift":
            assert base % dec == 0
            out.append((next(ratios), base // dec, dec))
        else:
            dec *= int(arg[1])
    return out


def deep_ambiguous(case, base, count):
    """the ambiguous multiplier components of every shift stage over the slab [base, base + count), as (stage, n, comp)"""
    out = []
    for k, (ratio, bk, dec) in enumerate(deep_shift_bases(case, base)):
        out += [(k, n, comp) for n, comp, _ in ambiguous_components(ratio, bk, bk + -(-count // dec))]
    return out


_DEEP_REFS = {}


def deep_reference(oracle, case, depth, w0, n, index_bits=None):
    """(slab bytes as a read-only uint8 array, base, the oracle's output of windows [w0, w0 + n) of the case's sink, the glyph / mark
    range used or None).  Seeded by the case's name and w0; built once per (case, w0, n).  The mark sink's min is the median of the
    reference's per-window maxima, so that both marks occur.
    index_bits (the CPU test of the comparison's bite only): plant the multipliers of the absolute indices truncated to that many bits."""
    key = (case.name, w0, n, index_bits)
    if key in _DEEP_REFS:
        return _DEEP_REFS[key]
    base, count = deep_slab_range(case, depth, w0, n)
    rng = np.random.default_rng(case.seed() + w0 % 1_000_003)
    if case.fmt == 0:
        raw = (rng.standard_normal((count, 2)) * 0.03).astype(np.float32).view(np.uint8).reshape(-1)
    else:
        raw = rng.integers(0, 256, count * FMT_BYTES[case.fmt], dtype=np.uint8)
    ch = oracle.Chain.from_bytes(raw, case.fmt, case.sr)
    shifts = iter(deep_shift_bases(case, base))
    k = 0
    for kind, arg in case.stages:
        if kind == "shift":
            ch = ch.shift(arg)
            ratio, bk, dec = next(shifts)
            m = -(-count // dec)
            if index_bits is None:
                c, s = oracle.shift_multipliers_f64(ratio, bk, m)      # (f64 as f32): the cast of src/shift.rs:49-50
            else:                                                      # NOT the referee: what an NCO that kept index_bits of the index would use
                c, s = (np.concatenate(x) for x in zip(*[oracle.shift_multipliers_f64(ratio, (bk + i) & ((1 << index_bits) - 1), 1) for i in range(m)]))
            ch.override_shift(k, np.arange(m, dtype=np.uint64), c.astype(np.float32), s.astype(np.float32))
            k += 1
        else:
            ch = ch.lowpass(*arg)
    W, S, used = case.W, case.S, None
    if case.sink == "blocks":
        rows = []
        for b in range(n):
            got, blk = ch.read_at(b * W, W)
            assert got == W, (case.name, b, got)
            rows.append(blk)
        ref = np.concatenate(rows)
    elif case.sink == "bucket":
        ref = ch.freq_levels(W, S, max_windows=n)
    elif case.sink == "norms":
        ref = ch.spark_fft(W, S, max_windows=n, want_codes=False)[0]
    elif case.sink == "glyph":
        used = DEEP_GLYPH_RNG
        ref = ch.spark_fft(W, S, rng=used, max_windows=n, want_norms=False)[1]
    else:
        norms = ch.spark_fft(W, S, max_windows=n, want_codes=False)[0]
        used = (float(np.median(norms.max(axis=1))), 1.0)
        ref = (ch.spark_fft(W, S, rng=used, max_windows=n, want_norms=False)[1] != 0).any(axis=1).astype(np.uint8)
    assert ref.shape[0] == n * (W if case.sink == "blocks" else 1), (case.name, w0, n, ref.shape)
    raw.setflags(write=False)
    ref.setflags(write=False)
    _DEEP_REFS[key] = (raw, base, ref, used)
    return _DEEP_REFS[key]


_SH = 999_983                                    # no ambiguous component in the slabs below (test_deep_slabs_cpu.py); 280 000 Hz has one every 75 samples
_SH2 = 1_000_003                                 # the two-stage cases' 295 000-sample slabs: 999 983 Hz has one ambiguous component in two of them
_SHL = [("shift", _SH)]
_LP = lambda lp: [("lowpass", lp)]               # noqa: E731
_GEN_LP = (700_000, 10, 24)
_HALF = (5_000_000, 8, 384)
_LONG = (900_000, 16, 256)
_SLSLS = [("shift", 123_457), ("lowpass", _CASC[0]), ("shift", -61_001), ("lowpass", _CASC[1]), ("shift", 7_919)]
_K_SPARK = _fam(kind=1, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0)
_K_CASC, _K_CFG2, _K_P3S = _fam(part="qd::k_cascade<"), _fam(kind=1, kernel="k_chain", eq_flags=65800), _fam(kind=1, kernel="k_chain_pipe3s")

DEEP_CASES = [
    # built-in FixedGeo k_chain: cfg2's and cfg3''s geometry behind a real shift; cfg4's without one (bit-exact indexing only)
    DeepCase("builtin-cfg2", 0, _SHL + _LP(_CFG2), 128, 128, _K_CFG2, tile=2, paths=True),
    DeepCase("builtin-cfg2-glyph", 0, _SHL + _LP(_CFG2), 128, 128, _K_CFG2, sink="glyph", tile=2),
    DeepCase("builtin-cfg2-bucket", 0, _SHL + _LP(_CFG2), 128, 128, _K_CFG2, sink="bucket", tile=2),
    DeepCase("builtin-cfg3p", 0, _SHL + _LP(_CFG3P), 128, 128, _fam(kind=1, kernel="k_chain", eq_flags=65868), tile=1),
    DeepCase("builtin-cfg3p-mark", 0, _SHL + _LP(_CFG3P), 128, 128, _fam(kind=1, kernel="k_chain"), sink="mark", tile=1),
    DeepCase("builtin-cfg4", 0, _LP(_CFG4), 1024, 1024, _fam(kind=1, kernel="k_chain", eq_flags=8392), sr=100_000_000, tile=1),
    # built-in streaming three-stage kernel, 64 / 16 behind 400 taps / 32: the cf32 and the cs8 set
    DeepCase("builtin-pipe3s-cf32", 0, _SHL + _LP(_CFG3), 64, 16, _K_P3S, tile=14, paths=True),
    DeepCase("builtin-pipe3s-cf32-glyph", 0, _SHL + _LP(_CFG3), 64, 16, _K_P3S, sink="glyph", tile=14),
    DeepCase("builtin-pipe3s-cf32-bucket", 0, _SHL + _LP(_CFG3), 64, 16, _K_P3S, sink="bucket", tile=14),
    DeepCase("builtin-pipe3s-cs8", 1, _SHL + _LP(_CFG3), 64, 16, _K_P3S, tile=14),
    # runtime geometry (DynGeo): every format behind shift + lowpass — their NCO rows are kThreads * (samples per load) long, so the row
    # index differs per format —, and the chain kernel without a lowpass at S < W
    DeepCase("generic-cf32", 0, _SHL + _LP(_GEN_LP), 16, 5, _GENERIC, policy="generic", tile=32),
    DeepCase("generic-cs8", 1, _SHL + _LP(_GEN_LP), 16, 5, _GENERIC, policy="generic", tile=32),
    DeepCase("generic-cu8", 2, _SHL + _LP(_GEN_LP), 16, 5, _GENERIC, policy="generic", tile=32),
    DeepCase("generic-cs16", 3, _SHL + _LP(_GEN_LP), 16, 5, _GENERIC, policy="generic", tile=32),
    DeepCase("generic-cf32-glyph", 0, _SHL + _LP(_GEN_LP), 16, 5, _GENERIC, sink="glyph", policy="generic", tile=32),
    DeepCase("generic-cf32-bucket", 0, _SHL + _LP(_GEN_LP), 16, 5, _GENERIC, sink="bucket", policy="generic", tile=32),
    DeepCase("generic-cu8-nolp", 2, _SHL, 64, 16, _GENERIC, policy="generic", tile=16),
    DeepCase("generic-cs16-nolp", 3, _SHL, 64, 16, _GENERIC, policy="generic", tile=16),
    DeepCase("generic-cf32-nolp-mark", 0, [], 64, 16, _GENERIC, sink="mark", policy="generic", tile=16),
    # plan-time builds of the chain templates, one each: a decimation that is no power of two, half-window tiles, the long-filter policy's
    # 512-thread tile (T >= 8 D, S = W), and the tile-at-a-time three-stage kernel k_chain_pipe3 (a tile hint: the library's own choice
    # for 64 / 16 is the streaming form).  The cfg3' recipe's flags run deep as the built-in kernel above.
    DeepCase("specialise-d12", 0, _SHL + _LP(_D12), 256, 256, _fam(kind=2, kernel="k_chain"), policy="specialise", tile=1),
    DeepCase("specialise-half-window", 0, _LP(_HALF), 1024, 1024, _fam(kind=2, kernel="k_chain", flags=8192), policy="specialise",
             sr=100_000_000, tile=1),
    DeepCase("specialise-long-filter-512", 0, _SHL + _LP(_LONG), 512, 512, _fam(kind=2, kernel="k_chain", threads=512), policy="specialise", tile=1),
    DeepCase("specialise-pipe3", 1, _SHL + _LP(_CFG3), 64, 16, _fam(kind=2, kernel="k_chain_pipe3", flags=32768, no_flags=131072, threads=1024),
             policy="specialise", tile=12, tile_hint=[12, 512, 1, 8, 4, 2, 1 | (32800 << 8), 0]),
    # wave-local, behind a shift: the built-in k_spark with its lane table, k_spark2, the interleaved launches on their phase grids
    DeepCase("spark-cf32-w8", 0, _SHL, 8, 8, _K_SPARK, tile=64),
    DeepCase("spark-cf32-w64", 0, _SHL, 64, 64, _K_SPARK, tile=8),
    DeepCase("spark-cf32-w64-glyph", 0, _SHL, 64, 64, _K_SPARK, sink="glyph", tile=8),
    DeepCase("spark-cf32-w64-bucket", 0, _SHL, 64, 64, _K_SPARK, sink="bucket", tile=8),
    DeepCase("spark-cf32-w1024", 0, _SHL, 1024, 1024, _K_SPARK, tile=1),
    DeepCase("spark-cs8-w128", 1, _SHL, 128, 128, _K_SPARK, tile=4),
    DeepCase("spark-cs16-w128", 3, _SHL, 128, 128, _K_SPARK, tile=4),
    DeepCase("spark2-cf32-w128", 0, _SHL, 128, 128, _fam(kind=2, kernel="k_spark2", flags=_SPARK | _SPARK2), policy="specialise", tile=8),
    DeepCase("spark2-cf32-w128-glyph", 0, _SHL, 128, 128, _fam(kind=2, kernel="k_spark2", flags=_SPARK | _SPARK2), sink="glyph", policy="specialise", tile=8),
    # the interleaved form: a k_spark built for 64 / 16 whose own tile is 8 windows while the plan's tile_windows is R * (512 / W) = 4 * 8,
    # the unit of its W / S = 4 launches' NCO row grids — only a plan with spark_R = 4 reports that
    DeepCase("interleaved-w64-s16", 0, _SHL, 64, 16, _fam(kind=2, kernel="k_spark", flags=_SPARK, no_flags=_SPARK2 | _SPARK0, part="FixedGeo<64, 16, 1, 0, 8,"),
             policy="specialise", tile=32),
    # wave-local, no shift: a window per lane (window indices past 2^32: S = 2)
    DeepCase("spark0-w4-s2", 0, [], 4, 2, _fam(kind=2, kernel="k_spark0", flags=_SPARK | _SPARK0), policy="specialise", tile=64),
    # k_cascade: lowpass lowpass, and shift lowpass shift lowpass shift (the inner shifts' absolute indices are base / 4 and base / 16)
    DeepCase("cascade-ll", 0, _LP(_CASC[0]) + _LP(_CASC[1]), 16, 8, _K_CASC, sr=2_000_000, tile=1),
    DeepCase("cascade-slsls", 0, _SLSLS, 16, 8, _K_CASC, sr=2_000_000, tile=1),
    DeepCase("cascade-slsls-glyph", 0, _SLSLS, 16, 8, _K_CASC, sink="glyph", sr=2_000_000, tile=1),
    DeepCase("cascade-slsls-bucket", 0, _SLSLS, 16, 8, _K_CASC, sink="bucket", sr=2_000_000, tile=1),
    # write sinks: the one-stage QD_EPI_CF32_BLOCKS at two block lengths, the cascade's
    DeepCase("write-b64", 0, _SHL + _LP(_CFG2), 64, 64, _GENERIC, sink="blocks", tile=4),
    DeepCase("write-b1024", 1, _SHL + _LP(_CFG2), 1024, 1024, _GENERIC, sink="blocks", tile=1),
    DeepCase("cascade-write-b1024", 1, _SHL + _LP(_CASC[0]) + _LP(_CASC[1]), 1024, 1024, _fam(part="qd::k_cascade_write<"), sink="blocks", tile=1),
    # the two-stage plan: a window past the LDS tile, behind a shift
    DeepCase("two-stage-w1024", 1, [("shift", _SH2)] + _LP(_CFG3P), 1024, 1024, _fam(part="two stages:"), tile=1, paths=True),
    DeepCase("two-stage-w1024-glyph", 1, [("shift", _SH2)] + _LP(_CFG3P), 1024, 1024, _fam(part="two stages:"), sink="glyph", tile=1),
    DeepCase("two-stage-w1024-bucket", 1, [("shift", _SH2)] + _LP(_CFG3P), 1024, 1024, _fam(part="two stages:"), sink="bucket", tile=1),
]


# ------------------------------------------------------------------ qd_gen against the oracle (test_gen_cpu.py, test_gpu_gen.py)
#
# The rule: a generated sample equals the reference's bytes wherever none of its terms cos(f), sin(f) (src/gen.rs:41, before the f32
# casts: oracle.gen_terms_f64) is ambiguous under nco_candidates(term, NCO_ABS_ERR) — the bound covers a device sincos (<= 2 ulp of a
# value <= 1) plus glibc's ulp —, and lies between the f32 sums of the low and of the high candidates where one is (f32 addition is
# monotone in either addend, and so is the sequential sum).

GEN_BLOCK = 1 << 16
GEN_SR = 100_000_000


def gen_tone_lists(vec_tones):
    """name -> (tones, sample rate): cfg4's own list; 1, 2, 64 and 255 tones with negative, zero and repeated frequencies; tones of
    magnitude 2^40 and 2^62 Hz, whose arguments take the huge-argument reduction of a sincos"""
    rng = np.random.default_rng(20261019)
    t64 = [int(v) for v in rng.integers(-49_999_999, 50_000_000, 64)]
    t64[3], t64[10], t64[40], t64[41] = 0, t64[9], -t64[5], 0
    t255 = [int(v) | 1 for v in rng.integers(-49_999_999, 50_000_000, 255)]
    return {"cfg4": ([int(v) for v in vec_tones], GEN_SR), "one": ([1_234_567], GEN_SR), "two": ([-999_983, 0], 21_000_000), "t64": (t64, GEN_SR),
            "t255": (t255, GEN_SR), "huge": ([(1 << 40) + 1, -((1 << 62) + 3), 12_345], GEN_SR)}


GEN_FIRSTS = {"0": 0, "2^24-100": (1 << 24) - 100, "2^32-2^15": (1 << 32) - (1 << 15), "2^40": 1 << 40, "2^53-2^15": (1 << 53) - (1 << 15), "2^63": 1 << 63}
# the short lists, cheap, at every offset; the long ones at one to three of them
GEN_RUNS = [(name, first) for name in ("one", "two", "huge") for first in GEN_FIRSTS] + \
           [("cfg4", "0"), ("cfg4", "2^32-2^15"), ("t64", "2^24-100"), ("t64", "2^53-2^15"), ("t64", "2^63"), ("t255", "2^40")]

GEN_TERM_P = 5.8e-7
"""The chance that one term cos(f) or sin(f) of uniformly distributed phase is ambiguous under NCO_ABS_ERR = 2e-15.  A value in the binade
[2^-k-1, 2^-k) has f32 rounding boundaries 2^-k-24 apart and is ambiguous within 2e-15 of one: a chance of 4e-15 * 2^(k+24).  |cos| falls
into binade 0 with probability 2/3 (4.5e-8 in all) and into binade k >= 1 with (2 / pi) 2^-(k+1), which gives (2 / pi) 4e-15 2^23 = 2.1e-8
for EACH binade until the boundaries lie closer than the bound itself (k = 23): 4.9e-7; below 2^-24 every value is ambiguous: 3.8e-8.
Measured: 17 samples of 65 536 with 255 tones, 5.1e-7 per term."""


def gen_ambiguous_bound(name, tones, n):
    """how many of n consecutive samples of a tone list may hold an ambiguous term: 3 x the expected count of 2 K n GEN_TERM_P (K the
    tones that turn: a zero frequency gives exactly (1, 0)) + 5, a margin no Poisson count of that mean reaches; cfg4's own list adds its
    structure — its tones are odd multiples of 100 MHz / 256, the sines cross zero at every 128th sample and the cosines at the 64th
    between: n / 64 + 1 samples"""
    turning = sum(1 for t in tones if t != 0)
    return int(np.ceil(3 * 2 * turning * n * GEN_TERM_P)) + 5 + (n // 64 + 1 if name == "cfg4" else 0)


_GEN_REFS = {}


def _maybe_ambiguous(v, f, eps=NCO_ABS_ERR):
    """a cheap superset of the elements of the f64 array v (f its f32 rounding) within eps of an f32 rounding boundary: the distance to
    f against half the f32 spacing at f, taken as the quarter where f is a power of two (the spacing below it is half), with a margin
    of 4 eps.  nco_candidates decides among those."""
    d = np.abs(v - f.astype(np.float64))
    u = np.spacing(np.abs(f)).astype(np.float64)
    mant, _ = np.frexp(f)
    half = np.where(np.abs(mant) == 0.5, u / 4, u / 2)
    return half - d <= 4 * eps


def gen_reference(oracle, tones, sr, first, n, piece=4096):
    """(ref float32 (n, 2), ambiguous bool (n), lo float32 (n, 2), hi float32 (n, 2)): the oracle's Gen::read_at(first, n), the samples
    with an ambiguous term, and the sums of the low / high candidates.  Built once per argument set, read-only."""
    key = (tuple(tones), sr, first, n)
    if key not in _GEN_REFS:
        got, ref = oracle.Chain.gen(tones, sr, 1.0).read_at(first, n)
        assert got == n
        amb = np.zeros(n, dtype=bool)
        lo, hi = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        for a in range(0, n, piece):
            m = min(piece, n - a)
            for comp, v in enumerate(oracle.gen_terms_f64(tones, sr, first + a, m)):
                l = v.astype(np.float32)
                h = l.copy()
                at = _maybe_ambiguous(v, l)
                # a term that is exactly 0 is sin(+-0): pi is irrational, no other double is a zero of sin, and every sincos returns
                # its argument there — it has one candidate
                at &= v != 0.0
                l[at], h[at] = nco_candidates(v[at])
                amb[a:a + m] |= (l != h).any(axis=1)
                lo[a:a + m, comp] = np.cumsum(l, axis=1, dtype=np.float32)[:, -1]
                hi[a:a + m, comp] = np.cumsum(h, axis=1, dtype=np.float32)[:, -1]
        for x in (ref, amb, lo, hi):
            x.setflags(write=False)
        _GEN_REFS[key] = (ref, amb, lo, hi)
    return _GEN_REFS[key]


def gen_rule_violations(ref, amb, lo, hi, got):
    """samples of `got` that break the rule: (indices that differ from ref without an ambiguous term, indices outside [lo, hi] with one)"""
    got = np.asarray(got, dtype=np.float32).reshape(ref.shape)
    ne = (got.view(np.uint32) != ref.view(np.uint32)).any(axis=1)
    with np.errstate(invalid="ignore"):
        outside = ~((got >= lo) & (got <= hi)).all(axis=1)
    return np.flatnonzero(ne & ~amb), np.flatnonzero(amb & outside)


GEN_LONG = dict(tones="t64", first=(1 << 32) - (1 << 23) - 5, n=(1 << 24) + 4097)      # one call past k_gen's 65536 blocks of 256: its grid-stride branch


def gen_long_stretches(n, stretch=1 << 14):
    """offsets of the four stretches of a long call that are held to the oracle: its first and last samples and two inner stretches,
    the second of them across the end of the grid's first pass (sample 2^24)"""
    return [0, n // 3, (1 << 24) - stretch + 2048, n - stretch]


# ------------------------------------------------------------------ designed on/off shapes (test_emission_shapes_cpu.py, test_gpu_emission_shapes.py)
#
# Boolean masks [n windows, W bins] on which a tiled connected-component labelling goes wrong, and the cf32 stream that plants one:
# a window that is the inverse DFT of a row of levels has exactly those levels as its norms, up to the transform's rounding.

EMISSIONS_TILE_COLS = 256                        # kEmissionsTileCols: a tile of the emission kernels is at most this many bins wide


def emissions_tile_rows(W):
    """emissions_tile_rows of qd_emissions.h: 8 rows at W >= 256, 16 at 128, 512 at 4, 1024 at 2 and 1"""
    return 2048 // (2 * ((min(int(W), EMISSIONS_TILE_COLS) + 1) // 2))


def serpentine(n, W, phase=0):
    """Every other window is fully on; the window between two of them holds one cell, at bin 0 and bin W - 1 in turn: one emission that
    sweeps every row in both directions.  phase 0: the odd windows are the full ones, so a full row is the last row above every
    tile-row border (window k tr - 1, tr even); phase 1: the even ones, so a single connector cell is."""
    m = np.zeros((n, W), dtype=bool)
    m[(1 - phase) % 2::2] = True
    for k, i in enumerate(range(phase % 2, n, 2)):
        m[i, 0 if k % 2 == 0 else W - 1] = True
    return m


def spiral(n, W, gap=1):
    """A single-armed rectangular spiral from (0, 0) inwards, clockwise, one cell thick, `gap` off cells between two turns: one
    emission; with gap 1 the off cells are one 4-connected region too"""
    m = np.zeros((n, W), dtype=bool)
    step = gap + 1
    t, b, l, r = 0, n - 1, 0, W - 1              # the rows and bins that keep `gap` cells away from what is drawn, the arm's own line apart
    i = j = d = 0
    m[0, 0] = True
    while t <= b and l <= r:
        if d == 0:
            if r <= j:
                break
            m[i, j:r + 1] = True
            j, t = r, i + step
        elif d == 1:
            if b <= i:
                break
            m[i:b + 1, j] = True
            i, r = b, j - step
        elif d == 2:
            if l >= j:
                break
            m[i, l:j + 1] = True
            j, b = l, i - step
        else:
            if t >= i:
                break
            m[t:i + 1, j] = True
            i, l = t, j + step
        d = (d + 1) % 4
    return m


def rings(n, W):
    """The cells whose distance to the border is even: nested closed rings, none touching another, each around the next.  Ring d (d even)
    spans windows d ... n - 1 - d and bins d ... W - 1 - d, so the innermost ends first."""
    i, b = np.arange(n)[:, None], np.arange(W)[None, :]
    return np.minimum(np.minimum(i, n - 1 - i), np.minimum(b, W - 1 - b)) % 2 == 0


def comb_lengths(n, W, seed):
    """the tooth lengths of comb(n, W, seed), one per even bin: seeded, 1 ... n - 3, the greatest exactly once and not at bin 0"""
    rng = np.random.default_rng(seed)
    ln = rng.integers(1, n - 3, (W + 1) // 2)    # 1 ... n - 4
    ln[int(rng.integers(1, ln.size))] = n - 3
    return ln


def comb(n, W, seed):
    """Window 0 is off, window 1 a full spine, and from every even bin a tooth of comb_lengths hangs down from window 2: one emission,
    which stays open through a seam as many cells of one root that are no neighbours of each other, and which ends where its longest
    tooth ends, in window n - 2 at that tooth's bin"""
    m = np.zeros((n, W), dtype=bool)
    m[1] = True
    for k, ln in enumerate(comb_lengths(n, W, seed)):
        m[2:2 + int(ln), 2 * k] = True
    return m


def corner_figures(n, W, tr):
    """[(window k tr, bin 256 j, figure, mirrored)] of corners(n, W, tr): the interior tile corners in reading order, the figures
    0, 1, 2 in rotation, mirrored on every second round"""
    out = []
    for k in range(1, (n - 1) // tr + 1):
        for j in range(1, (W - 1) // EMISSIONS_TILE_COLS + 1):
            out.append((k * tr, j * EMISSIONS_TILE_COLS, len(out) % 3, (len(out) // 3) % 2))
    return out


def corners(n, W, tr):
    """At every interior tile corner (between windows k tr - 1 and k tr, bins 256 j - 1 and 256 j) one of three figures: 0, two cells
    that meet only diagonally across the corner (two emissions of one cell); 1, an L through three of the four tiles; 2, a block of
    2 x 2 cells, one in each tile.  Mirrored figures use the other diagonal."""
    m = np.zeros((n, W), dtype=bool)
    for i, b, fig, mirrored in corner_figures(n, W, tr):
        left, right = (b, b - 1) if mirrored else (b - 1, b)
        if fig == 2:
            m[i - 1:i + 1, b - 1:b + 1] = True
        else:
            m[i - 1, left] = m[i, right] = True
            if fig == 1:
                m[i, left] = True
    return m


def checker(n, W):
    """(window + bin) even: every on cell is an emission of its own, and every slot (pair of bins) of every row holds a root"""
    return (np.arange(n)[:, None] + np.arange(W)[None, :]) % 2 == 0


def shape_levels(mask, seed):
    """f32 levels of a mask: seeded integers 1 ... 3 where it is on, 0 where it is off"""
    rng = np.random.default_rng(seed)
    return np.where(mask, rng.integers(1, 4, mask.shape), 0).astype(np.float32)


def tone_stream(mask_levels):
    """The cf32 bytes of n + 1 windows of W samples for f32 levels [n, W] (0: off): window i is the inverse DFT, normalised by 1 / W, of
    row i laid in the norms sink's fftshifted order (column o is frequency o ^ W/2), so that the norm of cell (i, o) is its level and
    an off cell's is the transform's rounding alone; the trailing window is zeros, as impulse_stream's.  W is a power of two."""
    lv = np.ascontiguousarray(mask_levels, dtype=np.float32)
    n, W = lv.shape
    assert W >= 2 and W & (W - 1) == 0
    x = np.fft.ifft(lv.astype(np.float64)[:, np.arange(W) ^ (W // 2)], axis=1)
    out = np.zeros((n + 1, W, 2), dtype=np.float32)
    out[:-1, :, 0], out[:-1, :, 1] = x.real, x.imag
    return out.tobytes()
