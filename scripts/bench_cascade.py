"""The cascaded chain at scale (qd_plan_create_stages, quadrs_amd/csrc/qd_cascade.h): one GPU, input resident in HBM.

16 GiB cf32 at 21 Msps: shift 280000 -> lowpass -decimate 4 2000000 (40 taps) -> lowpass -power 100 -decimate 8 200000 ->
sparkfft -width 128 — the output rate and algorithmic bytes of bench.py's default chain (cfg3') through two lowpass stages.
Same synthetic stream, same HIP-event timing and the same instruction-class VALU model as bench.py (its issue rates, helpers
and constants are imported, not restated), extended with the first stage's FIR and the window-overlap recompute.  Prints one
JSON line.  Accepts bench.py's profiling flags so that scripts/profile_round.sh can run it (BENCH_SCRIPT=scripts/bench_cascade.py).

--sink write: the same stream and stages into the write sink (read_at blocks of 4096 decimated cf32 samples, k_cascade_write), timed
alternately with the sparkfft cascade in one process over one HBM-resident slab; one JSON line with both legs' kernel ms,
Gsamples/s of input and (bytes read + bytes written) / s.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402  (helpers and constants of the benchmark; sets the harness gate)

STAGES = [("shift", 280000), ("lowpass", (2_000_000, 4, 40)), ("lowpass", (200_000, 8, 200))]
CFG = dict(fmt=0, n=1 << 31, sr=21_000_000, W=128, S=128, stages=STAGES)


def ops_per_sample(cfg):
    """bench.py::valu_ops_per_sample's classes per INPUT sample, for a cascade.  A window reads a source span of
    (W D2 + T2) D1 + T1 samples but advances S D2 D1: unpack, the source-rate NCO and the first FIR (W D2 + T2 outputs of T1 taps)
    are paid on the span; the second FIR (W outputs of T2 taps), the later NCOs (second order, on their own stage's samples),
    FFT and |X| on the window.  Returns (scalar f32, f64-rate, packed f32) operations."""
    W, S = cfg["W"], cfg["S"]
    lps = [a for k, a in cfg["stages"] if k == "lowpass"]
    (_, D1, T1), (_, D2, T2) = lps[0], (lps[1] if len(lps) > 1 else (0, 1, 0))
    n2 = W * D2 + T2 if len(lps) > 1 else W
    span, step = n2 * D1 + T1, S * D2 * D1
    pk = (2.0 * n2 * T1 + 2.0 * W * T2) / step
    f32 = (5.0 * W * math.log2(W) + 11.0 * W) / step
    f64 = 10.0 * W / step
    per_nco, n_lp = span, 0                 # samples each NCO multiplies per window: its own stage's
    for k, a in cfg["stages"]:
        if k == "lowpass":
            n_lp += 1
            per_nco = n2 if n_lp == 1 else W
        else:
            pk += 3.0 * per_nco / step
            f64 += 14.0 * per_nco / step
    f32 += {0: 0.0, 1: 2.0, 2: 2.0, 3: 2.0}[cfg["fmt"]] * span / step
    pk += {0: 0.0, 1: 2.0, 2: 3.0, 3: 3.0}[cfg["fmt"]] * span / step
    return f32, f64, pk


def run_write_sink(args, cfg):
    """the write sink and the sparkfft cascade on the same slab, step for step alternating; kernel time from HIP events"""
    import numpy as np
    import torch
    import quadrs_amd as Q
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    bps, B_ = B.BPS[cfg["fmt"]], 4096
    spark = Q.Plan(cfg["fmt"], cfg["sr"], cfg["n"], stages=cfg["stages"], width=cfg["W"], stride=cfg["S"])
    write = Q.Plan(cfg["fmt"], cfg["sr"], cfg["n"], stages=cfg["stages"], width=B_, stride=B_, epilogue=Q.EPI_CF32_BLOCKS)
    nws, nww = spark.complete_windows(), write.complete_windows()
    count = max(sum(spark.src_range(0, nws)), sum(write.src_range(0, nww)))
    slab = B.synth_slab(torch, cfg["fmt"], 0, count, B.STREAM_SEED, device)
    out_s = torch.empty(nws, cfg["W"], dtype=torch.float32, device=device)
    out_w = torch.empty(nww * B_, 2, dtype=torch.float32, device=device)
    legs = {"write": (write, out_w, nww), "sparkfft": (spark, out_s, nws)}

    def step(name):
        plan, out, nw = legs[name]
        plan.run_device(slab, out, 0, nw, src_first=0, src_count=count)

    t_settle = time.perf_counter()
    while time.perf_counter() - t_settle < args.settle:
        step("write"); step("sparkfft")
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step("write"); step("sparkfft")
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for i in range(args.steps):
        for name in (("write", "sparkfft") if i % 2 == 0 else ("sparkfft", "write")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); step(name); b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    finite = bool(torch.isfinite(out_w).all().item()) and bool(torch.isfinite(out_s).all().item())
    res = {"workload": "cascade-write", "unit": "ms",
           "config": {"chain": "16 GiB cf32 @21Msps: shift 280000 -> lowpass -decimate 4 2000000 (40 taps) -> lowpass -power 100 -decimate 8 200000"
                      if cfg["n"] == CFG["n"] else f"2^{args.samples_log2} samples of the same chain",
                      "samples": cfg["n"], "steps": args.steps, "block": B_}, "outputs_finite": finite}
    for name, (plan, out, nw) in legs.items():
        kms = float(np.median(ms[name]))
        samples = nw * plan.info.raw_step
        read_b, written_b = plan.src_range(0, nw)[1] * bps, out.numel() * 4
        res[name] = {"kernel": plan.kernel_name(), "windows": nw, "ms_median": kms, "ms_min": float(np.min(ms[name])),
                     "ms_max": float(np.max(ms[name])), "gsamples_per_s": samples / (kms * 1e-3) / 1e9,
                     "bytes_read": read_b, "bytes_written": written_b, "gbytes_per_s": (read_b + written_b) / (kms * 1e-3) / 1e9,
                     "lds_bytes": plan.info.lds_bytes}
    res["value"] = res["write"]["ms_median"]
    res["write_over_sparkfft"] = res["write"]["ms_median"] / res["sparkfft"]["ms_median"]
    print(json.dumps(res), flush=True)
    return 0 if finite else 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=float, default=0.3)
    ap.add_argument("--samples-log2", type=int, default=None, help="override samples (2^k); rehearsals only")
    ap.add_argument("--workload", default="cascade", choices=["cascade"])
    ap.add_argument("--no-power", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(accepted for scripts/profile_round.sh; there is no CPU leg)")
    ap.add_argument("--no-others", action="store_true", help="(accepted for scripts/profile_round.sh)")
    ap.add_argument("--sink", default="sparkfft", choices=["sparkfft", "write"], help="write: the write sink against the sparkfft cascade")
    args = ap.parse_args()

    import numpy as np
    import torch
    import quadrs_amd as Q
    cfg = dict(CFG)
    if args.samples_log2:
        cfg["n"] = 1 << args.samples_log2
    if args.sink == "write":
        return run_write_sink(args, cfg)
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    bps = B.BPS[cfg["fmt"]]
    plan = Q.Plan(cfg["fmt"], cfg["sr"], cfg["n"], stages=cfg["stages"], width=cfg["W"], stride=cfg["S"])
    info, nw = plan.info, plan.complete_windows()
    first, count = plan.src_range(0, nw)
    slab = B.synth_slab(torch, cfg["fmt"], first, count, B.STREAM_SEED, device)
    out = torch.empty(nw, cfg["W"], dtype=torch.float32, device=device)

    def step():
        plan.run_device(slab, out, 0, nw, src_first=first, src_count=count)

    t_settle = time.perf_counter()
    while time.perf_counter() - t_settle < args.settle:
        step()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ev = {}
    t0 = time.perf_counter()
    for i in range(args.steps):
        if i % 4 == 0:
            ev[i] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[i][0].record()
            step()
            ev[i][1].record()
        else:
            step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kernel_ms = float(np.mean([a.elapsed_time(b) for a, b in ev.values()]))
    finite = bool(torch.isfinite(out).all().item())
    power = None if args.no_power else B.sample_power(step, torch, 2.5)

    samples = nw * info.raw_step
    alg_bytes = count * bps + nw * cfg["W"] * 4
    f32, f64, pk = ops_per_sample(cfg)
    ns = f32 * B.T_F32_NS + f64 * B.T_F64_NS + pk * B.T_PK_NS
    valu_roof = B.LANES_PER_CHIP / (ns * 1e-9) / 1e6
    kernel_msamples = samples / (kernel_ms * 1e-3) / 1e6
    achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
    hbm_roof = B.HBM_PEAK_GBPS * 1e9 / (alg_bytes / samples) / 1e6
    valu = {"achieved": kernel_msamples, "peak": valu_roof, "unit": "Msamples/s", "frac": kernel_msamples / valu_roof,
            "f32_ops_per_sample": f32 + 2.0 * pk, "f64_ops_per_sample": f64,
            "issue_ns_per_wave_instr": {"f32": B.T_F32_NS, "f64": B.T_F64_NS, "packed_f32": B.T_PK_NS}}
    if power and power.get("sclk_mhz_mean"):
        scale = power["sclk_mhz_mean"] / B.SCLK_MAX_MHZ
        valu.update(sclk_mhz=power["sclk_mhz_mean"], peak_at_sclk=valu_roof * scale, frac_at_sclk=kernel_msamples / (valu_roof * scale))
    res = {"workload": "cascade", "value": samples / (elapsed / args.steps) / 1e6, "unit": "Msamples/s", "ms_per_step": elapsed / args.steps * 1e3,
           "config": {"chain": "16 GiB cf32 @21Msps: shift 280000 -> lowpass -decimate 4 2000000 (40 taps) -> lowpass -power 100 -decimate 8 200000 -> sparkfft -width 128"
                      if cfg["n"] == CFG["n"] else f"2^{args.samples_log2} samples of the same chain",
                      "samples": cfg["n"], "windows": nw, "n_windows": plan.n_windows, "kernel_kind": info.kernel_kind,
                      "kernel_flags": info.kernel_flags, "threads": info.threads, "lds_bytes": info.lds_bytes},
           "outputs_finite": finite,
           "roofline": {"bound": "hbm" if hbm_roof <= valu_roof else "valu", "kernel": plan.kernel_name(), "kernel_ms": kernel_ms,
                        "algorithmic_bytes": alg_bytes,
                        "hbm": {"achieved": achieved, "peak": B.HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / B.HBM_PEAK_GBPS},
                        "valu": valu, "power": power}}
    print(json.dumps(res), flush=True)
    return 0 if finite else 4


if __name__ == "__main__":
    sys.exit(main())
