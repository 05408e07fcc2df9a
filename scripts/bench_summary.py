"""The level summary against the norms run it rides on (qd_plan_summarize): one GPU, input resident in HBM.

Two chains — cfg3' (bench.py's default: cf32, shift -> 200-tap FIR decimate 32 -> 128-point FFT, W = S = 128: the norms are 1.5 % of
the traffic) and the cfg3 shape (cs8, 400 taps, W 64, S 16: 25 %) — each on bench.py's noise-like stream and on an all-zero stream
(every value in histogram bucket 0: the worst case for the LDS counters).  Legs, alternating in one process and timed with HIP
events as in scripts/bench_cascade.py:
  run        qd_plan_run of the norms plan into a device buffer                        (the reference point, same commit)
  summarize  qd_plan_summarize over the same windows (the result's copy down included; the call synchronises)
The carrier's extra write and read of the norms sets the expected overhead.  Prints one JSON line per (chain, stream).

With a development library (python quadrs_amd/build.py --dev; QD_LIB_PATH=quadrs_amd/libquadrs_hip_dev.so) --layouts 0,1,2,3 times
k_summary's histogram layouts: bit 0 one copy per workgroup instead of one per wave, bit 1 no wave-uniform shortcut.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402  (helpers and constants of the benchmark; sets the harness gate)

CHAINS = {
    "cfg3p": dict(fmt=0, log2=29, sr=21_000_000, shift=280000, lp=(200_000, 32, 200), W=128, S=128),
    "cfg3": dict(fmt=1, log2=30, sr=21_000_000, shift=280000, lp=(200_000, 32, 400), W=64, S=16),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chains", default="cfg3p,cfg3")
    ap.add_argument("--streams", default="noise,zero")
    ap.add_argument("--samples-log2", type=int, default=None, help="override the stream length (2^k samples)")
    ap.add_argument("--layouts", default="0", help="development library only: QD_SUMMARY_LAYOUT values to time")
    args = ap.parse_args()

    import numpy as np
    import torch
    import quadrs_amd as Q
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    layouts = [int(v) for v in args.layouts.split(",")]
    dev_lib = "dev" in os.path.basename(os.environ.get("QD_LIB_PATH", ""))
    if layouts != [0] and not dev_lib:
        sys.exit("--layouts needs the development library (QD_LIB_PATH)")
    for name in args.chains.split(","):
        cfg = CHAINS[name]
        n = 1 << (args.samples_log2 or cfg["log2"])
        plan = Q.Plan(cfg["fmt"], cfg["sr"], n, shift_hz=cfg["shift"], lowpass=cfg["lp"], width=cfg["W"], stride=cfg["S"])
        nw = plan.n_windows
        first, count = plan.src_range(0, nw)
        out = torch.empty(nw, cfg["W"], dtype=torch.float32, device=device)
        for stream in args.streams.split(","):
            slab = B.synth_slab(torch, cfg["fmt"], first, count, B.STREAM_SEED, device)
            if stream == "zero":
                slab.zero_()
                if cfg["fmt"] == 2:
                    slab.fill_(128)
            legs = {"run": lambda: plan.run_device(slab, out, 0, nw, src_first=first, src_count=count)}
            for lay in layouts:
                def leg(lay=lay):
                    os.environ["QD_SUMMARY_LAYOUT"] = str(lay)
                    return plan.summarize(slab, 0, nw, src_first=first)
                legs[f"summarize{lay if layouts != [0] else ''}"] = leg
            last = {}
            for _ in range(args.warmup):
                for k, f in legs.items():
                    last[k] = f()
            torch.cuda.synchronize()
            ms = {k: [] for k in legs}
            order = list(legs)
            for i in range(args.steps):
                for k in (order if i % 2 == 0 else order[::-1]):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); last[k] = legs[k](); b.record()
                    torch.cuda.synchronize()
                    ms[k].append(a.elapsed_time(b))
            s = last[order[1]]
            ok = int(s.hist.sum()) + s.n_nan == nw * cfg["W"] and all(last[k].tobytes() == s.tobytes() for k in order[1:])
            norms_b, src_b = nw * cfg["W"] * 4, count * B.BPS[cfg["fmt"]]
            res = {"workload": "summary", "chain": name, "stream": stream, "samples": n, "windows": nw, "kernel": plan.kernel_name(),
                   "src_bytes": src_b, "norms_bytes": norms_b, "norms_share": norms_b / (norms_b + src_b), "consistent": bool(ok),
                   "min": float(s.min), "max": float(s.max), "q50": [float(v) for v in s.quantile(0.5)], "buckets_used": int((s.hist > 0).sum()),
                   "top_bucket_share": float(s.hist.max() / max(int(s.hist.sum()), 1))}
            for k in order:
                res[k] = {"ms_median": float(np.median(ms[k])), "ms_min": float(np.min(ms[k])), "ms_max": float(np.max(ms[k]))}
            for k in order[1:]:
                res[k]["over_run"] = res[k]["ms_median"] / res["run"]["ms_median"]
            print(json.dumps(res), flush=True)
            del slab
    return 0


if __name__ == "__main__":
    sys.exit(main())
