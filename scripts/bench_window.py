"""Development: what the window of a windowed plan costs (qd_chain_desc.windowing = 1), on one device-resident cf32
stream in one process.  Two pairs of plans, each pair timed alternately, 12 steps a leg, HIP events around qd_plan_run:
  recipe   cf32, shift 280000, 192 taps / 32, W = S = 128 (a shape without a table entry), kernel_policy = 2: the plan-time build of the
           shape's recipe with and without the variant bit kGeoWindow — the same kernel but for one table read and two products an output
  headline the north_star chain (200 taps / 32, W = S = 128): the built-in table kernel, unwindowed, beside the windowed plan, which runs the
           plan-time build of the recipe because the table kernels carry no window — the gap is what that costs
usage: python scripts/bench_window.py [log2 samples, default 30] [log path, default profiles/r14/window_sink.log]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import statistics
import torch
import bench
import quadrs_amd as Q

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 30)
dev = torch.device("cuda", 0)
src = bench.synth_slab(torch, 0, 0, n, 0x5EED0002, dev)
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r14", "window_sink.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
log = open(log_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


PAIRS = (("recipe", dict(shift_hz=280000, lowpass=(200_000, 32, 192), width=128, stride=128, kernel_policy=2)),
         ("headline", dict(shift_hz=280000, lowpass=(200_000, 32, 200), width=128, stride=128)))
STEPS = 12
say(f"# {n} cf32 samples ({n * 8 / 2**30:.0f} GiB), {STEPS} steps per leg, alternating; ms per step (HIP events)")
for name, chain in PAIRS:
    plans = {"rect": Q.Plan(0, 21_000_000, n, **chain), "bh": Q.Plan(0, 21_000_000, n, windowing=Q.WINDOW_BH, **chain)}
    nw = plans["rect"].n_windows
    outs = {k: torch.empty(nw, 128, dtype=torch.float32, device=dev) for k in plans}
    for k, p in plans.items():
        say(f"{name} {k}: kind {p.info.kernel_kind} flags {p.info.kernel_flags} {p.kernel_name()}")
    for _ in range(2):
        for k, p in plans.items():
            p.run_device(src, outs[k])
    torch.cuda.synchronize()
    ms = {k: [] for k in plans}
    order = list(plans)
    for i in range(STEPS):
        for k in (order if i % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            plans[k].run_device(src, outs[k])
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    # the legs differ as a window makes them differ: the windowed rows sum to less (the window's mean is 0.36), and neither is empty
    a, b = float(outs["rect"][:4096].double().sum()), float(outs["bh"][:4096].double().sum())
    say(f"{name}: sum of the first 4096 rows rect {a:.6g} bh {b:.6g} ratio {b / a:.3f}")
    for k in order:
        v = ms[k]
        say(f"{name} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}, {n / statistics.median(v) / 1e3:.0f} Msamples/s")
    say(f"{name}: bh / rect = {statistics.median(ms['bh']) / statistics.median(ms['rect']):.4f}")
    for p in plans.values():
        p.close()
    del outs
