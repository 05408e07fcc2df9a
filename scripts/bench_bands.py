"""Development: the band traces' rate (qd_plan_bands) against the average-trace rows at pool 64 (qd_plan_mean,
section 3.13, whose code this work does not touch: its leg is the parent commit's) and one norms-sink pass on the same plan in the same
run, on one device-resident cf32 stream in one process: cfg3''s chain (shift -> 200-tap FIR decimate 32 -> W = S = 128) and the cfg3
shape (400 taps, W 64, S 16).  Legs, 12 steps each, alternating, each timed with HIP events:
  run         qd_plan_run of the norms plan into a device buffer             (one norms-sink pass)
  mean=64     qd_plan_mean into device rows at pool 64                       (yardstick: one load and one mean_add per value, too)
  bands=2     qd_plan_bands, the window cut into 2 equal bands, all six outputs into device rows
  bands=16    ... into 16 equal bands
  bands=W     ... into W one-bin bands
  one4        ... one band of 4 bins in the middle of the window
The partitions read every value once, as the mean does; what they add is the reduction across lanes per item and loads that are not
16 bytes wide.  usage: python scripts/bench_bands.py [log2 samples, default 31] [log path, default profiles/r12/bands_sink.log]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import statistics
import torch
import bench
import quadrs_amd as Q

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 31)
dev = torch.device("cuda", 0)
src = bench.synth_slab(torch, 0, 0, n, 0x5EED0002, dev)
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r12", "bands_sink.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
log = open(log_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


CHAINS = (("cfg3p", dict(shift_hz=280000, lowpass=(200_000, 32, 200), width=128, stride=128)),
          ("cfg3_shape", dict(shift_hz=280000, lowpass=(200_000, 32, 400), width=64, stride=16)))
STEPS = 12
say(f"# {n} cf32 samples ({n * 8 / 2**30:.0f} GiB), {STEPS} steps per leg, alternating; ms per step (HIP events)")
for cname, chain in CHAINS:
    p = Q.Plan(0, 21_000_000, n, **chain)
    nw, W = p.n_windows, chain["width"]
    out = torch.empty(nw, W, dtype=torch.float32, device=dev)
    sets = {"bands=2": [(k * W // 2, (k + 1) * W // 2) for k in range(2)], "bands=16": [(k * W // 16, (k + 1) * W // 16) for k in range(16)],
            f"bands={W}": [(b, b + 1) for b in range(W)], "one4": [(W // 2 - 2, W // 2 + 2)]}
    legs = {"run": lambda: p.run_device(src, out), "mean=64": lambda: p.mean(src, 64)}
    for k, b in sets.items():
        legs[k] = lambda b=b: p.bands(src, b)
    say(f"{cname}: {nw} windows of {W}, norms {nw * W * 4 / 2**20:.0f} MiB, {p.kernel_name()[:70]}")
    last = {}
    for _ in range(2):
        for k, f in legs.items():
            last[k] = f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    order = list(legs)
    for i in range(STEPS):
        for k in (order if i % 2 == 0 else order[::-1]):
            last[k] = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = legs[k]()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    # the legs agree with each other: one-bin bands are the norms, and every partition counts the same values
    bins, two, sixteen = last[f"bands={W}"], last["bands=2"], last["bands=16"]
    same = bool(((bins[0] == out) | out.isnan()).all()) and bool((bins[2] == (~out.isnan())).all())
    same = same and bool((two[2].sum(dim=1) == bins[2].sum(dim=1)).all()) and bool((sixteen[2].sum(dim=1) == bins[2].sum(dim=1)).all())
    same = same and bool((two[3].max(dim=1).values == bins[3].max(dim=1).values).all())
    say(f"{cname}: consistent {same}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    run, mean = statistics.median(ms["run"]), statistics.median(ms["mean=64"])
    for k in sets:
        a = statistics.median(ms[k])
        say(f"{cname}: {k} - run = {a - run:+.3f} ms, mean=64 - run = {mean - run:+.3f} ms, ratio {(a - run) / (mean - run):.2f}"
            + ("" if k == "one4" else f" -> {'within' if a - run <= 2 * (mean - run) else 'OUTSIDE'} 2x of the mean's time above one pass"))
    p.close()
    del out, last, bins, two, sixteen
