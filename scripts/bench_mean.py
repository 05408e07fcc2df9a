"""Development: the average-trace rows' rate (qd_plan_mean) against the peak-hold rows (qd_plan_pool, section
3.12, whose code this work does not touch: its leg is the parent commit's) on the same plan and pool in the same run, on one
device-resident 16 GiB cf32 stream in one process: cfg3''s chain (shift -> 200-tap FIR decimate 32 -> W = S = 128) and the cfg3 shape
(400 taps, W 64, S 16).  Legs, 12 steps each, alternating, each timed with HIP events:
  run         qd_plan_run of the norms plan into a device buffer          (one norms-sink pass)
  pool=P      qd_plan_pool into device rows at P = 1, 64, n / 2048 and n  (yardstick)
  mean=P      qd_plan_mean into device rows at the same P
A mean leg does strictly more work per value than a pool leg (an exponent split and two 64-bit adds against two compares, three outputs
against two): it is expected to be slower; by how much is what this measures.
usage: python scripts/bench_mean.py [log2 samples, default 31] [log path, default profiles/r07/mean_sink.log]"""
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
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r07", "mean_sink.log")
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
    pools = sorted({1, 64, max(nw // 2048, 1), nw})
    legs = {"run": lambda: p.run_device(src, out)}
    for P in pools:
        legs[f"pool={P}"] = lambda P=P: p.pool(src, P)
        legs[f"mean={P}"] = lambda P=P: p.mean(src, P)
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
    # the legs agree with each other: pool = 1 is the norms, and every pool counts and sums the same values
    one, all_ = last["mean=1"], last[f"mean={nw}"]
    same = bool(((one[0] == out) | out.isnan()).all()) and bool((one[2] == (~out.isnan())).all())
    same = same and bool((all_[2][0] == one[2].sum(dim=0)).all())
    mid = last[f"mean={pools[1]}"]
    same = same and bool((mid[2].sum(dim=0) == all_[2][0]).all())
    say(f"{cname}: consistent {same}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    run = statistics.median(ms["run"])
    for P in pools:
        a, b = ms[f"mean={P}"], ms[f"pool={P}"]
        say(f"{cname}: mean / pool at {P} = {statistics.median(a) / statistics.median(b):.3f} (medians; {min(a) / max(b):.3f} - {max(a) / min(b):.3f} over the "
            f"repetitions); mean - pool = {statistics.median(a) - statistics.median(b):+.3f} ms, one norms-sink pass {run:.3f} ms -> "
            f"{'within' if statistics.median(a) - statistics.median(b) <= run else 'MORE than'} pool plus one pass")
    p.close()
    del out, last, one, all_, mid
