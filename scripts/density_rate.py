"""Development: the level counts' rate (qd_plan_density) against qd_plan_pool on the same plan, source and pool, on
one device-resident cf32 stream in one process: cfg3''s chain (shift -> 200-tap FIR decimate 32 -> W = S = 128).  Both read the same
carrier once behind the same norms kernel, so the difference is the fold kernel alone.  Legs, 12 steps each, alternating, each timed
with HIP events:
  run                 qd_plan_run of the norms plan into a device buffer   (one norms-sink pass)
  pool=512            qd_plan_pool into device rows                        (yardstick: the parent's code)
  density L=64        qd_plan_density, counts in device rows, pool 512, 64 levels around the median bucket
  density L=256       the hard case: 64 columns a workgroup, four lanes a column
  density L=64 +q     the same with the 0.5 and 0.9 traces (k_density_quantile behind the fold)
usage: python scripts/density_rate.py [log2 samples, default 31] [log path, default profiles/r09/density.log]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import statistics
import numpy as np
import torch
import bench
import quadrs_amd as Q

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 31)
dev = torch.device("cuda", 0)
src = bench.synth_slab(torch, 0, 0, n, 0x5EED0002, dev)
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r09", "density.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
log = open(log_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


POOL, STEPS = 512, 12
chain = dict(shift_hz=280000, lowpass=(200_000, 32, 200), width=128, stride=128)
p = Q.Plan(0, 21_000_000, n, **chain)
nw, W = p.n_windows, chain["width"]
out = torch.empty(nw, W, dtype=torch.float32, device=dev)
s = p.summarize(src)
lo, _ = s.quantile(0.5)
mid = int(np.array([lo], np.float32).view(np.uint32)[0]) >> 20
grids = {64: min(max(mid - 32, 0), 2041 - 64), 256: min(max(mid - 128, 0), 2041 - 256)}
say(f"# {n} cf32 samples ({n * 8 / 2**30:.2f} GiB), {nw} windows of {W}, norms {nw * W * 4 / 2**20:.0f} MiB, pool {POOL}, median bucket {mid}; "
    f"{STEPS} steps per leg, alternating; ms per step (HIP events); {p.kernel_name()[:70]}")
legs = {
    "run": lambda: p.run_device(src, out),
    f"pool={POOL}": lambda: p.pool(src, POOL),
    "density L=64": lambda: p.density(src, POOL, grids[64], 64),
    "density L=256": lambda: p.density(src, POOL, grids[256], 256),
    "density L=64 +q": lambda: p.density(src, POOL, grids[64], 64, q=(0.5, 0.9)),
}
last = {}
for _ in range(2):
    for k, f in legs.items():
        last[k] = f()
torch.cuda.synchronize()
ms = {k: [] for k in legs}
order = list(legs)
for i in range(STEPS):
    for k in (order if i % 2 == 0 else order[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        last[k] = legs[k]()
        e1.record()
        torch.cuda.synchronize()
        ms[k].append(e0.elapsed_time(e1))
# the legs agree with each other: every window is counted once at either L, and the 64 levels are the 256 with the ends folded in
c64, c256 = last["density L=64"][0].long(), last["density L=256"][0].long()
rows = c64.shape[0]
per_row = torch.full((rows,), POOL, device=dev)
per_row[-1] = nw - (rows - 1) * POOL
a = grids[64] - grids[256]
folded = torch.cat([c256[:, :, :a + 1].sum(2, keepdim=True), c256[:, :, a + 1:a + 63], c256[:, :, a + 63:].sum(2, keepdim=True)], 2)
nan = int(out.isnan().sum())
same = bool((c64.sum(2) <= per_row[:, None]).all()) and int((per_row.sum() * W - c64.sum())) == nan and bool((folded == c64).all())
same = same and bool((last["density L=64 +q"][0].long() == c64).all())
say(f"consistent {same} ({nan} NaN norms)")
for k in order:
    v = ms[k]
    say(f"{k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
base = statistics.median(ms[f"pool={POOL}"])
spread = max(ms[f"pool={POOL}"]) - min(ms[f"pool={POOL}"])
for k in order[2:]:
    d = statistics.median(ms[k]) - base
    say(f"{k} - pool = {d:+.3f} ms (medians), x{statistics.median(ms[k]) / base:.3f}; pool's min-to-max spread {spread:.3f} ms")
p.close()
