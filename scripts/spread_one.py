"""Development: one call each of qd_plan_spread (all five outputs), qd_plan_power and qd_plan_mean at pool = 1 and pool = n on
the cfg3 shape (W 64, S 16) over a device-resident cf32 stream — the workload scripts/spread_counters.sh collects counters over.
usage: python scripts/spread_one.py [log2 samples, default 31]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import quadrs_amd as Q

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 31)
src = bench.synth_slab(torch, 0, 0, n, 0x5EED0002, torch.device("cuda", 0))
p = Q.Plan(0, 21_000_000, n, shift_hz=280000, lowpass=(200_000, 32, 400), width=64, stride=16)
for P in (1, p.n_windows):
    for call in (lambda: p.spread(src, P), lambda: p.power(src, P), lambda: p.mean(src, P)):
        r = call()
        torch.cuda.synchronize()
        del r
print(f"spread_one: {p.n_windows} windows of 64")
p.close()
