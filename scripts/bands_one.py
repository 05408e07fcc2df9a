"""Development: one call each of qd_plan_bands (all six outputs) with the window cut into 2, 16 and W equal bands, and of qd_plan_mean at
pool 64, on the cfg3 shape (W 64, S 16) over a device-resident cf32 stream — the workload scripts/bands_counters.sh collects counters
over.  usage: python scripts/bands_one.py [log2 samples, default 31]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import quadrs_amd as Q

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 31)
src = bench.synth_slab(torch, 0, 0, n, 0x5EED0002, torch.device("cuda", 0))
W = 64
p = Q.Plan(0, 21_000_000, n, shift_hz=280000, lowpass=(200_000, 32, 400), width=W, stride=16)
for K in (2, 16, W):
    r = p.bands(src, [(k * W // K, (k + 1) * W // K) for k in range(K)])
    torch.cuda.synchronize()
    del r
r = p.mean(src, 64)
torch.cuda.synchronize()
del r
print(f"bands_one: {p.n_windows} windows of {W}")
p.close()
