"""Development: the emission list's rate (qd_plan_emissions) against one norms-sink pass and the burst list at the
same threshold, on the same plan in the same run, on one device-resident cf32 stream in one process: cfg3''s chain (shift -> 200-tap FIR
decimate 32 -> W = S = 128) and the cfg3 shape (400 taps, W 64, S 16).  Legs, 8 steps each, alternating, each timed with HIP events:
  run               qd_plan_run of the norms plan into a device buffer          (one norms-sink pass)
  bursts=median     qd_plan_bursts at the per-bin median                        (code this sink does not touch, like run)
  emissions=inf     qd_plan_emissions with every threshold +inf: nothing is on, the cost is that of the passes alone
  emissions=q99     ... at the 0.99 quantile of the norms as one level: sparse emissions
  emissions=median  ... at the per-bin median: about half the cells on, near the percolation threshold, the labelling's hard case
  emissions=0       ... at threshold 0: one emission holds every cell, the contention case of the record fold
The lists are device memory.  usage: python scripts/bench_emissions.py [log2 samples, default 31] [log path, default
emissions_sink.log in the next free profiles/rNN]"""
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


def next_free_round():
    """profiles/rNN of the first NN that does not exist yet: a run never overwrites a committed log"""
    nn = 1
    while os.path.exists(os.path.join(ROOT, "profiles", "r%02d" % nn)):
        nn += 1
    return os.path.join(ROOT, "profiles", "r%02d" % nn)


log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(next_free_round(), "emissions_sink.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
log = open(log_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


CHAINS = (("cfg3p", dict(shift_hz=280000, lowpass=(200_000, 32, 200), width=128, stride=128)),
          ("cfg3_shape", dict(shift_hz=280000, lowpass=(200_000, 32, 400), width=64, stride=16)))
STEPS = 8
CAP = 1 << 20
say(f"# {n} cf32 samples ({n * 8 / 2**30:.0f} GiB), {STEPS} steps per leg, alternating; ms per step (HIP events); cap {CAP} records")
for cname, chain in CHAINS:
    p = Q.Plan(0, 21_000_000, n, **chain)
    nw, W = p.n_windows, chain["width"]
    out = torch.empty(nw, W, dtype=torch.float32, device=dev)
    p.run_device(src, out)
    torch.cuda.synchronize()
    part = out[:: max(nw // 65536, 1)][:65536].float().cpu().numpy()                 # thresholds from a sample of the windows
    q99 = np.full(W, np.nanquantile(part.astype(np.float64), 0.99), dtype=np.float32)
    median = np.nanmedian(part, axis=0).astype(np.float32)
    thr = {"emissions=inf": np.full(W, np.inf, dtype=np.float32), "emissions=q99": q99, "emissions=median": median,
           "emissions=0": np.zeros(W, dtype=np.float32)}
    lst = torch.empty(CAP * 56, dtype=torch.uint8, device=dev)
    blst = torch.empty(CAP * 32, dtype=torch.uint8, device=dev)
    cnt = torch.empty(W, dtype=torch.int64, device=dev)
    legs = {"run": lambda: p.run_device(src, out), "bursts=median": lambda: p.bursts(src, median, 1, CAP, out=blst, counts_out=cnt)}
    for k, t in thr.items():
        legs[k] = lambda t=t: p.emissions(src, t, 1, 1, CAP, out=lst)
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
    # the legs agree with the norms: the cells of the listed emissions are on cells, all of them while the list has room
    for k, t in thr.items():
        rec, found = legs[k]()
        torch.cuda.synchronize()
        on = int((out >= torch.from_numpy(t).to(dev)).sum())
        cells = int(rec.cpu().numpy().reshape(-1).view(Q.EMISSION_DTYPE)["cells"].sum())
        say(f"{cname} {k}: found {found}, listed {rec.shape[0]}, their cells {cells}, on cells {on} of {nw * W}; consistent {cells == on if found <= CAP else cells <= on}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    run, bur = statistics.median(ms["run"]), statistics.median(ms["bursts=median"])
    for k in thr:
        a = statistics.median(ms[k])
        say(f"{cname}: {k} / run = {a / run:.2f}, / bursts=median = {a / bur:.2f}; above one pass {a - run:+.3f} ms (bursts=median: {bur - run:+.3f} ms)")
    a, b = statistics.median(ms["emissions=0"]), statistics.median(ms["emissions=median"])
    say(f"{cname}: emissions=0 / emissions=median = {a / b:.2f}")
    p.close()
    del out, last, lst, blst, cnt
