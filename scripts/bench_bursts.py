"""Development: the burst list's rate (qd_plan_bursts) against the average-trace rows at pool 64 (qd_plan_mean),
the band traces cut in two (qd_plan_bands) and one norms-sink pass on the same plan in the same run, on one device-resident cf32 stream
in one process: cfg3''s chain (shift -> 200-tap FIR decimate 32 -> W = S = 128) and the cfg3 shape (400 taps, W 64, S 16).  Legs, 8
steps each, alternating, each timed with HIP events:
  run           qd_plan_run of the norms plan into a device buffer           (one norms-sink pass)
  mean=64       qd_plan_mean into device rows at pool 64
  bands=2       qd_plan_bands, the window cut into 2 equal bands
  bursts=inf    qd_plan_bursts with every threshold +inf: nothing is on, the cost is that of the passes alone
  bursts=q99    ... at the 0.99 quantile of the norms as one level: sparse bursts
  bursts=median ... at the per-bin median: most bins flicker; the list holds the first 2^20 records
The list and on_counts are device memory.  usage: python scripts/bench_bursts.py [log2 samples, default 31] [log path, default
bursts_sink.log in the next free profiles/rNN]"""
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


log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(next_free_round(), "bursts_sink.log")
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
    thr = {"bursts=inf": np.full(W, np.inf, dtype=np.float32), "bursts=q99": q99, "bursts=median": median}
    lst = torch.empty(CAP * 32, dtype=torch.uint8, device=dev)
    cnt = torch.empty(W, dtype=torch.int64, device=dev)
    legs = {"run": lambda: p.run_device(src, out), "mean=64": lambda: p.mean(src, 64),
            "bands=2": lambda: p.bands(src, [(0, W // 2), (W // 2, W)])}
    for k, t in thr.items():
        legs[k] = lambda t=t: p.bursts(src, t, 1, CAP, out=lst, counts_out=cnt)
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
    # the legs agree with the norms: on_counts is the count of cells at or above the threshold
    same = True
    for k, t in thr.items():
        _, found, counts = legs[k]()
        torch.cuda.synchronize()
        want = (out >= torch.from_numpy(t).to(dev)).sum(dim=0)
        same = same and bool((counts == want).all())
        say(f"{cname} {k}: found {found}, on cells {int(counts.sum())} of {nw * W}")
    say(f"{cname}: consistent {same}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    run, mean = statistics.median(ms["run"]), statistics.median(ms["mean=64"])
    for k in thr:
        a = statistics.median(ms[k])
        say(f"{cname}: {k} / run = {a / run:.2f}, / mean=64 = {a / mean:.2f}; above one pass {a - run:+.3f} ms (mean=64: {mean - run:+.3f} ms)")
    p.close()
    del out, last, lst, cnt
