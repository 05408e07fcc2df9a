"""Development: the deviation-trace rows' rate (qd_plan_spread) against the average-trace rows (qd_plan_mean,
section 3.13) and the RMS-trace rows (qd_plan_power, section 3.17), whose kernels this work does not touch: their legs are the parent
commit's, on the same plan and pool in the same run, on one device-resident 16 GiB cf32 stream in one process: cfg3''s chain (shift ->
200-tap FIR decimate 32 -> W = S = 128) and the cfg3 shape (400 taps, W 64, S 16); and, for the widths at the ends of the range, bare FFT
plans of W = 4 and W = 2048 on the first 2 GiB.  Legs, 12 steps each, alternating, each timed with HIP events:
  run          qd_plan_run of the norms plan into a device buffer          (one norms-sink pass)
  mean=P       qd_plan_mean into device rows at P = 1, 64, n / 2048 and n  (yardstick)
  power=P      qd_plan_power at the same P                                 (yardstick)
  std=P        qd_plan_spread with std_rows alone
  all=P        qd_plan_spread with all five outputs
Reported per chain and pool: all against mean + power together (one pass for what a caller now pays two for), and std against power.
usage: python scripts/bench_spread.py [log2 samples, default 31] [log path, default profiles/r11/spread_sink.log]"""
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
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r11", "spread_sink.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
log = open(log_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# (name, chain, samples): the two chains on the whole stream; two bare FFT plans at the ends of the width range on its first eighth
CHAINS = (("cfg3p", dict(shift_hz=280000, lowpass=(200_000, 32, 200), width=128, stride=128), n),
          ("cfg3_shape", dict(shift_hz=280000, lowpass=(200_000, 32, 400), width=64, stride=16), n),
          ("plain_w4", dict(width=4, stride=4), n >> 3),
          ("plain_w2048", dict(width=2048, stride=2048), n >> 3))
STEPS = 12
say(f"# {n} cf32 samples ({n * 8 / 2**30:.0f} GiB), {STEPS} steps per leg, alternating; ms per step (HIP events)")
whole = src
for cname, chain, ns in CHAINS:
    src = whole.view(-1)[:whole.numel() // (n // ns)]
    p = Q.Plan(0, 21_000_000, ns, **chain)
    nw, W = p.n_windows, chain["width"]
    out = torch.empty(nw, W, dtype=torch.float32, device=dev)
    pools = sorted({1, 64, max(nw // 2048, 1), nw})
    legs = {"run": lambda: p.run_device(src, out)}
    for P in pools:
        legs[f"mean={P}"] = lambda P=P: p.mean(src, P)
        legs[f"power={P}"] = lambda P=P: p.power(src, P)
        legs[f"std={P}"] = lambda P=P: p.spread(src, P, outputs=("std",))
        legs[f"all={P}"] = lambda P=P: p.spread(src, P)
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
    # the legs agree with each other: the five-output leg's mean, rms and count are the yardsticks' bits, std alone is its std, the
    # deviation never passes the rms, and pool = 1 has none
    same = True
    for P in pools:
        a, s, m, q = last[f"all={P}"], last[f"std={P}"], last[f"mean={P}"], last[f"power={P}"]
        same = same and bool((bits(a[3]) == bits(m[0])).all()) and bool((bits(a[4]) == bits(q[0])).all()) and bool((a[2] == m[2]).all())
        same = same and bool((bits(a[0]) == bits(s[0])).all()) and bool(((a[0] <= a[4]) | a[0].isnan()).all())
    one = last["all=1"]
    same = same and bool(((bits(one[0]) == 0) | one[0].isnan()).all()) and bool((one[1][~one[1].isnan()] == 0).all())
    say(f"{cname}: consistent {same}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    med = {k: statistics.median(v) for k, v in ms.items()}
    for P in pools:
        both = med[f"mean={P}"] + med[f"power={P}"]
        say(f"{cname}: all / (mean + power) at {P} = {med[f'all={P}'] / both:.3f} (medians; all {med[f'all={P}']:.3f} ms against {both:.3f} ms: "
            f"{'within' if med[f'all={P}'] <= both else 'MORE than'} the two calls); std / power = {med[f'std={P}'] / med[f'power={P}']:.3f} "
            f"({min(ms[f'std={P}']) / max(ms[f'power={P}']):.3f} - {max(ms[f'std={P}']) / min(ms[f'power={P}']):.3f} over the repetitions)")
    p.close()
    del out, last, one, a, s, m, q
