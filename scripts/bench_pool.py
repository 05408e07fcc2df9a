"""Development: the peak-hold rows' rate (qd_plan_pool) against the two calls it sits between, on one
device-resident 16 GiB cf32 stream in one process: cfg3''s chain (shift -> 200-tap FIR decimate 32 -> W = S = 128) and the cfg3 shape
(400 taps, W 64, S 16).  Legs, 12 steps each, alternating, each timed with HIP events:
  run         qd_plan_run of the norms plan into a device buffer          (yardstick)
  summarize   qd_plan_summarize over the same windows                     (yardstick: the same carrier pass, plus a histogram)
  pool=P      qd_plan_pool into device rows at P = 1, 64, n / 2048 and n
Expected: a pool leg is no slower than summarize, within summarize's own min-to-max spread; pool = 1 may cost up to the norms sink's
write on top.
usage: python scripts/bench_pool.py [log2 samples, default 31] [log path, default profiles/r07/pool_sink.log]"""
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
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r07", "pool_sink.log")
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
    legs = {"run": lambda: p.run_device(src, out), "summarize": lambda: p.summarize(src)}
    for P in pools:
        legs[f"pool={P}"] = lambda P=P: p.pool(src, P)
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
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = legs[k]()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    # the legs agree with each other: one row is the summary's arrays, pool = 1 the norms
    s, one, all_ = last["summarize"], last["pool=1"], last[f"pool={nw}"]
    same = all_[0][0].cpu().numpy().tobytes() == s.peak.tobytes() and all_[1][0].cpu().numpy().tobytes() == s.floor.tobytes()
    same = same and bool(((one[0] == out) | out.isnan()).all()) and bool(((one[1] == out) | out.isnan()).all())
    say(f"{cname}: consistent {same}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    spread = max(ms["summarize"]) - min(ms["summarize"])
    for P in pools:
        delta = statistics.median(ms[f"pool={P}"]) - statistics.median(ms["summarize"])
        say(f"{cname}: pool={P} - summarize = {delta:+.3f} ms (medians); summarize's min-to-max spread {spread:.3f} ms -> "
            f"{'within' if delta <= spread else 'SLOWER than'} the yardstick")
    p.close()
    del out, last
