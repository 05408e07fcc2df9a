"""Development: the mark sink's rate against the bucket sink of the same chain (and the glyph sink) on a device-resident 16 GiB cf32
stream, for cfg3''s chain and the lowpass-free W = 128 chain: 12 steps per sink, alternating, each timed with HIP events.
usage: python scripts/mark_sink_rate.py [log2 samples, default 31]   (writes profiles/r06/mark_sink.log)"""
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
os.makedirs(os.path.join(ROOT, "profiles", "r06"), exist_ok=True)
log = open(os.path.join(ROOT, "profiles", "r06", "mark_sink.log"), "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


CHAINS = (("cfg3p", dict(shift_hz=280000, lowpass=(200_000, 32, 200))), ("nolp_w128", {}))
SINKS = ((Q.EPI_MARK_U8, "mark"), (Q.EPI_BUCKET2_U8, "bucket"), (Q.EPI_GLYPH_U8, "glyph"))
STEPS = 12
say(f"# {n} cf32 samples ({n * 8 / 2**30:.0f} GiB), W = 128, {STEPS} steps per sink, alternating; ms per step (HIP events)")
for cname, chain in CHAINS:
    plans, outs, ms = {}, {}, {}
    for epi, name in SINKS:
        p = Q.Plan(0, 21_000_000, n, width=128, stride=128, epilogue=epi, rng=(0.01, 0.5), **chain)
        plans[name] = p
        outs[name] = torch.empty(p.n_windows * p.info.out_bytes_per_window, dtype=torch.uint8, device=dev)
        ms[name] = []
        for _ in range(2):
            p.run_device(src, outs[name])
        torch.cuda.synchronize()
    for _ in range(STEPS):
        for _, name in SINKS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            plans[name].run_device(src, outs[name])
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    for _, name in SINKS:
        v = ms[name]
        say(f"{cname} {name}: {plans[name].kernel_name()[:70]}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    spread = max(ms["bucket"]) - min(ms["bucket"])
    delta = statistics.median(ms["mark"]) - statistics.median(ms["bucket"])
    say(f"{cname}: mark - bucket = {delta:+.3f} ms (medians); bucket's min-to-max spread {spread:.3f} ms -> {'within' if delta <= spread else 'SLOWER than'} the yardstick")
    for p in plans.values():
        p.close()
    del outs
