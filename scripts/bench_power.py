"""Development: the RMS-trace rows' rate (qd_plan_power) against the average-trace rows (qd_plan_mean, section
3.13, whose kernels this work does not touch: its leg is the parent commit's) on the same plan and pool in the same run, on one
device-resident 16 GiB cf32 stream in one process: cfg3''s chain (shift -> 200-tap FIR decimate 32 -> W = S = 128) and the cfg3 shape
(400 taps, W 64, S 16); and, for the widths at the ends of the range, bare FFT plans of W = 4 and W = 2048 on the first 2 GiB.  Legs, 12 steps each, alternating, each timed with HIP events:
  run          qd_plan_run of the norms plan into a device buffer          (one norms-sink pass)
  mean=P       qd_plan_mean into device rows at P = 1, 64, n / 2048 and n  (yardstick)
  power1=P     qd_plan_power at the same P (k_power<1>, the shipped form)
  power4=P     ... with k_power<4>: development library only (python quadrs_amd/build.py --dev;
               QD_LIB_PATH=quadrs_amd/libquadrs_hip_dev.so), which reads QD_POWER_V at every call
A power leg adds three limbs a value over eighteen where a mean leg adds two over nine: it is expected to be the dearer; by how much is
what this measures, for each form of the kernel.
usage: python scripts/bench_power.py [log2 samples, default 31] [log path, default profiles/r10/power_sink.log]"""
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
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r10", "power_sink.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
log = open(log_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


# (name, chain, samples): the two chains on the whole stream; two bare FFT plans at the ends of the width range on its first eighth
CHAINS = (("cfg3p", dict(shift_hz=280000, lowpass=(200_000, 32, 200), width=128, stride=128), n),
          ("cfg3_shape", dict(shift_hz=280000, lowpass=(200_000, 32, 400), width=64, stride=16), n),
          ("plain_w4", dict(width=4, stride=4), n >> 3),
          ("plain_w2048", dict(width=2048, stride=2048), n >> 3))
STEPS = 12
FORMS = ("4", "1") if "dev" in os.path.basename(os.environ.get("QD_LIB_PATH", "")) else ("1",)
say(f"# {n} cf32 samples ({n * 8 / 2**30:.0f} GiB), {STEPS} steps per leg, alternating; ms per step (HIP events)")
whole = src
for cname, chain, ns in CHAINS:
    src = whole.view(-1)[:whole.numel() // (n // ns)]
    p = Q.Plan(0, 21_000_000, ns, **chain)
    nw, W = p.n_windows, chain["width"]
    out = torch.empty(nw, W, dtype=torch.float32, device=dev)
    pools = sorted({1, 64, max(nw // 2048, 1), nw})
    legs = {"run": lambda: p.run_device(src, out)}
    def power(P, form):
        os.environ["QD_POWER_V"] = form                          # the development library reads it at every call
        try:
            return p.power(src, P)
        finally:
            del os.environ["QD_POWER_V"]
    for P in pools:
        legs[f"mean={P}"] = lambda P=P: p.mean(src, P)
        for form in FORMS:
            legs[f"power{form}={P}"] = lambda P=P, form=form: power(P, form)
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
    # the legs agree with each other: pool = 1 is the norms, both forms give the same bytes, and every pool counts the same values
    one, all_ = last["power1=1"], last[f"power1={nw}"]
    same = bool(((one[0] == out) | out.isnan()).all()) and bool((one[2] == (~out.isnan())).all())
    same = same and bool((all_[2][0] == one[2].sum(dim=0)).all())
    for P in pools:
        x, y, m = last[f"power1={P}"], last[f"power{FORMS[0]}={P}"], last[f"mean={P}"]
        same = same and all(bool((x[i].view(torch.int32 if i != 1 else torch.int64) == y[i].view(torch.int32 if i != 1 else torch.int64)).all()) for i in range(3))
        same = same and bool((x[2] == m[2]).all()) and bool(((m[0] <= x[0]) | m[0].isnan()).all())
    say(f"{cname}: consistent {same}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    run = statistics.median(ms["run"])
    for P in pools:
        for form in FORMS:
            a, b = ms[f"power{form}={P}"], ms[f"mean={P}"]
            say(f"{cname}: power{form} / mean at {P} = {statistics.median(a) / statistics.median(b):.3f} (medians; {min(a) / max(b):.3f} - {max(a) / min(b):.3f} over the "
                f"repetitions); power{form} - mean = {statistics.median(a) - statistics.median(b):+.3f} ms, one norms-sink pass {run:.3f} ms -> "
                f"{'within' if statistics.median(a) - statistics.median(b) <= run else 'MORE than'} mean plus one pass")
    p.close()
    del out, last, one, all_, x, y, m
