"""Development: the waterfall picture's rate (qd_plan_picture) against the peak-hold rows at pool 1 (qd_plan_pool,
section 3.12, whose code this work does not touch: its leg is the parent commit's) and one norms-sink pass on the same plan in the same
run, on one device-resident cf32 stream in one process: cfg3''s chain (shift -> 200-tap FIR decimate 32 -> W = S = 128) and the cfg3
shape (400 taps, W 64, S 16).  Legs, 12 steps each, alternating, each timed with HIP events:
  run         qd_plan_run of the norms plan into a device buffer             (one norms-sink pass)
  pool=1      qd_plan_pool at pool 1, peak rows only, into device rows       (yardstick: reads the same carrier, writes one word a cell)
  picture s1  qd_plan_picture at stretch 1 into a device picture wide enough that no window is dropped: 3 bytes a cell
  picture s4  ... at stretch 4: 12 bytes a cell
Both folds read every value once; the picture adds the colour map, the transposition through LDS and byte-granular run ends.
usage: python scripts/bench_picture.py [log2 samples, default 31] [log path, default profiles/r13/picture_sink.log]"""
import ctypes as C
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import statistics
import torch
import bench
import quadrs_amd as Q
from quadrs_amd import _ffi

n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 31)
dev = torch.device("cuda", 0)
src = bench.synth_slab(torch, 0, 0, n, 0x5EED0002, dev)
log_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13", "picture_sink.log")
os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
log = open(log_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


CHAINS = (("cfg3p", dict(shift_hz=280000, lowpass=(200_000, 32, 200), width=128, stride=128), 4096),
          ("cfg3_shape", dict(shift_hz=280000, lowpass=(200_000, 32, 400), width=64, stride=16), 8192))
STEPS = 12
SCALE = 0.05                    # the synthetic stream's norms lie well below 2.29: a scale at which the pictures are not black
say(f"# {n} cf32 samples ({n * 8 / 2**30:.0f} GiB), {STEPS} steps per leg, alternating; ms per step (HIP events)")
for cname, chain, w in CHAINS:
    p = Q.Plan(0, 21_000_000, n, **chain)
    nw, W = p.n_windows, chain["width"]
    count = src.numel() * src.element_size() // 8
    out = torch.empty(nw, W, dtype=torch.float32, device=dev)
    peak = torch.empty(nw, W, dtype=torch.float32, device=dev)
    strips = -(-nw // w)
    descs = {k: Q.picture_desc(w, strips * (k * W + 16), k, 0, SCALE) for k in (1, 4)}
    pics = {k: torch.empty(d.px_height, w, 3, dtype=torch.uint8, device=dev) for k, d in descs.items()}
    for k, d in descs.items():
        assert Q.picture_geometry(d, W)[1] >= nw

    def pool1():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _ffi.check(_ffi.lib().qd_plan_pool(p._h, C.c_void_p(src.data_ptr()), _ffi.MEM_DEVICE, 0, count, 0, nw, 1, C.c_void_p(peak.data_ptr()), None,
                                           _ffi.MEM_DEVICE, st))

    legs = {"run": lambda: p.run_device(src, out), "pool=1": pool1}
    for k in descs:
        legs[f"picture s{k}"] = lambda k=k: p.picture(src, descs[k], out=pics[k])
    say(f"{cname}: {nw} windows of {W}, norms {nw * W * 4 / 2**20:.0f} MiB, page width {w}, pictures "
        + ", ".join(f"{pics[k].numel() / 2**20:.0f} MiB" for k in descs) + f", {p.kernel_name()[:70]}")
    for _ in range(2):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    order = list(legs)
    for i in range(STEPS):
        for k in (order if i % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            legs[k]()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    # the legs agree with each other: pool 1 gives the norms, and the stretch-4 picture is the stretch-1 picture with every bin row four times
    same = bool(((peak == out) | out.isnan()).all())
    a = pics[1].flip(0).reshape(strips, W + 16, w, 3)[:, :W]
    b = pics[4].flip(0).reshape(strips, 4 * W + 16, w, 3)[:, :4 * W].reshape(strips, W, 4, w, 3)
    same = same and bool((b == a[:, :, None]).all()) and bool(a.any())
    say(f"{cname}: consistent {same}")
    for k in order:
        v = ms[k]
        say(f"{cname} {k}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    run, pool = statistics.median(ms["run"]), statistics.median(ms["pool=1"])
    for k in descs:
        t = statistics.median(ms[f"picture s{k}"])
        say(f"{cname}: picture s{k} - run = {t - run:+.3f} ms, pool=1 - run = {pool - run:+.3f} ms, ratio {(t - run) / (pool - run):.2f}"
            + (f" -> {'within' if t - run <= 2 * (pool - run) else 'OUTSIDE'} 2x of the pool's time above one pass" if k == 1 else ""))
    p.close()
    del out, peak, pics, a, b
