"""Cut list against what the library offered before it, on a device-resident stream.  Not part of bench.py.

64 and 1024 cuts over a 1 GiB cf32 stream at 21 MHz (2^27 samples), D = 32, T = 256, counts 2^12 ... 2^16 in turn, spans spread over the
stream, a different shift per cut:
  one call    all of them in one qd_cuts_run, device source, device output;
  per cut     one QD_EPI_CF32_BLOCKS plan (same shift, same lowpass, blocks of 4096 as `write` uses; no plan-time build) created, run over
              the blocks that cover the cut, and destroyed, per cut: the same samples and the rest of the covering blocks.
Prints both wall times (median of --reps after a warm-up; both paths return after the device is done), the bytes the cuts read and
write, and writes the lines to --log.  The kernels' share of the one-call time comes from a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_cuts.py --only-cuts 1024
No ratio is fixed in advance."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("QUADRS_AMD_HARNESS_ENV", "0")

SR, N, D, T, LP, B = 21_000_000, 1 << 27, 32, 256, 200_000, 4096


def make_cuts(Q, n):
    cuts = np.zeros(n, dtype=Q.CUT_DTYPE)
    room = (N - T) // (B * D) * B                               # the outputs the per-cut plans' full blocks cover
    for k in range(n):
        count = 1 << (12 + k % 5)
        first = (k * 2_654_435_761 % (room - count)) // 64 * 64 + k % 7
        cuts[k] = (100_003 + 997 * k, LP, D, T, min(first, room - count), count)
    return cuts


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-cuts", type=int, default=0, help="run just the one-call path on this many cuts (for a profiler)")
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    import torch
    import quadrs_amd as Q
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    src.normal_(0.0, 0.03, generator=g)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for n in ([a.only_cuts] if a.only_cuts else [64, 1024]):
        cuts = make_cuts(Q, n)
        offs, _, _ = Q.cuts_geometry(SR, N, cuts)
        total = int(offs[-1])
        out = torch.empty((total, 2), dtype=torch.float32, device="cuda")
        read = int((cuts["count"] * D + T).sum()) * 8
        ms = timed(lambda: Q.cuts_run(Q.FMT_CF32, SR, N, src, cuts, out=out), a.reps)
        say(f"cuts={n} D={D} T={T} outputs={total} read={read} B written={total * 8} B one_call_ms={ms:.3f} ({read / ms / 1e6:.1f} GB/s of source)")
        if a.only_cuts:
            continue

        def per_cut():
            for c in cuts:
                first, count = int(c["first"]), int(c["count"])
                b0, b1 = first // B, -(-(first + count) // B)
                plan = Q.Plan(Q.FMT_CF32, SR, N, shift_hz=int(c["shift_hz"]), lowpass=(LP, D, T), width=B, epilogue=Q.EPI_CF32_BLOCKS,
                              kernel_policy=Q.KERNEL_NO_PLAN_TIME)
                blocks = torch.empty(((b1 - b0) * B, 2), dtype=torch.float32, device="cuda")
                plan.run_device(src, blocks, first_window=b0, n_windows=b1 - b0)
                torch.cuda.synchronize()
                plan.close()
        ms_old = timed(per_cut, 1 if n > 64 else a.reps)
        blocks_read = sum((-(-(int(c["first"]) + int(c["count"])) // B) - int(c["first"]) // B) * (B * D) + T for c in cuts) * 8
        say(f"cuts={n} per_cut_plans_ms={ms_old:.3f} (blocks of {B}: {blocks_read} B read) one_call_is={ms_old / ms:.2f}x")
        # the same bytes: a shift-free control is held by tests/test_gpu_cuts.py; here one shifted cut against its plan's blocks
        c = cuts[0]
        first, count = int(c["first"]), int(c["count"])
        b0, b1 = first // B, -(-(first + count) // B)
        plan = Q.Plan(Q.FMT_CF32, SR, N, shift_hz=int(c["shift_hz"]), lowpass=(LP, D, T), width=B, epilogue=Q.EPI_CF32_BLOCKS, kernel_policy=Q.KERNEL_NO_PLAN_TIME)
        blocks = torch.empty(((b1 - b0) * B, 2), dtype=torch.float32, device="cuda")
        plan.run_device(src, blocks, first_window=b0, n_windows=b1 - b0)
        torch.cuda.synchronize()
        mine = out[:count].cpu().numpy()
        theirs = blocks[first - b0 * B:first - b0 * B + count].cpu().numpy()
        inner = slice(0, count - (T - T // 2 + D - 1) // D)        # a cut truncates at ITS end, a block at the block's
        same = float((mine[inner].view(np.uint32) == theirs[inner].view(np.uint32)).mean())
        say(f"cuts={n} cut 0 against its plan's blocks: {same:.6f} of the untruncated components bit-equal")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
