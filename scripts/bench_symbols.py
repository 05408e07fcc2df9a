"""Symbol list against what the library offered before it, on a device-resident stream.  Not part of bench.py.

The cuts of scripts/bench_cuts.py (64 and 1024 cuts over a 1 GiB cf32 stream at 21 MHz, D = 32, T = 256, counts 2^12 ... 2^16 in turn), and
behind them the bucket sink at W = 64, S = 64 and the mark sink at W = 64, S = 16:
  one call   qd_cuts_symbols, device source, device output: the IQ stays in the device workspace;
  sink only  qd_symbols_run alone over the cuts' IQ already in device memory (a qd_cuts_run output), device output;
  per cut    what the library offered before: qd_cuts_run to the host, then one plan of the sink created, run from the host and destroyed
             per cut.
Every path returns after the device is done.  Prints the median and the spread (min ... max) of --reps timed calls after a warm-up, the
PCIe bytes of the one-call and the per-cut path, and that the two give the same bytes; appends the lines to --log.  The kernels' shares
come from a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_symbols.py --only 1024 --sink bucket
No ratio is fixed in advance."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
os.environ.setdefault("QUADRS_AMD_HARNESS_ENV", "0")

from bench_cuts import D, N, SR, T, make_cuts  # noqa: E402

SINKS = {"bucket": (64, 64), "mark": (64, 16)}


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", type=int, default=0, help="run just the one-call path on this many cuts (for a profiler)")
    ap.add_argument("--sink", default="", help="bucket | mark (default: both)")
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
    for n in ([a.only] if a.only else [64, 1024]):
        cuts = make_cuts(Q, n)
        coffs, _, _ = Q.cuts_geometry(SR, N, cuts)
        total_iq = int(coffs[-1])
        segs = np.zeros(n, dtype=Q.SEGMENT_DTYPE)
        segs["first"], segs["count"] = coffs[:-1], cuts["count"]
        for name in ([a.sink] if a.sink else ["bucket", "mark"]):
            W, S = SINKS[name]
            epi = Q.EPI_BUCKET2_U8 if name == "bucket" else Q.EPI_MARK_U8
            desc = Q.symbols_desc(epi, W, S)
            offs = Q.symbols_geometry(desc, segs)
            total = int(offs[-1])
            out = torch.empty(total, dtype=torch.uint8, device="cuda")
            ms, lo, hi = timed(lambda: Q.cuts_symbols(Q.FMT_CF32, SR, N, src, cuts, desc, out=out), a.reps)
            say(f"cuts={n} sink={name} W={W} S={S} windows={total} iq={total_iq * 8} B one_call_ms={ms:.3f} ({lo:.3f} ... {hi:.3f}) pcie: 0 B of IQ or symbols "
                f"(device out; {total} B down with a host out)")
            if a.only:
                continue
            fused = out.cpu().numpy().copy()
            iq = torch.empty((total_iq, 2), dtype=torch.float32, device="cuda")
            Q.cuts_run(Q.FMT_CF32, SR, N, src, cuts, out=iq)
            ms_s, lo, hi = timed(lambda: Q.symbols_run(desc, iq, segs, out=out), a.reps)
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == fused).all()
            say(f"cuts={n} sink={name} sink_only_ms={ms_s:.3f} ({lo:.3f} ... {hi:.3f}) ({total_iq * 8 / ms_s / 1e6:.1f} GB/s of IQ)")
            got = []

            def per_cut():
                got.clear()
                host = Q.cuts_run(Q.FMT_CF32, SR, N, src, cuts)
                for c, y in zip(cuts, host):
                    plan = Q.Plan(Q.FMT_CF32, SR // D, int(c["count"]), width=W, stride=S, epilogue=epi, kernel_policy=Q.KERNEL_NO_PLAN_TIME)
                    got.append(plan.run_host(y).reshape(-1))
                    plan.close()
            ms_old, lo, hi = timed(per_cut, 1 if n > 64 else min(a.reps, 3))
            same = bool((np.concatenate(got) == fused).all())
            say(f"cuts={n} sink={name} per_cut_ms={ms_old:.3f} ({lo:.3f} ... {hi:.3f}) pcie: {total_iq * 8} B of IQ down, {total_iq * 8} B up again, {total} B of symbols "
                f"down; same bytes: {same}; one_call_is={ms_old / ms:.2f}x")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
