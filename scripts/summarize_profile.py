"""Turns a scripts/profile_round.sh output directory into the small files kept under profiles/."""
import collections, csv, glob, json, os, sys

out, tag = sys.argv[1], sys.argv[2]
args = sys.argv[3:]
workload = "cfg3p"
if "--workload" in args:
    workload = args[args.index("--workload") + 1]
res = {"tag": tag, "workload": workload, "bench_args": args}
ks = glob.glob(f"{out}/kt/*/*kernel_stats.csv")
rows = list(csv.DictReader(open(ks[0])))
chain = [r for r in rows if "k_chain" in r["Name"] or "k_spark" in r["Name"] or "k_cascade" in r["Name"]]
# a run may launch a second, tiny chain kernel for windows at an unaligned slab end: the profiled kernel is the one with the most time
chain.sort(key=lambda r: -float(r["AverageNs"]) * float(r["Calls"]))
main_name = chain[0]["Name"] if chain else ""
res["kernel_stats"] = [{k: r[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs", "Percentage")} for r in chain]
# kernel_stats.csv averages every launch of the process, including bench.py's settle phase (isolated launches, each
# followed by a synchronize, run a few % faster than back-to-back ones).  The timed region is the last 40 launches of
# the kernel trace: their durations are what bench.py's roofline.kernel_ms must agree with.
kt = glob.glob(f"{out}/kt/*/*kernel_trace.csv")
if kt:
    tr = [r for r in csv.DictReader(open(kt[0])) if r["Kernel_Name"] == main_name]
    tr.sort(key=lambda r: int(r["Start_Timestamp"]))
    tr = tr[-40:]
    dur = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in tr]
    gap = [int(tr[i + 1]["Start_Timestamp"]) - int(tr[i]["End_Timestamp"]) for i in range(len(tr) - 1)]
    res["timed_region"] = {"launches": len(tr), "kernel_avg_ns": sum(dur) / len(dur), "kernel_min_ns": min(dur),
                           "gap_avg_ns": sum(gap) / max(1, len(gap)), "period_avg_ns": (sum(dur) + sum(gap)) / len(dur)}
pmc = {}
for d in ("fetch", "write", "sq", "sq2"):
    f = glob.glob(f"{out}/{d}/*/*counter_collection.csv")
    if not f:
        continue
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f[0])):
        if r["Kernel_Name"] == main_name:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k, v in agg.items():
        pmc[k] = sum(v) / len(v)
res["pmc_mean_per_launch"] = pmc
# which kernel this is: the FixedGeo template arguments of the profiled kernel's name (W, S, D, T, G, FIRB, FIRR, PAD, BATCH, FLAGS) —
# scripts/collect_profiles.py refuses to publish traffic for a kernel other than the one bench.py reports for the workload
import re
m = re.search(r"FixedGeo<([0-9u, ]+)>", chain[0]["Name"]) if chain else None
if m:
    geo = [int(v.strip().rstrip("u")) for v in m.group(1).split(",")]
    res["kernel_identity"] = {"geo": geo, "flags": geo[9] if len(geo) > 9 else 0, "pipe": "k_chain_pipe" in chain[0]["Name"]}
# MI355X_MICROARCH.md §HBM: FETCH_SIZE (KiB) reports exactly half of a 16 B/lane streaming read on gfx950
# -> double it; WRITE_SIZE (KiB) is exact for 16 B/lane... our 4 B/lane output stores are a small term.
if "FETCH_SIZE" in pmc and "WRITE_SIZE" in pmc:
    res["hbm_bytes_per_launch"] = 2 * pmc["FETCH_SIZE"] * 1024 + pmc["WRITE_SIZE"] * 1024
    res["hbm_note"] = "2*FETCH_SIZE*1024 + WRITE_SIZE*1024 (gfx950 correction for wide coalesced reads)"
summ = os.path.join(os.path.dirname(os.path.abspath(out)), "profiles_out")       # beside the run's own directory
os.makedirs(summ, exist_ok=True)
json.dump(res, open(f"{summ}/{tag}.json", "w"), indent=1)
with open(f"{summ}/{tag}_kernel_stats.csv", "w") as f:
    f.write(open(ks[0]).read())
print(json.dumps(res, indent=1)[:1500])
