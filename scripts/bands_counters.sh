#!/bin/bash
# development: one counter-only run (no tracing) of k_bands with the window cut into 2, 16 and 64 bands and of k_mean at pool 64 on the cfg3
# shape (scripts/bands_one.py); sums over the launches of each call.  usage: [OUT_DIR=dir] scripts/bands_counters.sh [log2 samples] [log]
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
out=${OUT_DIR:-out}/pmc_bands
log=${2:-profiles/r12/bands_counters.log}
rm -rf $out; mkdir -p $out "$(dirname "$log")"
timeout -k 10 500 rocprofv3 --kernel-include-regex 'k_bands|k_mean' --pmc SQ_INSTS_VALU SQ_INSTS_VMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY GRBM_GUI_ACTIVE \
    --output-format csv -d $out -- python3 scripts/bands_one.py ${1:-31} > $out/run.log 2>&1 || { tail -5 $out/run.log; exit 1; }
python3 - $out "$log" <<'PY'
import csv, glob, sys, collections
out, log = sys.argv[1:3]
acc, order = collections.defaultdict(lambda: collections.defaultdict(float)), []
launches = collections.Counter()
for f in glob.glob(out + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        # one call's launches share a kernel and a grid; the three band calls differ in their grids
        key = (r["Kernel_Name"].split("(")[0], r["Grid_Size"])
        if key not in acc:
            order.append(key)
        acc[key][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Counter_Name"] == "SQ_INSTS_VALU":
            launches[key] += 1
lines = ["# one counter-only run: the cfg3 shape (W 64, S 16), qd_plan_bands (all six outputs) with 2, 16 and 64 equal bands, qd_plan_mean at pool 64",
         "# sums over the launches of a kernel at a grid size; grid in work-items"]
for key in order:
    c = acc[key]
    share = c["SQ_ACTIVE_INST_VALU"] / c["SQ_ACTIVE_INST_ANY"] if c.get("SQ_ACTIVE_INST_ANY") else float("nan")
    wait = c["SQ_WAIT_INST_ANY"] / c["SQ_WAVE_CYCLES"] if c.get("SQ_WAVE_CYCLES") else float("nan")
    lines.append(f"{key[0]} grid {key[1]} launches {launches[key]}: " + " ".join(f"{k} {v:.4g}" for k, v in sorted(c.items())) +
                 f" | VALU share of active {share:.2f}, waiting share of wave cycles {wait:.2f}")
open(log, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
PY
rm -rf $out
