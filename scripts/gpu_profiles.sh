#!/bin/bash
# rocprofv3 evidence for the round: kernel trace + PMC passes per workload (scripts/profile_round.sh), then the summaries
# usage: [OUT_DIR=dir] scripts/gpu_profiles.sh [round tag, default r04] [workloads...]   (logs under $OUT_DIR, default out/)
rnd=${1:-r04}; shift || true
wls=${@:-cfg3p cfg2 cfg3 cfg4}
export OUT_DIR=${OUT_DIR:-out}
mkdir -p $OUT_DIR
rm -rf $OUT_DIR/profiles_out
for wl in $wls; do
  timeout -k 10 500 bash scripts/profile_round.sh ${rnd}_$wl --workload $wl > $OUT_DIR/prof_${rnd}_$wl.txt 2>&1; echo "$wl rc=$?"
  if [ $? -ge 124 ]; then exit 1; fi
done
if [ -z "$NO_DEFAULT_BENCH" ]; then timeout -k 10 600 python bench.py --full > $OUT_DIR/profiles_out/${rnd}_bench_default.json 2> $OUT_DIR/${rnd}_bench_default.err; echo "bench rc=$?"; fi
for wl in $wls; do
  [ $wl = cfg3p ] && continue
  timeout -k 10 300 python bench.py --full --workload $wl --no-others > $OUT_DIR/profiles_out/${rnd}_bench_$wl.json 2>/dev/null; echo "bench $wl rc=$?"
done
ls -la $OUT_DIR/profiles_out
