#!/bin/bash
# Copy one GPU round's evidence from tools/profile_round.sh's output directory
# (scratch, $OUT, default profile_out/) into profiles/ (tracked).
# Usage: [OUT=dir] bash tools/save_profiles.sh TAG
set -e
TAG=$1
OUT=${OUT:-profile_out}
grep '^{' $OUT/${TAG}_bench.log | tail -1 > profiles/${TAG}_bench.json
cp $OUT/${TAG}_trace/bench_kernel_stats.csv profiles/${TAG}_kernel_stats.csv
cp $OUT/${TAG}_pmc/summary.json profiles/${TAG}_pmc_summary.json
cp $OUT/${TAG}_pmc.log profiles/${TAG}_pmc_table.txt
cp $OUT/${TAG}_pmc/pmc_traffic.json profiles/pmc_traffic.json
if [ -d $OUT/${TAG}_pmcbf16 ]; then
  cp $OUT/${TAG}_pmcbf16/summary.json profiles/${TAG}_bf16_pmc_summary.json
  cp $OUT/${TAG}_pmcbf16.log profiles/${TAG}_bf16_pmc_table.txt
  cp $OUT/${TAG}_pmcbf16/pmc_traffic.json profiles/pmc_traffic_bf16.json
fi
if [ -d $OUT/${TAG}_pmcinfer ]; then
  cp $OUT/${TAG}_pmcinfer/summary.json profiles/${TAG}_bf16_infer_pmc_summary.json
  cp $OUT/${TAG}_pmcinfer/pmc_traffic.json profiles/pmc_traffic_bf16_infer.json
fi
[ -f $OUT/${TAG}_gputests.log ] && cp $OUT/${TAG}_gputests.log profiles/${TAG}_gputests.log
true
