#!/bin/bash
# One round's GPU evidence (run on the GPU box from the repo root):
#   1. rocprofv3 --kernel-trace --stats over the bench command
#   2. PMC passes (tools/pmc_profile.sh) -> per-launch HBM traffic, fp32-parity
#      and bf16 modes (profiles/pmc_traffic.json, profiles/pmc_traffic_bf16.json)
#   3. the full bench line (bench.py --full, with the CPU baseline), roofline.traffic filled
# Usage: [OUT=dir] bash tools/profile_round.sh TAG   (outputs under $OUT/TAG_*, default profile_out/)
set -e
TAG=${1:-r02}
OUT=${OUT:-profile_out}
export TMPDIR=/tmp
mkdir -p "$OUT"
# the bench's own timed leg and its instrumented pass, nothing else (dropout
# off, no side lines): the k_fwd_fused / k_gru_bwd averages of this trace and
# the roofline of the JSON line in ${TAG}_trace.log come from the same launches
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_trace -o bench -- \
  python3 bench.py --steps 200 --warmup 10 --full --no-cpu-baseline --no-side --no-dropout-leg > $OUT/${TAG}_trace.log 2>&1
PMC_RUN=$TAG bash tools/pmc_profile.sh $OUT/${TAG}_pmc > $OUT/${TAG}_pmc.log 2>&1
cp $OUT/${TAG}_pmc/pmc_traffic.json profiles/pmc_traffic.json
PMC_RUN=$TAG bash tools/pmc_profile.sh $OUT/${TAG}_pmcbf16 --steps 2 --warmup 1 --full --no-cpu-baseline --no-side \
  --precision bf16 --pmc-unfused-leg > $OUT/${TAG}_pmcbf16.log 2>&1
cp $OUT/${TAG}_pmcbf16/pmc_traffic.json profiles/pmc_traffic_bf16.json
# inference-only forwards (no saves): the GRU's bytes against SURVEY §8d's 12 v h
bash tools/pmc_profile_infer.sh $OUT/${TAG}_pmcinfer bf16 > $OUT/${TAG}_pmcinfer.log 2>&1
cp $OUT/${TAG}_pmcinfer/pmc_traffic.json profiles/pmc_traffic_bf16_infer.json
timeout -k 10 600 python3 bench.py --full > $OUT/${TAG}_bench.log 2>&1
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1
