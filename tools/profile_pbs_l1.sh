#!/bin/bash
# Runs on the GPU box: how much of SET_1's bootstrap-key stream the CUs' vector L1 serves, for the throughput kernel with one ciphertext per workgroup (group 0)
# and with four (group 4; MOSFHET_HIP_PBS_GROUP), 4096 programmable bootstraps per launch (tools/gpu_perf.py 4096 set1).
#   tools/profile_pbs_l1.sh <tag> ["0 4"]  ->  $PROF_OUT/prof_<tag>_g<group>/summary.txt  (PROF_OUT: default prof_out/ in the tree; copy the summaries into profiles/)
# Kernel-trace statistics and counters are taken in SEPARATE runs, every --pmc pass is a run of its own, and no tracing rides along with a counter pass.
# Every run has its own time limit and a failed run ends the script.
set -u
TAG=${1:-pbs_l1}
GROUPS_=${2:-"0 4"}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
SETS="FETCH_SIZE;WRITE_SIZE;TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum;TCP_TOTAL_READ_sum TCP_TOTAL_ACCESSES_sum;TCC_HIT_sum TCC_MISS_sum;SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD"
for G in $GROUPS_; do
  OUT=${PROF_OUT:-$ROOT/prof_out}/prof_${TAG}_g$G
  mkdir -p $OUT
  export MOSFHET_HIP_PBS_GROUP=$G
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 $ROOT/tools/gpu_perf.py 4096 set1 > $OUT/trace.log 2>&1 || { echo "trace run of group $G failed ($?)"; tail -5 $OUT/trace.log; exit 1; }
  IFS=';' read -ra LIST <<< "$SETS"
  for C in "${LIST[@]}"; do
    N=$(echo $C | tr ' ' '_' | cut -c1-40)
    timeout -k 10 240 rocprofv3 --pmc $C --output-format csv -d $OUT/pmc_$N -- python3 $ROOT/tools/gpu_perf.py 4096 set1 > $OUT/pmc_$N.log 2>&1 || { echo "counter run '$C' of group $G failed ($?)"; tail -5 $OUT/pmc_$N.log; exit 1; }
  done
  python3 $ROOT/tools/summarize_prof.py $OUT > $OUT/summary.txt 2>&1
  echo "=== group $G"; grep -E "calls=|per-dispatch" $OUT/summary.txt | grep pbs_kernel | head -30
done
