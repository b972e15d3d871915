#!/bin/bash
# Profile of the batch ranking (fpe_plan_rank*) at the headline shape (1000^2 @ 2 cm, B 4096, 8 cycles), on the GPU box:
#   bash profiles/collect_plan_rank.sh OUTDIR
# One run without the profiler: the host call against fpe_plan (all products / selected_packed only), alternating in one process,
# 200 calls each, for K = 16 and K = 1024.  Then, per K, the device form under rocprofv3 --kernel-trace --stats (no counters are
# collected).  Raw output -> OUTDIR/rank_*; `python3 profiles/probe_plan_rank.py --summarise OUTDIR/rank_stats` prints the
# per-kernel table of the committed summary.
set -u
OUT=${1:?usage: collect_plan_rank.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/rank_stats
timeout -k 10 300 python3 profiles/probe_plan_rank.py --host --calls 200 > $OUT/rank_host.txt 2>&1 || exit $?
for k in 16 1024; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/rank_stats/k$k -o rank -- \
    python3 profiles/probe_plan_rank.py --device --k $k --calls 50 > $OUT/rank_stats/k$k.log 2>&1 || exit $?
done
cat $OUT/rank_host.txt
python3 profiles/probe_plan_rank.py --summarise $OUT/rank_stats | tee $OUT/rank_summary.txt
