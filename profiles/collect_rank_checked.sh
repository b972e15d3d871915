#!/bin/bash
# Profile of the checked ranking's check stage (fpe_check_plan_device: plan_check_kernel<false>) beside the three plan-bound checks it
# fuses, and of fpe_plan_rank_checked_device beside fpe_plan_rank_device, on the GPU box:
#   bash profiles/collect_rank_checked.sh OUTDIR
# For each configuration (headline: 1000 x 1000 at 2 cm; cfg5: 4000 x 4000 at 0.5 cm; 4 096 poses x 8 cycles each): one run without the
# profiler (device-event time per call, the two sides alternating in blocks, same map, same process), then a separate run under
# rocprofv3 --kernel-trace --stats with no counters in it; last, the counters in a run of their own with no tracing beside them
# (headline only).  Every GPU step has its own time limit and the script ends at the first failure.  Raw output ->
# OUTDIR/rank_checked_*; `python3 profiles/probe_rank_checked.py --summarise OUTDIR/rank_checked_stats` prints the kernel lines of the
# committed summary (profiles/rank_checked_summary.txt).
set -u
OUT=${1:?usage: collect_rank_checked.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/rank_checked_stats
for cfg in headline cfg5; do
  timeout -k 10 300 python3 profiles/probe_rank_checked.py --config $cfg --calls 20 --blocks 4 >> $OUT/rank_checked_events.txt 2>&1 || { rc=$?; cat $OUT/rank_checked_events.txt; exit $rc; }
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/rank_checked_stats/$cfg -o rank_checked -- \
    python3 profiles/probe_rank_checked.py --config $cfg --calls 20 --blocks 1 --no-check > $OUT/rank_checked_stats/$cfg.log 2>&1 || { rc=$?; tail -30 $OUT/rank_checked_stats/$cfg.log; exit $rc; }
done
cat $OUT/rank_checked_events.txt
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE SQ_INSTS_VALU SQ_WAVES --output-format csv -d $OUT/rank_checked_stats/headline_counters -o rank_checked -- \
  python3 profiles/probe_rank_checked.py --config headline --calls 5 --blocks 1 --no-check > $OUT/rank_checked_stats/headline_counters.log 2>&1 || { rc=$?; tail -30 $OUT/rank_checked_stats/headline_counters.log; exit $rc; }
python3 profiles/probe_rank_checked.py --summarise $OUT/rank_checked_stats | tee $OUT/rank_checked_summary.txt
