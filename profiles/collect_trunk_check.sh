#!/bin/bash
# Profile of the trunk check (fpe_trunk_plan_device) beside the plan that produced its input (fpe_plan_device) and the swing check of
# the same batch (fpe_swing_plan_device), on the GPU box:
#   bash profiles/collect_trunk_check.sh OUTDIR
# For each configuration (headline, cfg5's geometry): one run without the profiler (device-event time per call of the three, same
# batch, same process), then a separate run under rocprofv3 --kernel-trace --stats with no counters in it; last, the counters in
# a run of their own (FETCH_SIZE, headline only).  Every GPU step has its own time limit and the script ends at the first failure.
# Raw output -> OUTDIR/trunk_*; `python3 profiles/probe_trunk_check.py --summarise OUTDIR/trunk_stats` prints the kernel lines of
# the committed summary (profiles/trunk_check_summary.txt).
set -u
OUT=${1:?usage: collect_trunk_check.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/trunk_stats
for cfg in headline cfg5; do
  sample=4; [ $cfg = cfg5 ] && sample=1   # (the reference walks every cell of the map per stance: 16 M cells at cfg5)
  timeout -k 10 300 python3 profiles/probe_trunk_check.py --config $cfg --calls 20 --sample $sample >> $OUT/trunk_events.txt 2>&1 || { rc=$?; cat $OUT/trunk_events.txt; exit $rc; }
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trunk_stats/$cfg -o trunk -- \
    python3 profiles/probe_trunk_check.py --config $cfg --calls 20 --sample 0 > $OUT/trunk_stats/$cfg.log 2>&1 || { rc=$?; tail -30 $OUT/trunk_stats/$cfg.log; exit $rc; }
done
cat $OUT/trunk_events.txt
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/trunk_stats/headline_fetch -o trunk -- \
  python3 profiles/probe_trunk_check.py --config headline --calls 5 --sample 0 > $OUT/trunk_stats/headline_fetch.log 2>&1 || { rc=$?; tail -30 $OUT/trunk_stats/headline_fetch.log; exit $rc; }
python3 profiles/probe_trunk_check.py --summarise $OUT/trunk_stats | tee $OUT/trunk_summary.txt
