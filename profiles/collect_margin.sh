#!/bin/bash
# Profile of the edge margin (fpe_margin_map_device, fpe_margin_plan_device) beside the foothold map's flags product on the same map and
# beside the plan and the trunk check of the same batch, on the GPU box:
#   bash profiles/collect_margin.sh OUTDIR
# For each configuration (headline: 1000 x 1000 at 2 cm; cfg5: 4000 x 4000 at 0.5 cm): one run without the profiler (device-event time
# per call, same map, same process), then a separate run under rocprofv3 --kernel-trace --stats with no counters in it; last, the
# counters in a run of their own with no tracing beside them (headline only).  Every GPU step has its own time limit and the script ends
# at the first failure.  Raw output -> OUTDIR/margin_*; `python3 profiles/probe_margin.py --summarise OUTDIR/margin_stats` prints the
# kernel lines of the committed summary (profiles/margin_summary.txt).
set -u
OUT=${1:?usage: collect_margin.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/margin_stats
for cfg in headline cfg5; do
  timeout -k 10 300 python3 profiles/probe_margin.py --config $cfg --calls 20 >> $OUT/margin_events.txt 2>&1 || { rc=$?; cat $OUT/margin_events.txt; exit $rc; }
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/margin_stats/$cfg -o margin -- \
    python3 profiles/probe_margin.py --config $cfg --calls 20 --no-check > $OUT/margin_stats/$cfg.log 2>&1 || { rc=$?; tail -30 $OUT/margin_stats/$cfg.log; exit $rc; }
done
cat $OUT/margin_events.txt
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE SQ_INSTS_LDS --output-format csv -d $OUT/margin_stats/headline_counters -o margin -- \
  python3 profiles/probe_margin.py --config headline --calls 5 --no-check > $OUT/margin_stats/headline_counters.log 2>&1 || { rc=$?; tail -30 $OUT/margin_stats/headline_counters.log; exit $rc; }
python3 profiles/probe_margin.py --summarise $OUT/margin_stats | tee $OUT/margin_summary.txt
