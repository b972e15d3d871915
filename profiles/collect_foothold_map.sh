#!/bin/bash
# Kernel-trace profile of the dense foothold map (fpe_foothold_map_device) on whole maps, on the GPU box:
#   bash profiles/collect_foothold_map.sh OUTDIR
# For each map (1000^2 @ 2 cm, 2000^2 @ 1 cm, 4000^2 @ 0.5 cm) and product set (flags + heights, flags only): one run without the
# profiler (device-event time per call), then one under rocprofv3 --kernel-trace --stats.  Raw output -> OUTDIR/fmap_*;
# `python3 profiles/probe_foothold_map.py --summarise OUTDIR/fmap_stats` prints the committed summary.
set -u
OUT=${1:?usage: collect_foothold_map.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/fmap_stats
for cfg in 1000_2cm 2000_1cm 4000_05cm; do
  for prod in both flags; do
    timeout -k 10 300 python3 profiles/probe_foothold_map.py --config $cfg --products $prod --calls 50 >> $OUT/fmap_events.txt 2>&1 || exit $?
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/fmap_stats/${cfg}_${prod} -o fmap -- \
      python3 profiles/probe_foothold_map.py --config $cfg --products $prod --calls 50 > $OUT/fmap_stats/${cfg}_${prod}.log 2>&1 || exit $?
  done
done
cat $OUT/fmap_events.txt
python3 profiles/probe_foothold_map.py --summarise $OUT/fmap_stats | tee $OUT/fmap_summary.txt
