#!/bin/bash
# Kernel-trace profile of the dense centroid map (fpe_centroid_map_device) against fpe_centroid_legs_device on whole maps, on the GPU
# box:
#   bash profiles/collect_centroid_map.sh OUTDIR
# For each map (1000^2 @ 2 cm, 2000^2 @ 1 cm, 4000^2 @ 0.5 cm): one run without the profiler (device-event time per call), then one
# under rocprofv3 --kernel-trace --stats.  Raw output -> OUTDIR/cmap_*; `python3 profiles/probe_centroid_map.py --summarise
# OUTDIR/cmap_stats` prints the per-kernel table of the committed summary.
set -u
OUT=${1:?usage: collect_centroid_map.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/cmap_stats
for cfg in 1000_2cm 2000_1cm 4000_05cm; do
  timeout -k 10 600 python3 profiles/probe_centroid_map.py --config $cfg >> $OUT/cmap_events.txt 2>&1 || exit $?
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/cmap_stats/$cfg -o cmap -- \
    python3 profiles/probe_centroid_map.py --config $cfg > $OUT/cmap_stats/$cfg.log 2>&1 || exit $?
done
cat $OUT/cmap_events.txt
python3 profiles/probe_centroid_map.py --summarise $OUT/cmap_stats | tee $OUT/cmap_summary.txt
