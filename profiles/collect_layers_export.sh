#!/bin/bash
# Profile of the message-layer export (fpe_export_layers_device) and of the ingest's canonicalise_layer_kernel on whole maps, on
# the GPU box:
#   bash profiles/collect_layers_export.sh OUTDIR
# For each map (1000^2 @ 2 cm, 2000^2 @ 1 cm, 4000^2 @ 0.5 cm): one run without the profiler (device-event time per call), then a
# separate run under rocprofv3 --kernel-trace --stats with no counters in it.  Raw output -> OUTDIR/layers_*;
# `python3 profiles/probe_layers_export.py --summarise OUTDIR/layers_stats` prints the committed summary's kernel lines.
set -u
OUT=${1:?usage: collect_layers_export.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/layers_stats
for cfg in 1000_2cm 2000_1cm 4000_05cm; do
  timeout -k 10 240 python3 profiles/probe_layers_export.py --config $cfg --calls 20 >> $OUT/layers_events.txt 2>&1 || { rc=$?; cat $OUT/layers_events.txt; exit $rc; }
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/layers_stats/$cfg -o layers -- \
    python3 profiles/probe_layers_export.py --config $cfg --calls 20 > $OUT/layers_stats/$cfg.log 2>&1 || { rc=$?; tail -30 $OUT/layers_stats/$cfg.log; exit $rc; }
done
cat $OUT/layers_events.txt
python3 profiles/probe_layers_export.py --summarise $OUT/layers_stats | tee $OUT/layers_summary.txt
