#!/bin/bash
# Kernel-trace profile of the dense snap map (fpe_foothold_snap_device) against fpe_search_legs_device on whole maps, on the GPU box:
#   bash profiles/collect_foothold_snap.sh OUTDIR
# For each map (1000^2 @ 2 cm, 2000^2 @ 1 cm, 4000^2 @ 0.5 cm): one run without the profiler (device-event time per call), then one
# under rocprofv3 --kernel-trace --stats.  Raw output -> OUTDIR/fsnap_*; `python3 profiles/probe_foothold_snap.py --summarise
# OUTDIR/fsnap_stats` prints the per-kernel table of the committed summary.
set -u
OUT=${1:?usage: collect_foothold_snap.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT/fsnap_stats
for cfg in 1000_2cm 2000_1cm 4000_05cm; do
  timeout -k 10 600 python3 profiles/probe_foothold_snap.py --config $cfg >> $OUT/fsnap_events.txt 2>&1 || exit $?
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/fsnap_stats/$cfg -o fsnap -- \
    python3 profiles/probe_foothold_snap.py --config $cfg > $OUT/fsnap_stats/$cfg.log 2>&1 || exit $?
done
cat $OUT/fsnap_events.txt
python3 profiles/probe_foothold_snap.py --summarise $OUT/fsnap_stats | tee $OUT/fsnap_summary.txt
