#!/bin/bash
# What clearing the cells a scan sees through costs (fpe_scan_clear_device), on the GPU box:
#   bash profiles/collect_scan_clear.sh OUTDIR
# (a) one run of profiles/probe_scan_clear.py (one process, the profiler off): the forms of the ray pass, the fuse beside them and the
# whole ingest against ingest_clear, alternating block by block, device events, for a 640 x 480 depth image and a 64 x 2048 lidar sweep
# on 1000 x 1000 @ 2 cm with a 300 x 300 roi.  (b) the per-pass split: `rocprofv3 --kernel-trace --stats` over a short run of the same
# probe, a run of its own (no counters are collected).  (c) bench.py's headline line (the plan kernels are not touched).  Every GPU
# step runs under its own time limit and a failing step ends the script.  Raw output -> OUTDIR/scan_clear_*; the committed summary is
# profiles/scan_clear_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_scan_clear.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python3 profiles/probe_scan_clear.py 2>&1 | tee $OUT/scan_clear_probe.txt || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/scan_clear_trace -o scan_clear -- python3 profiles/probe_scan_clear.py --trace > $OUT/scan_clear_trace.log 2>&1 || exit $?
python3 profiles/probe_scan_clear.py --passes $OUT/scan_clear_trace | tee $OUT/scan_clear_passes.txt
timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/scan_clear_bench_head.json || exit $?
