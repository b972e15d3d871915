#!/bin/bash
# What fusing and clearing a depth or range image costs against the same scan as a point cloud, on the GPU box:
#   bash profiles/collect_scan_image.sh OUTDIR
# (a) one run of profiles/probe_scan_image.py (one process, the profiler off): fpe_scan_fuse_device against fpe_scan_fuse_image_device,
# the same pair for the clear (default form) and for ingest_closed against ingest_image with cp and kp, alternating block by block,
# device events; then the host forms of the fuse by wall clock — for the 640 x 480 depth image as uint16 and the 64 x 2048 sweep as a
# spherical float image on 1000 x 1000 @ 2 cm with a 300 x 300 roi.  (b) the per-pass split: `rocprofv3 --kernel-trace --stats` over a
# short run of the same probe, a run of its own (no counters are collected).  (c) bench.py's headline line (the plan kernels are not
# touched).  Every GPU step runs under its own time limit and a failing step ends the script.  Raw output -> OUTDIR/scan_image_*; the
# committed summary is profiles/scan_image_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_scan_image.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 240 python3 profiles/probe_scan_image.py 2>&1 | tee $OUT/scan_image_probe.txt || exit $?
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/scan_image_trace -o scan_image -- python3 profiles/probe_scan_image.py --trace > $OUT/scan_image_trace.log 2>&1 || exit $?
python3 profiles/probe_scan_image.py --passes $OUT/scan_image_trace | tee $OUT/scan_image_passes.txt
timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/scan_image_bench_head.json || exit $?
