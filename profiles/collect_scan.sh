#!/bin/bash
# What fusing one scan into the elevation layer costs (fpe_scan_fuse_device), on the GPU box:
#   bash profiles/collect_scan.sh OUTDIR
# (0) the streaming yardstick's library, built here when it is missing (hipcc, no GPU; a few seconds — build it before going to the GPU
# box).  (a) one run of profiles/probe_scan.py (one process, the profiler off): both forms of the point passes, the yardstick, the
# dirty-region update of the same rectangle and the whole ingest, alternating block by block, device events, for a 640 x 480 depth
# image and a 64 x 2048 lidar sweep on 1000 x 1000 @ 2 cm with a 300 x 300 roi.  (b) the per-pass split: `rocprofv3 --kernel-trace
# --stats` over a short run of the same probe, a run of its own (no counters are collected; a counter pass would be one more run).
# (c) bench.py's headline line (the plan kernels are not touched).  Every GPU step runs under its own time limit and a failing step
# ends the script.  Raw output -> OUTDIR/scan_*; the committed summary is profiles/scan_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_scan.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT profiles/_build
if [ ! -f profiles/_build/libscan_yardstick.so ] || [ profiles/scan_yardstick.hip -nt profiles/_build/libscan_yardstick.so ]; then
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared profiles/scan_yardstick.hip -o profiles/_build/libscan_yardstick.so || exit $?
fi
timeout -k 10 240 python3 profiles/probe_scan.py 2>&1 | tee $OUT/scan_probe.txt || exit $?
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/scan_trace -o scan -- python3 profiles/probe_scan.py --trace > $OUT/scan_trace.log 2>&1 || exit $?
python3 profiles/probe_scan.py --passes $OUT/scan_trace | tee $OUT/scan_passes.txt
timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/scan_bench_head.json || exit $?
