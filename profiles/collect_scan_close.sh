#!/bin/bash
# What closing the small gaps of a scan state's elevation costs (fpe_scan_close_device), on the GPU box:
#   bash profiles/collect_scan_close.sh OUTDIR
# (0) the streaming yardstick's library, built here when it is missing (hipcc, no GPU; a few seconds — build it before going to the GPU
# box).  (a) one run of profiles/probe_scan_close.py (one process, the profiler off): both forms of the close on an ingest's rectangle
# and on the whole map, the yardstick, the fuse beside them and ingest_clear against ingest_closed, alternating block by block, device
# events, for a 640 x 480 depth image on 1000 x 1000 @ 2 cm with a 300 x 300 roi.  (b) the kernels alone: `rocprofv3 --kernel-trace
# --stats` over a short run of the same probe, a run of its own (no counters are collected).  (c) bench.py's headline line (the plan
# kernels are not touched).  Every GPU step runs under its own time limit and a failing step ends the script.  Raw output ->
# OUTDIR/scan_close_*; the committed summary is profiles/scan_close_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_scan_close.sh OUTDIR}
export TMPDIR=/tmp
mkdir -p $OUT profiles/_build
if [ ! -f profiles/_build/libscan_yardstick.so ] || [ profiles/scan_yardstick.hip -nt profiles/_build/libscan_yardstick.so ]; then
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared profiles/scan_yardstick.hip -o profiles/_build/libscan_yardstick.so || exit $?
fi
timeout -k 10 240 python3 profiles/probe_scan_close.py 2>&1 | tee $OUT/scan_close_probe.txt || exit $?
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/scan_close_trace -o scan_close -- python3 profiles/probe_scan_close.py --trace > $OUT/scan_close_trace.log 2>&1 || exit $?
python3 profiles/probe_scan_close.py --passes $OUT/scan_close_trace | tee $OUT/scan_close_passes.txt
timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/scan_close_bench_head.json || exit $?
