#!/bin/bash
# What an incremental map update (fpe_update_map*) costs against the full upload it replaces, on the GPU box:
#   bash profiles/collect_map_update.sh OUTDIR [PARENT_TREE]
# (a), (b): one run of profiles/probe_map_update.py (one process, the profiler off): the device form against fpe_upload_map_device
# of the same composed map, alternating block by block and timed with device events, and the host form against fpe_upload_map from
# pageable and pinned arrays at the C entry point, for 1000 x 1000 @ 2 cm and 4000 x 4000.  (c), with PARENT_TREE — a checkout of
# the parent commit with its library built: bench.py's headline from both trees, this tree first and last (the plan kernels are
# not touched: the three lines should agree within the session's noise).  Every GPU step runs under its own time limit and a
# failing step ends the script.
# Raw output -> OUTDIR/map_update_*; the committed summary is profiles/map_update_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_map_update.sh OUTDIR [PARENT_TREE]}
PARENT=${2:-}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python3 profiles/probe_map_update.py 2>&1 | tee $OUT/map_update_probe.txt || exit $?
if [ -n "$PARENT" ]; then
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/map_update_bench_head_1.json || exit $?
  (cd $PARENT && timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1) | tee $OUT/map_update_bench_parent.json || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/map_update_bench_head_2.json || exit $?
fi
