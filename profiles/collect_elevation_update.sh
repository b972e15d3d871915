#!/bin/bash
# What an elevation-driven map update (fpe_update_elevation_device) costs against the path it replaces — the full filter chain
# over the composed elevation plus fpe_upload_map_device — on the GPU box:
#   bash profiles/collect_elevation_update.sh OUTDIR [PARENT_TREE]
# (a) one run of profiles/probe_elevation_update.py (one process, the profiler off): the two routes alternating block by block,
# timed with device events, for 1000 x 1000 @ 2 cm and 2000 x 2000 @ 1 cm, a move by (5, 3) cells with the two exposed bands as
# patches and a 1 x 1 patch without a shift.  (b), with PARENT_TREE — a checkout of the parent commit with its library built:
# bench.py's headline from both trees, this tree first and last (the plan kernels are not touched: the three lines should agree
# within the session's noise).  Every GPU step runs under its own time limit and a failing step ends the script.
# Raw output -> OUTDIR/elevation_update_*; the committed summary is profiles/elevation_update_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_elevation_update.sh OUTDIR [PARENT_TREE]}
PARENT=${2:-}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python3 profiles/probe_elevation_update.py 2>&1 | tee $OUT/elevation_update_probe.txt || exit $?
if [ -n "$PARENT" ]; then
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/elevation_update_bench_head_1.json || exit $?
  (cd $PARENT && timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1) | tee $OUT/elevation_update_bench_parent.json || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/elevation_update_bench_head_2.json || exit $?
fi
