#!/bin/bash
# What the per-pose stride instantiations cost (fpe_plan_strides_device with uniform strides) at the headline shape and at cfg-3, on
# the GPU box:
#   bash profiles/collect_plan_strides.sh OUTDIR [PARENT_TREE]
# One run of profiles/probe_plan_strides.py (one process, device events, no profiler): stride / generic / today per shape and the
# two ratios.  With PARENT_TREE — a checkout of the parent commit with its library built — the same session also runs the probe's
# --plain-only mode from that tree (the parent commit's fpe_plan_device, generic and as launched today) and bench.py's headline
# from both trees, this tree first and last.  Raw output -> OUTDIR/strides_*.txt; the committed summary is
# profiles/plan_strides_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_plan_strides.sh OUTDIR [PARENT_TREE]}
PARENT=${2:-}
mkdir -p $OUT
timeout -k 10 300 python3 profiles/probe_plan_strides.py 2>&1 | tee $OUT/strides_probe.txt || exit $?
if [ -n "$PARENT" ]; then
  FPE_TREE=$PARENT timeout -k 10 300 python3 profiles/probe_plan_strides.py --plain-only 2>&1 | tee $OUT/strides_probe_parent.txt || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/strides_bench_head_1.json || exit $?
  (cd $PARENT && timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1) | tee $OUT/strides_bench_parent.json || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/strides_bench_head_2.json || exit $?
fi
