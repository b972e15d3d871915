#!/bin/bash
# What the resume instantiations cost (fpe_plan_resume_device from a cycle-0 state with uniform strides: the same plan as the stride
# call) at the headline shape and at cfg-3, and what planning in two segments costs, on the GPU box:
#   bash profiles/collect_plan_resume.sh OUTDIR [PARENT_TREE]
# One run of profiles/probe_plan_resume.py (one process, device events, no profiler): resume / start / stride (/ halves) per shape and
# the ratios.  With PARENT_TREE — a checkout of the parent commit with its library built — the same session also runs the probe's
# --stride-only mode from that tree (the parent commit's fpe_plan_strides_device: the yardstick) and bench.py's headline from both
# trees, this tree first and last.  Raw output -> OUTDIR/resume_*.txt; the committed summary is profiles/plan_resume_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_plan_resume.sh OUTDIR [PARENT_TREE]}
PARENT=${2:-}
mkdir -p $OUT
timeout -k 10 300 python3 profiles/probe_plan_resume.py 2>&1 | tee $OUT/resume_probe.txt || exit $?
if [ -n "$PARENT" ]; then
  FPE_TREE=$PARENT timeout -k 10 300 python3 profiles/probe_plan_resume.py --stride-only 2>&1 | tee $OUT/resume_probe_parent.txt || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/resume_bench_head_1.json || exit $?
  (cd $PARENT && timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1) | tee $OUT/resume_bench_parent.json || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/resume_bench_head_2.json || exit $?
fi
