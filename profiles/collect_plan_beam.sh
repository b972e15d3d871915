#!/bin/bash
# What the beam search over stride options (fpe_plan_beam_device) costs around its resume launches, on the GPU box:
#   bash profiles/collect_plan_beam.sh OUTDIR [PARENT_TREE]
# (a), (b): one run of profiles/probe_plan_beam.py (one process, device events, no profiler): the beam call at B 64 roots, W 8, M 8,
# S 4, k 2 on the headline map against the same four fpe_plan_resume_device launches alone at the same chain counts, the two
# alternating block by block.  Then the beam call alone under rocprofv3 --kernel-trace --stats (no counters) for the per-kernel
# split.  (c), with PARENT_TREE — a checkout of the parent commit with its library built: bench.py's headline from both trees, this
# tree first and last.  Every GPU step runs under its own time limit and a failing step ends the script.
# Raw output -> OUTDIR/beam_*; the committed summary is profiles/plan_beam_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_plan_beam.sh OUTDIR [PARENT_TREE]}
PARENT=${2:-}
export TMPDIR=/tmp
mkdir -p $OUT/beam_stats
timeout -k 10 300 python3 profiles/probe_plan_beam.py 2>&1 | tee $OUT/beam_probe.txt || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/beam_stats -o beam -- \
  python3 profiles/probe_plan_beam.py --beam-only --steps 10 --blocks 2 > $OUT/beam_stats/run.log 2>&1 || exit $?
find $OUT/beam_stats -name '*kernel_stats.csv' | head -1 | xargs -r cat | cut -c1-200 | tee $OUT/beam_kernel_stats.txt
if [ -n "$PARENT" ]; then
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/beam_bench_head_1.json || exit $?
  (cd $PARENT && timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1) | tee $OUT/beam_bench_parent.json || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/beam_bench_head_2.json || exit $?
fi
