#!/bin/bash
# What the checked beam (fpe_plan_beam_checked_device) costs beside the composed sequence it replaces — fpe_plan_beam_device plus one
# fpe_check_plan_device per segment — and beside the unchecked beam, on the GPU box:
#   bash profiles/collect_beam_checked.sh OUTDIR [PARENT_TREE]
# For each configuration (headline: 1000 x 1000 at 2 cm; cfg5: 4000 x 4000 at 0.5 cm; B 64 roots, W 8, M 8, S 4, k 2, all three
# checks on): one run of profiles/probe_beam_checked.py without the profiler (one process, device events, 3 warm-up blocks, four
# blocks of 20 back-to-back calls per variant, the variants alternating block by block), then the checked beam alone and the
# composed sequence alone, each in a separate run under rocprofv3 --kernel-trace --stats for the per-kernel split.  No counters are
# collected anywhere in this recipe.  With PARENT_TREE — a checkout of the parent commit with its library built: bench.py's headline
# from both trees, this tree first and last.  Every GPU step runs under its own time limit and a failing step ends the script.
# Raw output -> OUTDIR/beam_checked_*; the committed summary is profiles/beam_checked_summary.txt.
set -u -o pipefail
OUT=${1:?usage: collect_beam_checked.sh OUTDIR [PARENT_TREE]}
PARENT=${2:-}
export TMPDIR=/tmp
mkdir -p $OUT/beam_checked_stats
for cfg in headline cfg5; do
  timeout -k 10 300 python3 profiles/probe_beam_checked.py --config $cfg --steps 20 --blocks 4 2>&1 | tee -a $OUT/beam_checked_events.txt || exit $?
done
for cfg in headline cfg5; do
  for side in checked composed; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/beam_checked_stats/${cfg}_$side -o beam_checked -- \
      python3 profiles/probe_beam_checked.py --config $cfg --only $side --steps 10 --blocks 2 > $OUT/beam_checked_stats/${cfg}_$side.log 2>&1 \
      || { rc=$?; tail -30 $OUT/beam_checked_stats/${cfg}_$side.log; exit $rc; }
    echo "== $cfg $side" | tee -a $OUT/beam_checked_kernel_stats.txt
    find $OUT/beam_checked_stats/${cfg}_$side -name '*kernel_stats.csv' | head -1 | xargs -r cat | cut -c1-160 | head -14 | tee -a $OUT/beam_checked_kernel_stats.txt
  done
done
if [ -n "$PARENT" ]; then
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/beam_checked_bench_head_1.json || exit $?
  (cd $PARENT && timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1) | tee $OUT/beam_checked_bench_parent.json || exit $?
  timeout -k 10 200 python3 bench.py --gpus 1 --steps 50 --warmup 5 2>&1 | tail -1 | tee $OUT/beam_checked_bench_head_2.json || exit $?
fi
