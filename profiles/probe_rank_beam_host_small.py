"""The host forms of the ranking and the beam at a small batch, where the call is latency-bound: wall-clock per call through the
Python binding, on the headline map.

    python3 profiles/probe_rank_beam_host_small.py [--tree DIR] [--calls 300] [--warmup 30]
        plan_rank   B 64, 8 cycles, K 16, products nominal / cycle_ok / stance, with summary and score
        plan_beam   B 1, the default shape (S 4, k 2, W 8), M 8 options, products nominal / cycle_ok
      ONE process, the two calls alternating, median and p10 / p90 in microseconds.  --tree: the checkout whose package is
      measured (default: the one this file lies in), so that one copy of the probe serves an A/B of two trees.
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np

    from quadrupedal_foothold_planner_amd import synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_strides

    trav, elev, res, poses, n, _ = synth.make_config("headline")
    p = FootholdPlanner(0)
    p.gridmapCallback(trav, elev, res)
    step0, drift0 = float(p.params["stepLength"][0]), float(p.params["lateralDrift"][0])
    options = make_strides(step0 * np.linspace(0.6, 1.4, 8), drift0 + np.linspace(-0.01, 0.01, 8))
    runs = {
        "plan_rank B 64 K 16": lambda: p.plan_rank(poses[:64], n, 16),
        "plan_beam B 1 default shape, M 8": lambda: p.plan_beam(poses[:1], options),
    }
    times = {k: [] for k in runs}
    for it in range(a.warmup + a.calls):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                times[name].append(dt * 1e6)
    for name, t in times.items():
        t = np.sort(np.array(t))
        print(f"{name:34s} median {np.median(t):8.1f} us  p10 {t[len(t) // 10]:8.1f}  p90 {t[(9 * len(t)) // 10]:8.1f}  ({len(t)} calls)")
    p.close()


if __name__ == "__main__":
    main()
