"""Dense foothold map (fpe_foothold_map_device) on whole maps: the workload of the kernel-trace profile and its summary.

    python3 profiles/probe_foothold_map.py --config 4000_05cm --products both --calls 50
        uploads a synthetic rough map, warms up, then queues --calls device calls back to back on one stream and prints the
        event-timed mean per call (the profile of this run, collect_foothold_map.sh, gives the per-kernel times);
    python3 profiles/probe_foothold_map.py --summarise DIR
        reads DIR/<config>_<products>/*kernel_stats.csv of collect_foothold_map.sh and prints microseconds per kernel and
        the algorithmic bytes over kernel time as a fraction of 8 TB/s (HBM peak).

Algorithmic bytes per cell (what the products need from and to HBM, not what the caches move):
  footmap_flags_bits_kernel  16 B per 32 cells read (the four planes of a word group) + 1 B written  = 1.5 B
  footmap_height_kernel      4 B elevation read + 4 B height written                                 = 8 B
  build_bitmap_kernel        4 B traversability read + 0.5 B planes written (once per snapshot and threshold pair)
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"1000_2cm": (1000, 0.02), "2000_1cm": (2000, 0.01), "4000_05cm": (4000, 0.005)}
BYTES_PER_CELL = {"footmap_flags_bits_kernel": 1.5, "footmap_height_kernel": 8.0, "build_bitmap_kernel": 4.5}
HBM_PEAK = 8.0e12


def run(config, products, calls, warmup):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

    rows, res = CONFIGS[config]
    trav, elev = synth.rough_map(rows, rows, res, seed=5)
    p = FootholdPlanner(0)
    p.gridmapCallback(trav, elev, res)
    n = rows * rows
    d_f = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_h = torch.empty(n, dtype=torch.float32, device="cuda") if products == "both" else None
    s = torch.cuda.Stream()
    hp = d_h.data_ptr() if d_h is not None else 0
    with torch.cuda.stream(s):
        for _ in range(warmup):
            p.foothold_map_device(d_f.data_ptr(), hp, stream=s.cuda_stream)
        s.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(s)
        for _ in range(calls):
            p.foothold_map_device(d_f.data_ptr(), hp, stream=s.cuda_stream)
        t1.record(s)
    s.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / calls
    # the result of the timed calls equals the host path's (same snapshot)
    want = p.foothold_map(products=("flags", "height") if products == "both" else ("flags",))
    assert np.array_equal(d_f.cpu().numpy().reshape(rows, rows), want["flags"])
    if d_h is not None:
        assert np.array_equal(d_h.cpu().numpy().reshape(rows, rows).view(np.uint32), want["height"].view(np.uint32))
    p.close()
    print(f"{config} {products}: {rows}x{rows} cells, {us:.1f} us per call (device events over {calls} back-to-back calls)")


def summarise(directory):
    print(f"{'run':22s} {'kernel':28s} {'calls':>6s} {'us/call':>9s} {'B/cell':>7s} {'GB/s':>8s} {'of 8 TB/s':>9s}")
    for config, (rows, _) in CONFIGS.items():
        for products in ("both", "flags"):
            files = glob.glob(os.path.join(directory, f"{config}_{products}", "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                print(f"{config}_{products}: no kernel_stats.csv (not measured)")
                continue
            with open(files[0]) as f:
                for r in csv.DictReader(f):
                    name = next((k for k in BYTES_PER_CELL if k + "(" in r["Name"]), None)
                    if name is None:
                        continue
                    us = float(r["AverageNs"]) / 1e3
                    gbs = BYTES_PER_CELL[name] * rows * rows / (us * 1e-6) / 1e9
                    print(f"{config + '_' + products:22s} {name:28s} {int(r['Calls']):6d} {us:9.1f} {BYTES_PER_CELL[name]:7.1f} "
                          f"{gbs:8.0f} {gbs * 1e9 / HBM_PEAK:9.1%}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="4000_05cm")
    ap.add_argument("--products", choices=("both", "flags"), default="both")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    else:
        run(a.config, a.products, a.calls, a.warmup)
