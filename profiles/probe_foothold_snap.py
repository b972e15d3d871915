"""Dense snap map (fpe_foothold_snap_device) on whole maps against fpe_search_legs_device on the same cells: the workload of
the kernel-trace profile and its summary.

    python3 profiles/probe_foothold_snap.py --config 4000_05cm --calls 20
        uploads a synthetic rough map (yaml parameters), warms up, then queues --calls snap calls (offset + source) back to
        back on one stream and prints the event-timed mean per call; then the same for offset + source + z, and for
        fpe_search_legs_device over the queries of every cell (built once, outside the timed region), and checks that
        both give the same offsets and sources;
    python3 profiles/probe_foothold_snap.py --summarise DIR
        reads DIR/<config>/*kernel_stats.csv of collect_foothold_snap.sh and prints microseconds per kernel.
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"1000_2cm": (1000, 0.02), "2000_1cm": (2000, 0.01), "4000_05cm": (4000, 0.005)}
KERNELS = ("footsnap_bits_kernel", "footmap_height_kernel", "search_legs_kernel", "build_bitmap_kernel", "canonicalise")


def timed(fn, s, calls, warmup):
    import torch

    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
        s.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(s)
        for _ in range(calls):
            fn()
        t1.record(s)
    s.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def run(config, calls, warmup, legs_calls):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi, synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

    rows, res = CONFIGS[config]
    trav, elev = synth.rough_map(rows, rows, res, seed=5)
    p = FootholdPlanner(0)
    p.gridmapCallback(trav, elev, res)
    n = rows * rows
    d_off = torch.empty(2 * n, dtype=torch.int8, device="cuda")
    d_src = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_z = torch.empty(n, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    us_os = timed(lambda: p.foothold_snap_device(d_off.data_ptr(), d_src.data_ptr(), 0, stream=s.cuda_stream), s, calls, warmup)
    us_all = timed(lambda: p.foothold_snap_device(d_off.data_ptr(), d_src.data_ptr(), d_z.data_ptr(), stream=s.cuda_stream), s,
                   calls, warmup)
    src = d_src.cpu().numpy()
    off = d_off.cpu().numpy().reshape(n, 2)
    # the queries of every cell (the contract's), built on the host once: getPosition = base - res * index
    R = float(np.float32(p.params["searchRadius"][0]))
    x0 = 0.0 + (0.5 * (rows * res) - 0.5 * res)  # getPosition's base at map position (0, 0) (fpe_gridmath.hpp make_geom)
    ii, jj = np.meshgrid(np.arange(rows), np.arange(rows), indexing="ij")
    q = np.zeros(n, dtype=_capi.QUERY_DTYPE)
    cx = (x0 + res * -ii.astype(np.float64)).ravel()
    cy = (x0 + res * -jj.astype(np.float64)).ravel()
    q["cx"], q["cy"], q["search_radius"], q["n_vertices"] = cx, cy, np.float32(R), 4
    for k, (ax, ay) in enumerate([(R, 0.5 * R), (R, -0.5 * R), (-R, -0.5 * R), (-R, 0.5 * R)]):
        q["vx"][:, k] = cx + ax
        q["vy"][:, k] = cy + ay
    d_q = torch.from_numpy(q.view(np.uint8)).cuda()
    d_f = torch.empty(n * _capi.FOOTHOLD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    us_legs = timed(lambda: p.search_legs_device(d_q.data_ptr(), n, d_f.data_ptr(), stream=s.cuda_stream), s, legs_calls, 1)
    f = d_f.cpu().numpy().view(_capi.FOOTHOLD_DTYPE)
    assert np.array_equal(f["source"], src), "snap source != search_legs source"
    sp = f["source"] == 1
    assert np.array_equal(f["row"][sp] - ii.ravel()[sp], off[sp, 0].astype(np.int64))
    assert np.array_equal(f["col"][sp] - jj.ravel()[sp], off[sp, 1].astype(np.int64))
    frac = [float(np.mean(src == k)) for k in range(3)]
    p.close()
    print(f"{config}: {rows}x{rows} cells, sources 0/1/2 = {frac[0]:.3f}/{frac[1]:.3f}/{frac[2]:.3f}; per call (device events): "
          f"snap offset+source {us_os:.1f} us, snap +z {us_all:.1f} us, search_legs_device {us_legs:.1f} us "
          f"-> {us_legs / us_os:.1f}x")


def summarise(directory):
    print(f"{'run':12s} {'kernel':28s} {'calls':>6s} {'us/call':>9s}")
    for config in CONFIGS:
        files = glob.glob(os.path.join(directory, config, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print(f"{config}: no kernel_stats.csv (not measured)")
            continue
        with open(files[0]) as fh:
            for r in csv.DictReader(fh):
                name = next((k for k in KERNELS if k in r["Name"]), None)
                if name is None:
                    continue
                print(f"{config:12s} {name:28s} {int(r['Calls']):6d} {float(r['AverageNs']) / 1e3:9.1f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="4000_05cm")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--legs-calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    else:
        run(a.config, a.calls, a.warmup, a.legs_calls)
