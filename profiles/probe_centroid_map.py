"""Dense centroid map (fpe_centroid_map_device) on whole maps against fpe_centroid_legs_device on the same cells: the workload of
the kernel-trace profile and its summary.

    python3 profiles/probe_centroid_map.py --config 4000_05cm --calls 20
        uploads a synthetic rough map (yaml parameters), warms up, then queues --calls dense calls (code + offset) back to
        back on one stream and prints the event-timed mean per call; then the same for code + offset + z, and for
        fpe_centroid_legs_device over the queries of every cell (built once, outside the timed region), and checks that
        both give the same codes, offsets and z;
    python3 profiles/probe_centroid_map.py --summarise DIR
        reads DIR/<config>/*kernel_stats.csv of collect_centroid_map.sh and prints microseconds per kernel.
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"1000_2cm": (1000, 0.02), "2000_1cm": (2000, 0.01), "4000_05cm": (4000, 0.005)}
KERNELS = ("cmap_axes_kernel", "cmap_rows_kernel", "cmap_code_kernel", "cmap_z_kernel", "centroid_legs_kernel", "canonicalise")


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
    d_code = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(2 * n, dtype=torch.int8, device="cuda")
    d_z = torch.empty(n, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    us_co = timed(lambda: p.centroid_map_device(d_code.data_ptr(), d_off.data_ptr(), 0, stream=s.cuda_stream), s, calls, warmup)
    us_all = timed(lambda: p.centroid_map_device(d_code.data_ptr(), d_off.data_ptr(), d_z.data_ptr(), stream=s.cuda_stream), s,
                   calls, warmup)
    code = d_code.cpu().numpy()
    off = d_off.cpu().numpy().reshape(n, 2).astype(np.int64)
    z = d_z.cpu().numpy()
    # the queries of every cell centre, built on the host once: getPosition = base - res * index
    x0 = 0.0 + (0.5 * (rows * res) - 0.5 * res)  # getPosition's base at map position (0, 0) (fpe_gridmath.hpp make_geom)
    ii, jj = np.meshgrid(np.arange(rows), np.arange(rows), indexing="ij")
    q = np.zeros(n, dtype=_capi.CENTROID_QUERY_DTYPE)
    q["cx"] = (x0 + res * -ii.astype(np.float64)).ravel()
    q["cy"] = (x0 + res * -jj.astype(np.float64)).ravel()
    d_q = torch.from_numpy(q.view(np.uint8)).cuda()
    d_f = torch.empty(n * _capi.CENTROID_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    us_legs = timed(lambda: p.centroid_legs_device(d_q.data_ptr(), n, d_f.data_ptr(), stream=s.cuda_stream), s, legs_calls, 1)
    f = d_f.cpu().numpy().view(_capi.CENTROID_DTYPE)
    assert np.array_equal(f["code"], code), "dense code != centroid_legs code"
    mv = (code >= 1) & (code <= 4)
    assert np.array_equal(f["row"][mv] - ii.ravel()[mv], off[mv, 0]) and np.array_equal(f["col"][mv] - jj.ravel()[mv], off[mv, 1])
    assert np.all(off[~mv] == 0)
    assert np.array_equal(f["z"].view(np.uint32), z.view(np.uint32)), "dense z != centroid_legs z"
    frac = " ".join(f"{float(np.mean(code == k)):.3f}" for k in range(7))
    p.close()
    print(f"{config}: {rows}x{rows} cells, codes 0-6 = {frac}; per call (device events): "
          f"dense code+offset {us_co:.1f} us, dense +z {us_all:.1f} us, centroid_legs_device {us_legs:.1f} us "
          f"-> {us_legs / us_co:.1f}x")


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
