"""fpe_plan_rank at the headline shape (1000^2 @ 2 cm, B 4096, 8 cycles): the workload of the kernel-trace profile and the host-call
comparison of profiles/plan_rank_summary.txt.

    python3 profiles/probe_plan_rank.py --host --calls 200
        for K = 16 and K = 1024: the host call fpe_plan_rank with pinned destinations and best_products = {nominal, cycle_ok,
        stance} (once without and once with the B-sized summary and score) against fpe_plan with all seven products (pinned) and
        with selected_packed only (pinned) — ONE process, the four calls alternating, wall-clock per call, median and p10 / p90;
    python3 profiles/probe_plan_rank.py --device --k 16 --calls 50
        queues the device form back to back on one stream (the run rocprofv3 --kernel-trace --stats wraps);
    python3 profiles/probe_plan_rank.py --summarise DIR
        reads DIR/k<K>/**/*kernel_stats.csv of collect_plan_rank.sh and prints microseconds per kernel.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (16, 1024)
KERNELS = ("plan_bits_kernel", "rank_summary_kernel", "rank_select_kernel", "rank_gather_kernel")


def setup():
    from quadrupedal_foothold_planner_amd import synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

    trav, elev, res, poses, n, _ = synth.make_config("headline")
    p = FootholdPlanner(0)
    p.gridmapCallback(trav, elev, res)
    return p, poses, n


def host(calls, warmup):
    import numpy as np

    from quadrupedal_foothold_planner_amd import _capi
    from quadrupedal_foothold_planner_amd.planner import PRODUCT_FIELDS, product_shapes

    p, poses, n = setup()
    B = poses.shape[0]
    print(f"headline: B {B}, {n} cycles, {p.describe_plan()}")
    full = p.plan_outputs(B, n, pinned=True)
    packed = p.plan_outputs(B, n, products=("selected_packed",), pinned=True)
    for K in KS:
        shapes = product_shapes(K, n)
        wanted = ("nominal", "cycle_ok", "stance")
        best = p.host_array((K,), np.int32)
        n0 = p.host_array((1,), np.int32)
        prods = {k: p.host_array(*shapes[k]) for k in wanted}
        summary, score = p.host_array((B,), _capi.POSE_SUMMARY_DTYPE), p.host_array((B,), np.float64)
        ro = _capi.RankOut(None, None, _capi.ptr(best), _capi.ptr(n0))
        for k in wanted:
            setattr(ro.best_products, PRODUCT_FIELDS[k], _capi.ptr(prods[k]))
        ro_s = _capi.RankOut(_capi.ptr(summary), _capi.ptr(score), _capi.ptr(best), _capi.ptr(n0))
        for k in wanted:
            setattr(ro_s.best_products, PRODUCT_FIELDS[k], _capi.ptr(prods[k]))
        pp, dp = _capi.ptr(p.params), _capi.ptr(poses)

        def rank_call(r):
            assert p._lib.fpe_plan_rank(p._h, pp, None, dp, B, n, K, C.byref(r)) == 0

        runs = {
            "fpe_plan_rank (K products, no summary)": lambda: rank_call(ro),
            "fpe_plan_rank (K products + summary + score)": lambda: rank_call(ro_s),
            "fpe_plan all seven products": lambda: p.plan(poses, n, out=full),
            "fpe_plan selected_packed only": lambda: p.plan(poses, n, out=packed),
        }
        times = {k: [] for k in runs}
        for it in range(warmup + calls):
            for name, fn in runs.items():  # alternating: drift hits all four alike
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if it >= warmup:
                    times[name].append(dt * 1e6)
        again = p.plan(poses[best], n, products=wanted)
        for k in wanted:
            assert np.array_equal(prods[k].view(np.uint8), again[k].view(np.uint8)), k
        for name, t in times.items():
            t = np.sort(np.array(t))
            print(f"K {K:5d}  {name:46s} median {np.median(t):8.1f} us  p10 {t[len(t) // 10]:8.1f}  p90 {t[(9 * len(t)) // 10]:8.1f}  ({len(t)} calls)")
    p.close()


def device(K, calls):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi
    from quadrupedal_foothold_planner_amd.planner import product_shapes

    p, poses, n = setup()
    B = poses.shape[0]
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    shapes = product_shapes(K, n)
    bufs = {k: torch.empty(int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize, dtype=torch.uint8, device="cuda")
            for k in ("nominal", "cycle_ok", "stance")}
    d_best = torch.empty(K, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(calls):
            p.plan_rank_device(d_poses.data_ptr(), B, n, K, d_best.data_ptr(), best_products={k: t.data_ptr() for k, t in bufs.items()},
                               stream=s.cuda_stream)
    s.synchronize()
    p.close()
    print(f"K {K}: {calls} device-form calls queued and complete")


def summarise(directory):
    print(f"{'run':8s} {'kernel':24s} {'calls':>6s} {'us/call':>9s}")
    for K in KS:
        files = glob.glob(os.path.join(directory, f"k{K}", "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print(f"k{K}: no kernel_stats.csv (not measured)")
            continue
        with open(files[0]) as fh:
            for r in csv.DictReader(fh):
                name = next((k for k in KERNELS if k in r["Name"]), None)
                if name is not None:
                    print(f"k{K:<7d} {name:24s} {int(r['Calls']):6d} {float(r['AverageNs']) / 1e3:9.1f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    elif a.device:
        device(a.k, a.calls)
    else:
        host(a.calls, a.warmup)
