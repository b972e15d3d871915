"""Trunk check of a planned batch (fpe_trunk_plan_device) beside the plan that produced it (fpe_plan_device) and beside the swing
check of the same batch (fpe_swing_plan_device): the workload of the profile and its summary.

    python3 profiles/probe_trunk_check.py --config headline --calls 20
        uploads the configuration's map, plans its batch on the device (products nominal, cycle_ok, stance: what the two checks read)
        and, on one stream with device events around back-to-back calls, times fpe_plan_device, fpe_trunk_plan_device (records and
        summary) and fpe_swing_plan_device (records and summary) on that same batch in the same process; prints the three times,
        stances per second and the member cells of a stance, and checks a sample of the records against tests/trunk_reference.py.
    python3 profiles/probe_trunk_check.py --summarise DIR
        reads DIR/<config>/**/*kernel_trace.csv (and *counter_collection.csv, where a counter run left one) of
        collect_trunk_check.sh and prints the median time of the check's two kernels and of the plan kernel.

Configurations (synth.make_config): "headline" 1000 x 1000 cells at 2 cm, 4 096 poses x 8 cycles; "cfg5" 4000 x 4000 cells at
0.5 cm, 4 096 poses x 8 cycles with mixed gaits, per-leg radii and polygons.  32 768 records each.
"""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("headline", "cfg5")
KERNELS = ("trunk_stances_kernel", "trunk_summary_kernel", "swing_segments_kernel", "swing_summary_kernel")


def run(config, calls, warmup, sample):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi, synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner
    from tests import trunk_reference as ref

    trav, elev, res, poses, n, extra = synth.make_config(config)
    B = poses.shape[0]
    p = FootholdPlanner(0)
    if "search_radius" in extra:
        p.params["searchRadius"] = extra["search_radius"]
    if "max_leg_search_radius" in extra:
        p.set_max_leg_search_radius(extra["max_leg_search_radius"])
    p.gridmapCallback(trav, elev, res)
    dev = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    d_nom, d_ok, d_stance = dev(B * n * 4 * _capi.FOOTHOLD_DTYPE.itemsize), dev(B * n), dev(B * 12 * 8)
    d_rec, d_sum = dev(B * n * _capi.TRUNK_RECORD_DTYPE.itemsize), dev(B * _capi.TRUNK_SUMMARY_DTYPE.itemsize)
    d_srec, d_ssum = dev(B * n * 4 * _capi.SWING_RECORD_DTYPE.itemsize), dev(B * _capi.SWING_SUMMARY_DTYPE.itemsize)
    s = torch.cuda.Stream()

    def timed(fn, k):
        with torch.cuda.stream(s):
            for _ in range(warmup):
                fn()
            s.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            for _ in range(k):
                fn()
            t1.record(s)
        s.synchronize()
        return t0.elapsed_time(t1) * 1e3 / k

    plan = lambda: p.plan_device(d_poses.data_ptr(), B, n, d_nominal_ptr=d_nom.data_ptr(), d_cycle_ok_ptr=d_ok.data_ptr(),
                                 d_stance_ptr=d_stance.data_ptr(), stream=s.cuda_stream)
    trunk = lambda: p.trunk_plan_device(d_nom.data_ptr(), d_ok.data_ptr(), B, n, d_rec.data_ptr(), d_sum.data_ptr(), stream=s.cuda_stream)
    swing = lambda: p.swing_plan_device(d_nom.data_ptr(), d_ok.data_ptr(), B, n, d_srec.data_ptr(), d_ssum.data_ptr(),
                                        d_stance_ptr=d_stance.data_ptr(), stream=s.cuda_stream)
    t_plan = timed(plan, calls)
    t_trunk = timed(trunk, calls)
    t_swing = timed(swing, calls)
    rec = d_rec.cpu().numpy().view(_capi.TRUNK_RECORD_DTYPE).reshape(B, n)
    summ = d_sum.cpu().numpy().view(_capi.TRUNK_SUMMARY_DTYPE)
    st = (rec["flags"] & ref.STANCE) != 0
    n_st, cells = int(st.sum()), int(rec["n_cells"][st].sum())
    assert n_st == int(summ["n_stances"].sum())
    # a sample of the records against the brute-force reference (every cell of the map per stance: a few are enough here)
    if sample:
        nominal = d_nom.cpu().numpy().view(_capi.FOOTHOLD_DTYPE).reshape(B, n, 4)
        ok = d_ok.cpu().numpy().reshape(B, n)
        grid = ref.Grid(elev, res)
        pick = np.linspace(0, B - 1, sample).astype(int)
        body = (p.params["length"][0], p.params["width"][0])
        want = ref.plan_records(grid, nominal[pick, :2], ok[pick, :2], None, body)
        ref.assert_bitwise_equal(rec[pick, :2], want, "sampled records")
    p.close()
    print(f"{config}: {trav.shape[0]}x{trav.shape[1]} cells at {res} m, {B} poses x {n} cycles = {B * n} records, {n_st} stances; "
          f"device events, back-to-back calls: fpe_plan_device (nominal, cycle_ok, stance) {t_plan:.1f} us, fpe_trunk_plan_device "
          f"(records + summary) {t_trunk:.1f} us = {t_trunk / t_plan:.2f} x the plan, fpe_swing_plan_device (records + summary) "
          f"{t_swing:.1f} us = {t_swing / t_plan:.2f} x the plan; {n_st / (t_trunk * 1e-6) / 1e6:.1f} M stances/s; "
          f"{cells / max(n_st, 1):.1f} member cells = {4.0 * cells / max(n_st, 1):.0f} B read per stance")


def summarise(directory):
    for config in CONFIGS:
        files = glob.glob(os.path.join(directory, config, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            print(f"{config}: no kernel_trace.csv (not measured)")
            continue
        t = {}
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                key = next((k for k in KERNELS if k in name), "plan kernel" if "plan_" in name else None)
                if key:
                    t.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for key, v in sorted(t.items()):
            print(f"{config:9s} {key:24s} n {len(v):4d} median {statistics.median(v):9.1f} us")
        for cf in glob.glob(os.path.join(directory, config + "_fetch", "**", "*counter_collection.csv"), recursive=True)[:1]:
            fetch = {}
            with open(cf) as f:
                for r in csv.DictReader(f):
                    if r.get("Counter_Name") == "FETCH_SIZE":
                        k = next((k for k in KERNELS[:1] if k in r["Kernel_Name"]), None)
                        if k:
                            fetch.setdefault(k, []).append(float(r["Counter_Value"]))
            for k, v in fetch.items():
                print(f"{config:9s} {k:24s} FETCH_SIZE median {statistics.median(v):.0f} KiB per launch")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=CONFIGS, default="headline")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=4, help="poses whose first records are checked against the reference (0: none)")
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    else:
        run(a.config, a.calls, a.warmup, a.sample)
