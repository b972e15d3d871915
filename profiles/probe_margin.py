"""The edge margin (fpe_margin_*) beside the calls it is compared with: the workload of the profile and its summary.

    python3 profiles/probe_margin.py --config headline --calls 20
        uploads the configuration's map and times, on one stream with device events around back-to-back calls after warm-up calls:
        the dense form (fpe_margin_map_device, both products, default classes) at reach 8 and reach 31 beside fpe_foothold_map_device's
        flags product on the same map in the same process; and — the headline only — fpe_margin_plan_device (records and summary) on
        the configuration's batch beside fpe_plan_device (nominal, cycle_ok, stance) and fpe_trunk_plan_device of the same batch.
        A region of the dense output and a sample of the records are checked against tests/margin_reference.py.
    python3 profiles/probe_margin.py --summarise DIR
        reads DIR/<config>/**/*kernel_trace.csv (and *counter_collection.csv, where a counter run left one) of collect_margin.sh and
        prints the median time of the margin kernels and of the kernels beside them.

Configurations (synth.make_config): "headline" 1000 x 1000 cells at 2 cm, 4 096 poses x 8 cycles; "cfg5" 4000 x 4000 cells at 0.5 cm.
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
KERNELS = ("margin_map_kernel", "margin_cells_kernel", "margin_summary_kernel", "footmap_flags_bits_kernel", "footmap_direct_kernel",
           "trunk_stances_kernel", "trunk_summary_kernel")


def run(config, calls, warmup, check):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi, synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_margin_params
    from tests import margin_reference as ref

    trav, elev, res, poses, n, extra = synth.make_config(config)
    rows, cols = trav.shape
    B = poses.shape[0]
    p = FootholdPlanner(0)
    if "search_radius" in extra:
        p.params["searchRadius"] = extra["search_radius"]
    if "max_leg_search_radius" in extra:
        p.set_max_leg_search_radius(extra["max_leg_search_radius"])
    p.gridmapCallback(trav, elev, res)
    thr = ref.thresholds(p.params)
    dev = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def timed(fn):
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

    cells = rows * cols
    d_flags, d_dist, d_near = dev(cells), dev(2 * cells), dev(2 * cells)
    t_flags = timed(lambda: p.foothold_map_device(d_flags.data_ptr(), 0, stream=s.cuda_stream))
    line = [f"{config}: {rows}x{cols} cells at {res} m; device events, {calls} back-to-back calls after {warmup}: fpe_foothold_map_device (flags) "
            f"{t_flags:.1f} us"]
    for reach in (8, 31):
        mp = make_margin_params(reach_cells=reach)
        t = timed(lambda: p.margin_map_device(d_dist.data_ptr(), d_near.data_ptr(), mp=mp, stream=s.cuda_stream))
        t_d = timed(lambda: p.margin_map_device(d_dist.data_ptr(), 0, mp=mp, stream=s.cuda_stream))
        line.append(f"fpe_margin_map_device reach {reach} (dist_sq + nearest) {t:.1f} us = {t / t_flags:.2f} x the flags, {cells / t / 1e3:.2f} G cells/s; "
                    f"dist_sq alone {t_d:.1f} us = {t_d / t_flags:.2f} x")
        if check:  # the last call's products on a corner region against the brute-force reference
            p.margin_map_device(d_dist.data_ptr(), d_near.data_ptr(), mp=mp, stream=s.cuda_stream)
            s.synchronize()
            got = d_dist.cpu().numpy().view(np.uint16).reshape(rows, cols)[:96, :160]
            want = ref.dense(trav, thr, mp, (0, 0, 96, 160))
            assert np.array_equal(got, want["dist_sq"]), "dense form differs from the reference"
            assert np.array_equal(d_near.cpu().numpy().view(np.int8).reshape(rows, cols, 2)[:96, :160], want["nearest"])
    print("; ".join(line))
    if config == "headline":
        d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
        d_nom, d_ok, d_stance = dev(B * n * 4 * _capi.FOOTHOLD_DTYPE.itemsize), dev(B * n), dev(B * 12 * 8)
        d_rec, d_sum = dev(B * n * 4 * _capi.MARGIN_RECORD_DTYPE.itemsize), dev(B * _capi.MARGIN_SUMMARY_DTYPE.itemsize)
        d_trec, d_tsum = dev(B * n * _capi.TRUNK_RECORD_DTYPE.itemsize), dev(B * _capi.TRUNK_SUMMARY_DTYPE.itemsize)
        plan = lambda: p.plan_device(d_poses.data_ptr(), B, n, d_nominal_ptr=d_nom.data_ptr(), d_cycle_ok_ptr=d_ok.data_ptr(),
                                     d_stance_ptr=d_stance.data_ptr(), stream=s.cuda_stream)
        trunk = lambda: p.trunk_plan_device(d_nom.data_ptr(), d_ok.data_ptr(), B, n, d_trec.data_ptr(), d_tsum.data_ptr(), stream=s.cuda_stream)
        t_plan, t_trunk = timed(plan), timed(trunk)
        out = [f"{config}: {B} poses x {n} cycles x 4 = {B * n * 4} records; fpe_plan_device (nominal, cycle_ok, stance) {t_plan:.1f} us, "
               f"fpe_trunk_plan_device (records + summary) {t_trunk:.1f} us"]
        for reach in (8, 31):
            mp = make_margin_params(reach_cells=reach)
            t = timed(lambda: p.margin_plan_device(d_nom.data_ptr(), B, n, d_rec.data_ptr(), d_sum.data_ptr(), mp=mp, stream=s.cuda_stream))
            out.append(f"fpe_margin_plan_device reach {reach} (records + summary) {t:.1f} us = {t / t_plan:.2f} x the plan, {t / t_trunk:.2f} x the "
                       f"trunk check, {B * n * 4 / t:.0f} M records/s")
            if check:
                rec = d_rec.cpu().numpy().view(_capi.MARGIN_RECORD_DTYPE).reshape(B, n, 4)
                nominal = d_nom.cpu().numpy().view(_capi.FOOTHOLD_DTYPE).reshape(B, n, 4)
                pick = np.linspace(0, B - 1, 64).astype(int)
                want = ref.plan_records(trav, res, thr, nominal[pick], mp)
                ref.assert_equal_records(rec[pick], want, "sampled records")
                ref.assert_equal_records(d_sum.cpu().numpy().view(_capi.MARGIN_SUMMARY_DTYPE)[pick], ref.summary_from_records(want), "their summaries")
        print("; ".join(out))
    p.close()


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
                if key == "margin_cells_kernel":
                    key += "<true>" if "<true>" in name else "<false>"
                if key:
                    t.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for key, v in sorted(t.items()):
            if key.startswith("margin_map") or key.startswith("margin_cells"):  # run() launches reach 8 first, then reach 31: halves
                for reach, part in ((8, v[:len(v) // 2]), (31, v[len(v) // 2:])):
                    print(f"{config:9s} {key + f' reach {reach}':36s} n {len(part):4d} median {statistics.median(part):9.1f} us")
            else:
                print(f"{config:9s} {key:36s} n {len(v):4d} median {statistics.median(v):9.1f} us")
        for cf in glob.glob(os.path.join(directory, config + "_counters", "**", "*counter_collection.csv"), recursive=True)[:1]:
            vals = {}
            with open(cf) as f:
                for r in csv.DictReader(f):
                    k = next((k for k in KERNELS[:3] if k in r["Kernel_Name"]), None)
                    if k:
                        vals.setdefault((k, r.get("Counter_Name")), []).append(float(r["Counter_Value"]))
            for (k, c), v in sorted(vals.items()):
                print(f"{config:9s} {k:36s} {c} median {statistics.median(v):.0f} per launch (reach 8 and 31 together)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=CONFIGS, default="headline")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the reference")
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise)
    else:
        run(a.config, a.calls, a.warmup, not a.no_check)
