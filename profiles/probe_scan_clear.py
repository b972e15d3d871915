"""Scan visibility clearing (fpe_scan_clear_device) on profiles/probe_scan.py's workloads: a 1000 x 1000 map at 2 cm with a 300 x 300
roi, a 640 x 480 depth image and a 64 x 2048 lidar sweep; the state is what two fuses of the same scan left (the steady state of a
static scene: the rays are walked, next to nothing is cleared).

    python3 profiles/probe_scan_clear.py [--steps 10] [--blocks 6]
        ONE process, the profiler off; device events around blocks of --steps back-to-back calls on one stream; the variants alternate
        block by block; median / min / max over the blocks of the time per call, in us.
          clear lane / group16 / group32 / group64   fpe_scan_clear_device under scan_clear_form 1, and 2 with each group width
          fuse                                       fpe_scan_fuse_device, the engine's default form (code this probe's subject does not touch)
          ingest / ingest_clear                      fpe_scan_ingest_device and fpe_scan_ingest_clear_device (the default forms)
    python3 profiles/probe_scan_clear.py --trace
        a few calls of each, for `rocprofv3 --kernel-trace --stats`; `--passes TRACE_DIR` prints the clear's kernels per sensor from the
        trace (no GPU)."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from probe_scan import N, RES, ROI, depth_points, lidar_points, stats  # noqa: E402

FORMS = {"clear lane": (1, 0), "clear group16": (2, 16), "clear group32": (2, 32), "clear group64": (2, 64)}


def passes(trace_dir):
    """The clear's kernel times per sensor from a kernel trace.  The sensors are told apart by the order of the run: depth first."""
    import csv
    import glob
    import statistics

    rows = []
    for f in glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    times, sensor, seen_lidar = {}, "depth", False
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)", "").split("(")[0].split("::")[-1]
        if name.startswith("scan_top") and r["Grid_Size_X"] == "131072":
            seen_lidar = True
        sensor = "lidar" if seen_lidar else "depth"
        if name.startswith("scan_clear"):
            times.setdefault((sensor, name), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (sensor, name), t in sorted(times.items()):
        print(f"{sensor:6s} {name:36s} calls {len(t):3d}  median {statistics.median(t):9.2f} us  min {min(t):9.2f}  max {max(t):9.2f}")


def main(a):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_poses, make_scan, scan_clear_params, scan_params

    p = FootholdPlanner(0)
    st = p.scan_state(N, N, RES)
    sp, cp = scan_params(max_range=40.0, min_z=-2.0, max_z=3.0), scan_clear_params()
    s = torch.cuda.Stream()
    d_info = torch.zeros(16, dtype=torch.int32, device="cuda")
    d_cinfo = torch.zeros(16, dtype=torch.int32, device="cuda")
    print(f"--- {N} x {N} @ {RES} m, roi {ROI}; {a.blocks} blocks of {a.steps} calls per variant; device events, us per call")
    for name, (T, pts) in {"depth": depth_points(), "lidar": lidar_points()}.items():
        n = len(pts)
        scan = make_scan(T, n, ROI)
        d_pts = torch.from_numpy(pts).cuda()
        unknown = np.full((N, N), np.nan, np.float32)
        st.set_layers(unknown, unknown)
        torch.cuda.synchronize()
        for _ in range(2):
            st.fuse_device(scan, d_pts.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)
        st.install(stream=s.cuda_stream)
        s.synchronize()
        p.foothold_map(roi=(0, 0, 8, 8), products=("flags",))
        p.plan(make_poses([[0.0, 0.0, 0.0]]), 1)
        for k in range(2):  # the first clear takes what the scan itself sees through; the second shows the steady state
            st.clear_device(scan, d_pts.data_ptr(), sp, cp, d_cinfo.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            ci = np.frombuffer(d_cinfo.cpu().numpy().tobytes(), _capi.SCAN_CLEAR_INFO_DTYPE)[0]
            print(f"{name}: {n} points; clear {k}: {dict(zip(ci.dtype.names, ci.tolist()))}")

        def clear(form, group):
            def run():
                st.clear_device(scan, d_pts.data_ptr(), sp, cp, d_cinfo.data_ptr(), stream=s.cuda_stream)
            run.tuning = dict(scan_clear_form=form, scan_clear_group=group)
            return run

        def fuse():
            st.fuse_device(scan, d_pts.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)

        def ingest():
            st.ingest_device(scan, d_pts.data_ptr(), (0, 0), (0.0, 0.0), sp, d_info_ptr=d_info.data_ptr(), stream=s.cuda_stream)

        def ingest_clear():
            st.ingest_clear_device(scan, d_pts.data_ptr(), (0, 0), (0.0, 0.0), sp, cp, d_clear_info_ptr=d_cinfo.data_ptr(), d_info_ptr=d_info.data_ptr(),
                                   stream=s.cuda_stream)

        def block(fn, steps):
            p.set_tuning(**getattr(fn, "tuning", dict(scan_clear_form=0, scan_clear_group=0)))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                for _ in range(steps):
                    fn()
                e1.record(s)
            s.synchronize()
            return e0.elapsed_time(e1) / steps * 1e3

        variants = {q: clear(*fg) for q, fg in FORMS.items()}
        variants.update({"fuse": fuse, "ingest": ingest, "ingest_clear": ingest_clear})
        if a.trace:
            for fn in variants.values():
                block(fn, 3)
            continue
        for fn in variants.values():
            block(fn, 2)
        times = {q: [] for q in variants}
        for _ in range(a.blocks):
            for q, fn in variants.items():
                times[q].append(block(fn, a.steps))
        med = {q: float(np.median(times[q])) for q in variants}
        for q in variants:
            print(f"  {q:14s} {stats(times[q])}")
        best = min(FORMS, key=lambda q: med[q])
        print(f"  fastest clear: {best}; {best} / fuse {med[best] / med['fuse']:.2f}; ingest_clear - ingest {med['ingest_clear'] - med['ingest']:.2f} us = "
              f"{(med['ingest_clear'] - med['ingest']) / med['ingest_clear']:.3f} of an ingest_clear")
    p.set_tuning(scan_clear_form=0, scan_clear_group=0)
    st.close()
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--passes", metavar="TRACE_DIR", help="no GPU: the clear's kernel times of a kernel trace taken with --trace")
    a = ap.parse_args()
    passes(a.passes) if a.passes else main(a)
