"""Scan gap closing (fpe_scan_close_device) on profiles/probe_scan.py's depth workload: a 1000 x 1000 map at 2 cm with a 300 x 300
roi and a 640 x 480 depth image; the state is what two fuses of that scan left; the close's parameters are the defaults (reach 4), its
rectangle is the one an ingest closes (the roi grown by the reach: 308 x 308 cells), and the whole map as fpe_scan_install_closed does.

    python3 profiles/probe_scan_close.py [--steps 10] [--blocks 6]
        ONE process, the profiler off; device events around blocks of --steps back-to-back calls on one stream; the variants alternate
        block by block; median / min / max over the blocks of the time per call, in us.
          close direct / tiled            fpe_scan_close_device of the ingest's rectangle under scan_close_form 1 and 2 (no class bytes)
          close whole direct / tiled      the same over the whole map
          stream                          the yardstick (profiles/scan_yardstick.hip) over as many lanes as the rectangle has cells: 4 new
                                          bytes read and 8 written per lane
          fuse                            fpe_scan_fuse_device, the engine's default form (code this probe's subject does not touch)
          ingest_clear / ingest_closed    fpe_scan_ingest_clear_device and fpe_scan_ingest_closed_device with the same clear parameters
    python3 profiles/probe_scan_close.py --trace
        a few calls of each, for `rocprofv3 --kernel-trace --stats`; `--passes TRACE_DIR` prints the close's kernels from the trace (no
        GPU)."""
import argparse
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from probe_scan import N, RES, ROI, depth_points, stats  # noqa: E402

REACH = 4
RECT = (ROI[0] - REACH, ROI[1] - REACH, ROI[2] + 2 * REACH, ROI[3] + 2 * REACH)
WHOLE = (0, 0, N, N)


def passes(trace_dir):
    """The close's kernel times from a kernel trace, by kernel and grid size."""
    import csv
    import glob
    import statistics

    times = {}
    for f in glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].replace("(anonymous namespace)", "").split("(")[0].split("::")[-1]
            if name.startswith("scan_close"):
                key = (name, int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]))
                times.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, lanes), t in sorted(times.items()):
        print(f"{name:28s} {lanes:8d} lanes  calls {len(t):3d}  median {statistics.median(t):9.2f} us  min {min(t):9.2f}  max {max(t):9.2f}")


def main(a):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_poses, make_scan, scan_clear_params, scan_close_params, scan_params

    yard = C.CDLL(os.path.join(HERE, "_build", "libscan_yardstick.so"))  # built by collect_scan_close.sh
    yard.scan_yardstick.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    p = FootholdPlanner(0)
    st = p.scan_state(N, N, RES)
    sp, cp, kp = scan_params(max_range=40.0, min_z=-2.0, max_z=3.0), scan_clear_params(), scan_close_params()
    s = torch.cuda.Stream()
    d_info, d_cinfo, d_kinfo = (torch.zeros(16, dtype=torch.int32, device="cuda") for _ in range(3))
    d_out = torch.zeros(N * N, dtype=torch.float32, device="cuda")
    cells = RECT[2] * RECT[3]
    d_src, d_rec = torch.zeros(cells + 2, dtype=torch.float32, device="cuda"), torch.zeros(2 * cells, dtype=torch.int32, device="cuda")
    T, pts = depth_points()
    n = len(pts)
    scan = make_scan(T, n, ROI)
    d_pts = torch.from_numpy(pts).cuda()
    unknown = np.full((N, N), np.nan, np.float32)
    st.set_layers(unknown, unknown)
    torch.cuda.synchronize()
    for _ in range(2):
        st.fuse_device(scan, d_pts.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)
    st.install_closed(kp, stream=s.cuda_stream)
    s.synchronize()
    p.foothold_map(roi=(0, 0, 8, 8), products=("flags",))
    p.plan(make_poses([[0.0, 0.0, 0.0]]), 1)
    print(f"--- {N} x {N} @ {RES} m, roi {ROI}, rectangle {RECT} ({cells} cells); {n} points; {a.blocks} blocks of {a.steps} calls per variant; device events, us per call")
    for name, rect in (("rectangle", RECT), ("whole map", WHOLE)):
        st.close_gaps_device(rect, d_out.data_ptr(), rect[3], kp, 0, d_kinfo.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        ki = np.frombuffer(d_kinfo.cpu().numpy().tobytes(), _capi.SCAN_CLOSE_INFO_DTYPE)[0]
        print(f"{name}: {dict(zip(ki.dtype.names[:7], ki.tolist()[:7]))}")

    def close(form, rect):
        def run():
            st.close_gaps_device(rect, d_out.data_ptr(), rect[3], kp, 0, d_kinfo.data_ptr(), stream=s.cuda_stream)
        run.tuning = dict(scan_close_form=form)
        return run

    def stream():
        assert yard.scan_yardstick(d_src.data_ptr(), 1, cells, d_rec.data_ptr(), s.cuda_stream) == 0

    def fuse():
        st.fuse_device(scan, d_pts.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)

    def ingest_clear():
        st.ingest_clear_device(scan, d_pts.data_ptr(), (0, 0), (0.0, 0.0), sp, cp, d_clear_info_ptr=d_cinfo.data_ptr(), d_info_ptr=d_info.data_ptr(),
                               stream=s.cuda_stream)

    def ingest_closed():
        st.ingest_closed_device(scan, d_pts.data_ptr(), (0, 0), (0.0, 0.0), sp, cp, kp, d_clear_info_ptr=d_cinfo.data_ptr(), d_info_ptr=d_info.data_ptr(),
                                d_close_info_ptr=d_kinfo.data_ptr(), stream=s.cuda_stream)

    def block(fn, steps):
        p.set_tuning(**getattr(fn, "tuning", dict(scan_close_form=0)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(steps):
                fn()
            e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3

    variants = {"close direct": close(1, RECT), "close tiled": close(2, RECT), "close whole direct": close(1, WHOLE), "close whole tiled": close(2, WHOLE),
                "stream": stream, "fuse": fuse, "ingest_clear": ingest_clear, "ingest_closed": ingest_closed}
    if a.trace:
        for fn in variants.values():
            block(fn, 3)
    else:
        for fn in variants.values():
            block(fn, 2)
        times = {q: [] for q in variants}
        for _ in range(a.blocks):
            for q, fn in variants.items():
                times[q].append(block(fn, a.steps))
        med = {q: float(np.median(times[q])) for q in variants}
        for q in variants:
            print(f"  {q:18s} {stats(times[q])}")
        best = min(("close direct", "close tiled"), key=lambda q: med[q])
        print(f"  fastest close: {best}; {best} / stream {med[best] / med['stream']:.2f}; {best} / fuse {med[best] / med['fuse']:.2f}; "
              f"ingest_closed - ingest_clear {med['ingest_closed'] - med['ingest_clear']:.2f} us = "
              f"{(med['ingest_closed'] - med['ingest_clear']) / med['ingest_closed']:.3f} of an ingest_closed")
    p.set_tuning(scan_close_form=0)
    st.close()
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--passes", metavar="TRACE_DIR", help="no GPU: the close's kernel times of a kernel trace taken with --trace")
    a = ap.parse_args()
    passes(a.passes) if a.passes else main(a)
