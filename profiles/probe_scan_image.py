"""Scan images (fpe_scan_*_image*) against the point forms on profiles/probe_scan.py's workloads: a 1000 x 1000 map at 2 cm with a
300 x 300 roi, the 640 x 480 depth image as uint16 millimetres and the 64 x 2048 lidar sweep as a spherical float range image; the state
is what two fuses of the same scan left.  The point forms get the image's own points (fpe_scan_image_points), so both sides do the same
work downstream of the points; they are untouched code and the yardstick.

    python3 profiles/probe_scan_image.py [--steps 10] [--blocks 6]
        ONE process, the profiler off; device events around blocks of --steps back-to-back calls on one stream; the variants alternate
        block by block; median / min / max over the blocks of the time per call, in us.
          fuse points / fuse image        fpe_scan_fuse_device against fpe_scan_fuse_image_device
          clear points / clear image      fpe_scan_clear_device against fpe_scan_clear_image_device (the default form of the ray pass)
          ingest points / ingest image    fpe_scan_ingest_closed_device against fpe_scan_ingest_image_device with cp and kp
          host fuse points / image        fpe_scan_fuse against fpe_scan_fuse_image by wall clock (the upload is part of the call)
    python3 profiles/probe_scan_image.py --trace
        a few calls of each device form, for `rocprofv3 --kernel-trace --stats`; `--passes TRACE_DIR` prints the point passes per sensor
        from the trace (no GPU)."""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from probe_scan import N, RES, ROI, depth_points, ground, lidar_points, stats  # noqa: E402


def depth_image(width=640, height=480, focal=500.0):
    """probe_scan.depth_points as a uint16 image of millimetres (beyond 65.535 m: the largest value, which the range test drops)."""
    import numpy as np

    T, pts = depth_points(width=width, height=height, focal=focal)
    raw = np.clip(np.rint(pts[:, 2].astype(np.float64) * 1000.0), 1, 65535).astype(np.uint16).reshape(height, width)
    kw = dict(model="pinhole", format="u16", width=width, height=height, depth_scale=0.001, fx=focal, fy=focal, cx=0.5 * (width - 1), cy=0.5 * (height - 1))
    return T, kw, raw


def lidar_image(cam_z=1.0, rings=64, columns=2048):
    """probe_scan.lidar_points as a float range image with its two direction tables."""
    import numpy as np

    T, _ = lidar_points(cam_z, rings, columns)
    el = np.deg2rad(np.linspace(-30.0, -2.0, rings))[:, None]
    az = np.linspace(-np.pi, np.pi, columns, endpoint=False)[None, :]
    r = cam_z / np.sin(-el)
    for _ in range(2):
        r = (cam_z - ground(r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az))) / np.sin(-el)
    kw = dict(model="spherical", format="f32", width=columns, height=rings, depth_scale=1.0,
              row_dir=np.stack([np.cos(el[:, 0]), np.sin(el[:, 0])], 1).astype(np.float32), col_dir=np.stack([np.cos(az[0]), np.sin(az[0])], 1).astype(np.float32))
    return T, kw, np.ascontiguousarray(r.astype(np.float32))


def passes(trace_dir):
    """The point passes' kernel times per sensor from a kernel trace (grids: 307 200 depth, 131 072 lidar)."""
    import csv
    import glob
    import statistics

    rows = []
    for f in glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    times = {}
    for r in rows:
        name = r["Kernel_Name"].replace("fpe::", "").replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if name.startswith(("scan_top", "scan_sum", "scan_clear_rays_lane")):  # (the default ray pass: a lane per ray, the points' grid)
            sensor = {"307200": "depth", "131072": "lidar"}.get(r["Grid_Size_X"], r["Grid_Size_X"])
            times.setdefault((sensor, name), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (sensor, name), t in sorted(times.items()):
        print(f"{sensor:8s} {name:60s} calls {len(t):3d}  median {statistics.median(t):8.2f} us  min {min(t):8.2f}  max {max(t):8.2f}")


def main(a):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd.planner import (FootholdPlanner, make_poses, make_scan, make_scan_image, scan_clear_params, scan_close_params,
                                                          scan_image_points, scan_params)

    p = FootholdPlanner(0)
    st = p.scan_state(N, N, RES)
    sp, cp, kp = scan_params(max_range=40.0, min_z=-2.0, max_z=3.0), scan_clear_params(), scan_close_params()
    s = torch.cuda.Stream()
    d_info, d_cinfo, d_kinfo = (torch.zeros(16, dtype=torch.int32, device="cuda") for _ in range(3))
    print(f"--- {N} x {N} @ {RES} m, roi {ROI}; {a.blocks} blocks of {a.steps} calls per variant; device events, us per call")
    for name, (T, kw, image) in {"depth": depth_image(), "lidar": lidar_image()}.items():
        im_host = make_scan_image(**kw)
        pts = scan_image_points(im_host, image)
        n = len(pts)
        scan = make_scan(T, n, ROI)
        d_pts = torch.from_numpy(pts).cuda()
        d_img = torch.from_numpy(image.view(np.uint8).reshape(-1).copy()).cuda()
        tables = [torch.from_numpy(kw[k]).cuda() if kw.get(k) is not None else None for k in ("row_dir", "col_dir")]
        im = make_scan_image(**dict(kw, row_dir=tables[0].data_ptr() if tables[0] is not None else None,
                                    col_dir=tables[1].data_ptr() if tables[1] is not None else None))
        unknown = np.full((N, N), np.nan, np.float32)
        st.set_layers(unknown, unknown)
        torch.cuda.synchronize()
        infos = []
        for form in ("points", "image", "image"):  # the two forms' first fuse must agree; two image fuses leave the state
            if form == "points":
                st.fuse_device(scan, d_pts.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)
            else:
                st.fuse_image_device(scan, im, d_img.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            infos.append(d_info.cpu().numpy().tolist())
            if len(infos) == 1:
                st.set_layers(unknown, unknown)
        print(f"{name}: {n} points, image {image.nbytes} bytes against {pts.nbytes} bytes of points; info of the first fuse {infos[0]}")
        assert infos[0] == infos[1], (infos[0], infos[1])
        st.install_closed(kp, stream=s.cuda_stream)
        s.synchronize()
        p.foothold_map(roi=(0, 0, 8, 8), products=("flags",))
        p.plan(make_poses([[0.0, 0.0, 0.0]]), 1)

        def fuse_points():
            st.fuse_device(scan, d_pts.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)

        def fuse_image():
            st.fuse_image_device(scan, im, d_img.data_ptr(), sp, d_info.data_ptr(), stream=s.cuda_stream)

        def clear_points():
            st.clear_device(scan, d_pts.data_ptr(), sp, cp, d_cinfo.data_ptr(), stream=s.cuda_stream)

        def clear_image():
            st.clear_image_device(scan, im, d_img.data_ptr(), sp, cp, d_cinfo.data_ptr(), stream=s.cuda_stream)

        def ingest_points():
            st.ingest_closed_device(scan, d_pts.data_ptr(), (0, 0), (0.0, 0.0), sp, cp, kp, d_clear_info_ptr=d_cinfo.data_ptr(), d_info_ptr=d_info.data_ptr(),
                                    d_close_info_ptr=d_kinfo.data_ptr(), stream=s.cuda_stream)

        def ingest_image():
            st.ingest_image_device(scan, im, d_img.data_ptr(), (0, 0), (0.0, 0.0), sp, cp, kp, d_clear_info_ptr=d_cinfo.data_ptr(), d_info_ptr=d_info.data_ptr(),
                                   d_close_info_ptr=d_kinfo.data_ptr(), stream=s.cuda_stream)

        def block(fn, steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                for _ in range(steps):
                    fn()
                e1.record(s)
            s.synchronize()
            return e0.elapsed_time(e1) / steps * 1e3

        variants = {"fuse points": fuse_points, "fuse image": fuse_image, "clear points": clear_points, "clear image": clear_image,
                    "ingest points": ingest_points, "ingest image": ingest_image}
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
            print(f"  {q:18s} {stats(times[q])}")
        for what in ("fuse", "clear", "ingest"):
            print(f"  {what}: image / points {med[what + ' image'] / med[what + ' points']:.3f}")

        # the host forms by wall clock: the upload of the points or of the image is part of the call
        def wall(fn):
            t = []
            for _ in range(a.blocks * 2):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                t.append((time.perf_counter() - t0) / a.steps * 1e6)
            return t

        host = {"host fuse points": lambda: st.fuse(scan, pts, sp), "host fuse image": lambda: st.fuse_image(scan, im_host, image, sp)}
        for fn in host.values():
            fn()
        ht = {q: [] for q in host}
        for _ in range(2):
            for q, fn in host.items():
                ht[q] += wall(fn)
        for q in host:
            print(f"  {q:18s} {stats(ht[q])}   (wall clock)")
        print(f"  host fuse: image / points {np.median(ht['host fuse image']) / np.median(ht['host fuse points']):.3f}")
    st.close()
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--passes", metavar="TRACE_DIR", help="no GPU: the point passes' kernel times of a kernel trace taken with --trace")
    a = ap.parse_args()
    passes(a.passes) if a.passes else main(a)
