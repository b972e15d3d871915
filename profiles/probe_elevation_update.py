"""Elevation-driven map updates (fpe_update_elevation_device) against the path they replace on the same tree — the full filter
chain over the whole composed elevation (fpe_traversability_device) followed by fpe_upload_map_device — for a robot-centric map:

    python3 profiles/probe_elevation_update.py [--steps 10] [--blocks 8] [--sizes 1000,2000]
        ONE process, the profiler off, the variants alternating block by block (drift hits all alike); device events around blocks
        of --steps back-to-back calls on one stream; median / min / max over the blocks of the time per call.
        Per size (1000 x 1000 @ 2 cm, 2000 x 2000 @ 1 cm), two updates:
          move   shift (5, 3), the two exposed bands as elevation patches (device arrays)
          dot    no shift, one 1 x 1 patch in the middle of the map
        and for each the variants
          update   fpe_update_elevation_device
          full     fpe_traversability_device on the composed elevation (no layer buffer) + fpe_upload_map_device of both layers
        One threshold pair is in the snapshots' history: both routes rebuild its planes.  recomputed_cells / cells is reported."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MOVE = (5, 3)


def compose(a, shift, nan):
    """The layer shifted by whole cells, the cells without a source cleared (numpy, vectorised)."""
    import numpy as np

    rows, cols = a.shape
    sr, sc = shift
    out = np.full_like(a, nan)
    out[max(0, -sr):rows - max(0, sr), max(0, -sc):cols - max(0, sc)] = a[max(0, sr):rows + min(0, sr), max(0, sc):cols + min(0, sc)]
    return out


def stats(t):
    import numpy as np

    t = np.array(t)
    return f"median {np.median(t):10.2f}  min {t.min():10.2f}  max {t.max():10.2f}"


def run_size(n, res, a):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, filter_reach_cells, make_poses

    _, elev = synth.rough_map(n, n, res, seed=11)
    _, other = synth.rough_map(n, n, res, seed=12)
    p = FootholdPlanner(0)
    trav = p.traversability_from_elevation(elev, res)
    p.gridmapCallback(trav, elev, res)
    # one pair in the history (a dense call and a plan with the yaml thresholds): every later snapshot gets its planes
    p.foothold_map(roi=(0, 0, 8, 8), products=("flags",))
    p.plan(make_poses([[0.0, 0.0, 0.0]]), 1)
    s = torch.cuda.Stream()
    cells = n * n
    print(f"--- {n} x {n} @ {res} m ({cells} cells), {a.blocks} blocks of {a.steps} calls per variant; reach {filter_reach_cells(res)} cells")
    cases = {"move": (MOVE, [(n - MOVE[0], 0, MOVE[0], n), (0, n - MOVE[1], n - MOVE[0], MOVE[1])]), "dot": ((0, 0), [(n // 2, n // 2, 1, 1)])}
    for name, (shift, rects) in cases.items():
        pos = (-shift[0] * res, -shift[1] * res)
        new_e = compose(elev, shift, np.float32(np.nan))
        d_patches, keep = [], []
        for r0, c0, nr, nc in rects:
            pe = np.ascontiguousarray(other[r0:r0 + nr, c0:c0 + nc])
            new_e[r0:r0 + nr, c0:c0 + nc] = pe
            de = torch.from_numpy(pe.reshape(-1)).cuda()
            keep.append(de)
            d_patches.append((r0, c0, nr, nc, de.data_ptr(), nc, 1))
        d_new_e = torch.from_numpy(new_e.reshape(-1)).cuda()
        d_new_t = torch.empty(cells, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        info = {}

        def update():
            info.update(p.update_elevation_device(shift, pos, d_patches, stream=s.cuda_stream))

        def full():
            p.traversability_device(d_new_e.data_ptr(), d_new_t.data_ptr(), n, n, res, position=pos, stream=s.cuda_stream)
            p.upload_map_device(d_new_t.data_ptr(), d_new_e.data_ptr(), n, n, res, position=pos, stream=s.cuda_stream)

        def block(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                for _ in range(a.steps):
                    fn()
                e1.record(s)
            s.synchronize()
            return e0.elapsed_time(e1) / a.steps * 1e3  # us per call

        variants = {"update": update, "full": full}
        for fn in variants.values():
            for _ in range(2):
                block(fn)
        times = {q: [] for q in variants}
        for _ in range(a.blocks):
            for q, fn in variants.items():
                times[q].append(block(fn))
        med = {q: float(np.median(times[q])) for q in variants}
        share = info["recomputed_cells"] / cells
        print(f"{name}: shift {shift}, {len(rects)} patches; route {info['route']}, dirty {info['dirty_cells']} cells, recomputed {info['recomputed_cells']} "
              f"= {100.0 * share:.2f} % of the map; device events, us per call")
        for q in variants:
            print(f"  {q:8s} {stats(times[q])}")
        print(f"  ratio update / full {med['update'] / med['full']:.4f}   (recomputed share {share:.4f})")
        del keep
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--sizes", default="1000,2000")
    a = ap.parse_args()
    for n in map(int, a.sizes.split(",")):
        run_size(n, 0.02 if n <= 1000 else 0.01, a)
