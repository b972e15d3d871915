"""Per-pose strides (fpe_plan_strides_device) at the headline and the cfg-3 shape: what the stride instantiations cost when every
stride is the parameters' own pair, i.e. when the call computes exactly what fpe_plan_device computes.

    python3 profiles/probe_plan_strides.py [--steps 50] [--blocks 12]
        per shape, ONE process, device events, the profiler off; blocks of --steps back-to-back launches, the variants alternating
        block by block (drift hits all alike), median / min / max of the per-launch time over the blocks:
          stride    fpe_plan_strides_device, uniform strides                       (the generic body + one 16-byte load per pose)
          generic   fpe_plan_device under no_mid_variant = 1                       (the same generic body, the plan's own stride)
          today     fpe_plan_device as it is launched today                        (headline: the 3x3-only MID kernel)
        and the ratios stride / generic (the cost of the feature) and stride / today (the known cost of having no MID stride form).
    python3 profiles/probe_plan_strides.py --plain-only
        the `generic` and `today` lines alone, through entry points every earlier build has: run from a checkout of the PARENT commit
        (FPE_TREE=<that checkout>) in the same shell session, this gives the parent's fpe_plan_device numbers to set beside.
"""
import argparse
import os
import sys

ROOT = os.environ.get("FPE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(config, steps, blocks, plain_only):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, product_shapes

    trav, elev, res, poses, n, extra = synth.make_config(config)
    p = FootholdPlanner(0)
    if extra.get("search_radius"):
        p.params["searchRadius"] = np.float32(extra["search_radius"])
    p.set_max_leg_search_radius(float(extra.get("max_leg_search_radius", 0.0)))
    p.gridmapCallback(trav, elev, res)
    B = poses.shape[0]
    shapes = product_shapes(B, n)
    names = ("nominal", "centroid", "default", "cycle_ok", "stance", "selected", "pose_status")
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    out = {k: torch.empty(int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize, dtype=torch.uint8, device="cuda") for k in names}
    ptrs = [out[k].data_ptr() for k in names[:5]]
    kw = dict(d_selected_ptr=out["selected"].data_ptr(), d_pose_status_ptr=out["pose_status"].data_ptr())
    s = torch.cuda.Stream()

    def plain():
        p.plan_device(d_poses.data_ptr(), B, n, *ptrs, stream=s.cuda_stream, **kw)

    variants = {}
    if not plain_only:
        from quadrupedal_foothold_planner_amd.planner import make_strides

        strides = make_strides(np.full(B, p.params["stepLength"][0], np.float32), np.full(B, p.params["lateralDrift"][0], np.float64))
        d_strides = torch.from_numpy(strides.view(np.uint8).copy()).cuda()
        variants["stride"] = (p.describe_plan(strides=True), {}, lambda: p.plan_device(d_poses.data_ptr(), B, n, *ptrs, stream=s.cuda_stream,
                                                                                      d_strides_ptr=d_strides.data_ptr(), **kw))
    with p.tuning(no_mid_variant=1):
        generic_name = p.describe_plan()
    variants["generic"] = (generic_name, {"no_mid_variant": 1}, plain)
    variants["today"] = (p.describe_plan(), {}, plain)

    def block(fn, knobs):
        with p.tuning(**knobs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                for _ in range(steps):
                    fn()
                e1.record(s)
            s.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3  # us per launch

    for _, knobs, fn in variants.values():  # warm-up: every variant's kernel loaded, the device settled
        for _ in range(3):
            block(fn, knobs)
    times = {k: [] for k in variants}
    for _ in range(blocks):
        for k, (_, knobs, fn) in variants.items():
            times[k].append(block(fn, knobs))
    print(f"{config}: B {B}, {n} cycles, {blocks} blocks of {steps} launches per variant, device events, us per launch")
    med = {}
    for k, (name, _, _) in variants.items():
        t = np.array(times[k])
        med[k] = float(np.median(t))
        print(f"  {k:8s} median {med[k]:9.2f}  min {t.min():9.2f}  max {t.max():9.2f}   {name}")
    if not plain_only:
        print(f"  ratio stride / generic {med['stride'] / med['generic']:.4f}   (block spread of generic: max / min {max(times['generic']) / min(times['generic']):.4f})")
        print(f"  ratio stride / today   {med['stride'] / med['today']:.4f}")
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--configs", default="headline,cfg3")
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        run(cfg, a.steps, a.blocks, a.plain_only)
