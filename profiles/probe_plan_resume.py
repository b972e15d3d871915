"""Resumable plans (fpe_plan_resume_device) at the headline and the cfg-3 shape: what the resume instantiations cost against the
stride instantiations of the same kernels when both compute the same plan (a cycle-0 state, uniform strides), and what planning
in two segments costs against one call.

    python3 profiles/probe_plan_resume.py [--steps 50] [--blocks 12]
        per shape, ONE process, device events, the profiler off; blocks of --steps back-to-back launches, the variants alternating
        block by block (drift hits all alike), median / min / max of the per-launch time over the blocks; every variant writes the
        five products a continuation can return (nominal, centroid, default, cycle_ok, selected):
          resume    fpe_plan_resume_device, uniform strides, state_in = the poses' cycle-0 states, state_out given
          start     fpe_plan_resume_device, uniform strides, no state_in, state_out given   (today's prologue + the epilogue)
          stride    fpe_plan_strides_device, uniform strides                                (the stride twin of the same kernel)
          halves    (headline only) two calls of n / 2 cycles, the second one resuming the first one's state in place; per PAIR
        and the ratios resume / stride (the cost of the feature) and halves / resume (segmented planning; reported only).
    python3 profiles/probe_plan_resume.py --stride-only
        the `stride` line alone, through entry points the parent commit has: run from a checkout of the PARENT commit
        (FPE_TREE=<that checkout>) in the same shell session, this gives the yardstick to set beside.
"""
import argparse
import os
import sys

ROOT = os.environ.get("FPE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("nominal", "centroid", "default", "cycle_ok", "selected")


def run(config, steps, blocks, stride_only):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_strides, product_shapes

    trav, elev, res, poses, n, extra = synth.make_config(config)
    p = FootholdPlanner(0)
    if extra.get("search_radius"):
        p.params["searchRadius"] = np.float32(extra["search_radius"])
    p.set_max_leg_search_radius(float(extra.get("max_leg_search_radius", 0.0)))
    p.gridmapCallback(trav, elev, res)
    B = poses.shape[0]
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    strides = make_strides(np.full(B, p.params["stepLength"][0], np.float32), np.full(B, p.params["lateralDrift"][0], np.float64))
    d_strides = torch.from_numpy(strides.view(np.uint8).copy()).cuda()
    s = torch.cuda.Stream()

    def buffers(cycles):
        shapes = product_shapes(B, cycles)
        return {k: torch.empty(int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize, dtype=torch.uint8, device="cuda") for k in NAMES}

    out = buffers(n)
    ptrs = {k: out[k].data_ptr() for k in NAMES}

    def stride():
        p.plan_device(d_poses.data_ptr(), B, n, ptrs["nominal"], ptrs["centroid"], ptrs["default"], ptrs["cycle_ok"], stream=s.cuda_stream,
                      d_selected_ptr=ptrs["selected"], d_strides_ptr=d_strides.data_ptr())

    variants = {}
    if not stride_only:
        from quadrupedal_foothold_planner_amd.planner import make_plan_states

        start = make_plan_states(p.params, poses=poses)
        d_start = torch.from_numpy(start.view(np.uint8).copy()).cuda()
        d_state = torch.empty_like(d_start)
        name = p.describe_plan(resume=True)
        variants["resume"] = (name, lambda: p.plan_resume_device(d_poses.data_ptr(), B, n, ptrs, d_state_in_ptr=d_start.data_ptr(),
                                                                 d_state_out_ptr=d_state.data_ptr(), d_strides_ptr=d_strides.data_ptr(),
                                                                 stream=s.cuda_stream))
        variants["start"] = (name, lambda: p.plan_resume_device(d_poses.data_ptr(), B, n, ptrs, d_state_out_ptr=d_state.data_ptr(),
                                                                d_strides_ptr=d_strides.data_ptr(), stream=s.cuda_stream))
        if config == "headline" and n % 2 == 0:
            h = n // 2
            keep = [buffers(h), buffers(h)]  # (kept alive by the closure below)
            half = [{k: keep[i][k].data_ptr() for k in NAMES} for i in range(2)]

            def halves():
                p.plan_resume_device(d_poses.data_ptr(), B, h, half[0], d_state_in_ptr=d_start.data_ptr(), d_state_out_ptr=d_state.data_ptr(),
                                     d_strides_ptr=d_strides.data_ptr(), stream=s.cuda_stream)
                p.plan_resume_device(d_poses.data_ptr(), B, h, half[1], d_state_in_ptr=d_state.data_ptr(), d_state_out_ptr=d_state.data_ptr(),
                                     d_strides_ptr=d_strides.data_ptr(), stream=s.cuda_stream)

            variants["halves"] = (f"two calls of {h} cycles, state in place", halves)
    variants["stride"] = (p.describe_plan(strides=True), stride)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(steps):
                fn()
            e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3  # us per launch (halves: per pair)

    for _, fn in variants.values():  # warm-up: every variant's kernel loaded, the device settled
        for _ in range(3):
            block(fn)
    times = {k: [] for k in variants}
    for _ in range(blocks):
        for k, (_, fn) in variants.items():
            times[k].append(block(fn))
    print(f"{config}: B {B}, {n} cycles, {blocks} blocks of {steps} launches per variant, device events, us per launch")
    med = {}
    for k, (name, _) in variants.items():
        t = np.array(times[k])
        med[k] = float(np.median(t))
        print(f"  {k:8s} median {med[k]:9.2f}  min {t.min():9.2f}  max {t.max():9.2f}   {name}")
    if not stride_only:
        print(f"  ratio resume / stride {med['resume'] / med['stride']:.4f}   start / stride {med['start'] / med['stride']:.4f}"
              f"   (block spread of stride: max / min {max(times['stride']) / min(times['stride']):.4f})")
        if "halves" in med:
            print(f"  ratio halves / resume {med['halves'] / med['resume']:.4f}")
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--configs", default="headline,cfg3")
    ap.add_argument("--stride-only", action="store_true")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        run(cfg, a.steps, a.blocks, a.stride_only)
