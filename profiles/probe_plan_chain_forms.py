"""The stride and resume forms of the four plan-kernel families at small test rows scaled to a few thousand poses: device time per
launch, for A/B runs of two trees in one session.

    python3 profiles/probe_plan_chain_forms.py [--tree TREE] [--steps 20] [--blocks 8]
        ONE process, device events, the profiler off; blocks of --steps back-to-back launches, the variants alternating block by
        block; median / min / max of the per-launch time over the blocks, and one `medians` line to set beside another run's.
        --tree: the checkout whose package and library are loaded (default: this one).
    variants (rows of tests/test_gpu_plan_matrix.py, mixed per-pose strides as in tests/stride_reference.py):
        lane8_stride       w7_gen, B 4096, 9 cycles          fpe_plan_strides_device
        lane8_resume       w7_gen, B 4096, 9 cycles          fpe_plan_resume_device, strides, state_in (after 4 cycles) and state_out
        chained_stride     the same call as lane8_stride under no_bits = 1    (plan_chained_kernel<8, false> stride)
        sequential_resume  the same call as lane8_resume, B 1024, under plan_group = 65   (plan_sequential_kernel resume)
        seq_resume         w16_seq, B 1024, 5 cycles         fpe_plan_resume_device as above (plan_bits_seq_kernel<1, 2> resume)
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from quadrupedal_foothold_planner_amd._capi import PLAN_STATE_DTYPE  # noqa: E402
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, product_shapes  # noqa: E402
from tests import stride_reference as sref  # noqa: E402
from tests.test_gpu_plan_matrix import ROWS, row_inputs  # noqa: E402

PRODUCTS = ("nominal", "centroid", "default", "cycle_ok")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Case:
    def __init__(self, p, row_id, B, n, seed):
        self.p, self.row, self.B, self.n = p, ROWS[row_id], B, n
        self.params = sref.row_params(self.row)
        self.trav, self.elev, poses = row_inputs(self.row, B, seed, "seq" in self.row.kernel)
        self.poses, self.strides = dev(poses), dev(sref.mixed_strides(self.params, B, seed + 1))
        shapes = product_shapes(B, n)
        self.out = {k: torch.empty(int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize, dtype=torch.uint8, device="cuda") for k in PRODUCTS}
        self.state0 = torch.zeros(B * PLAN_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self.state1 = torch.zeros_like(self.state0)

    def use(self):
        self.p.params = self.params.copy()
        self.p.set_max_leg_search_radius(float(self.row.maxleg or 0.0))
        self.p.gridmapCallback(self.trav, self.elev, self.row.res)

    def stride(self, s, B=None):
        o = self.out
        self.p.plan_device(self.poses.data_ptr(), B or self.B, self.n, o["nominal"].data_ptr(), o["centroid"].data_ptr(), o["default"].data_ptr(),
                           o["cycle_ok"].data_ptr(), stream=s.cuda_stream, d_strides_ptr=self.strides.data_ptr())

    def resume(self, s, B=None, first=False):
        ptrs = {k: t.data_ptr() for k, t in self.out.items()}
        if first:  # four cycles from the poses: the state every timed call resumes from
            self.p.plan_resume_device(self.poses.data_ptr(), B or self.B, 4, ptrs, 0, self.state0.data_ptr(), self.strides.data_ptr(), s.cuda_stream)
        else:
            self.p.plan_resume_device(self.poses.data_ptr(), B or self.B, self.n, ptrs, self.state0.data_ptr(), self.state1.data_ptr(),
                                      self.strides.data_ptr(), s.cuda_stream)


def main():
    p = FootholdPlanner(0)
    s = torch.cuda.Stream()
    w7, w16 = Case(p, "w7_gen", 4096, 9, 9100), Case(p, "w16_seq", 1024, 5, 9200)
    # (name, case, tuning knobs, batch, call)
    variants = [("lane8_stride", w7, {}, 4096, Case.stride), ("lane8_resume", w7, {}, 4096, Case.resume),
                ("chained_stride", w7, {"no_bits": 1}, 4096, Case.stride), ("sequential_resume", w7, {"plan_group": 65}, 1024, Case.resume),
                ("seq_resume", w16, {}, 1024, Case.resume)]
    times = {v[0]: [] for v in variants}
    names = {}

    def block(case, knobs, B, call, steps):
        with p.tuning(**knobs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                for _ in range(steps):
                    call(case, s, B)
                e1.record(s)
            s.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3  # us per launch

    for case in (w7, w16):  # one map at a time: every variant of a case, warm-up first, then the alternating blocks
        case.use()
        mine = [v for v in variants if v[1] is case]
        for name, _, knobs, B, call in mine:
            with p.tuning(**knobs):
                names[name] = p.describe_plan(strides=True, resume=call is Case.resume)
                if call is Case.resume:
                    case.resume(s, B, first=True)
                    s.synchronize()
            for _ in range(2):
                block(case, knobs, B, call, args.steps)
        for _ in range(args.blocks):
            for name, _, knobs, B, call in mine:
                times[name].append(block(case, knobs, B, call, args.steps))
    p.close()
    print(f"tree {os.path.abspath(args.tree)}: {args.blocks} blocks of {args.steps} launches per variant, device events, us per launch")
    for name, case, _, B, _ in variants:
        t = np.array(times[name])
        print(f"  {name:18s} median {np.median(t):9.2f}  min {t.min():9.2f}  max {t.max():9.2f}   {case.row.id}, B {B}, {case.n} cycles: {names[name]}")
    print("medians " + " ".join(f"{name}={np.median(np.array(times[name])):.2f}" for name, *_ in variants))


if __name__ == "__main__":
    main()
