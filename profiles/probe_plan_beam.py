"""Beam search over stride options (fpe_plan_beam_device) on the headline map: what the beam's own kernels — expand, score,
select, keep, trace — cost on top of the resume launches they sit between.

    python3 profiles/probe_plan_beam.py [--steps 20] [--blocks 12] [--roots 64 --width 8 --options 8 --segments 4 --cycles 2]
        ONE process, device events, the profiler off; blocks of --steps back-to-back calls, the variants alternating block by block
        (drift hits all alike), median / min / max of the per-call time over the blocks:
          beam      fpe_plan_beam_device: nominal and cycle_ok requested, path, score, penalty, state and n_live written
          resume    the same S fpe_plan_resume_device launches ALONE, at the beam's chain counts (B * M, then B * W * M), each with
                    strides, state_in (from the second launch on: the chains' cycle-0 states, so every launch plans inside the map)
                    and state_out, writing nominal, default and cycle_ok — what the beam's plan calls write
        and the ratio beam / resume: the cost of the beam's own kernels, explained per kernel by the --trace run.
    python3 profiles/probe_plan_beam.py --beam-only --steps 5 --blocks 1
        the beam call alone (run under rocprofv3 --kernel-trace --stats for the per-kernel split).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(a):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi, synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_plan_states, make_strides, product_shapes

    trav, elev, res, poses, _, _ = synth.make_config("headline")
    p = FootholdPlanner(0)
    p.gridmapCallback(trav, elev, res)
    B, W, M, S, k = a.roots, a.width, a.options, a.segments, a.cycles
    roots = poses[:B]
    step0, drift0 = float(p.params["stepLength"][0]), float(p.params["lateralDrift"][0])
    options = make_strides(step0 * np.linspace(0.6, 1.4, M), drift0 + np.linspace(-0.01, 0.01, M))
    bp = _capi.beam_params_defaults(segments=S, cycles_per_segment=k, width=W)
    live = [min(W, M ** (s + 1)) for s in range(S)]
    chains = [B * (1 if s == 0 else live[s - 1]) * M for s in range(S)]
    s = torch.cuda.Stream()

    def dev(a_):
        return torch.from_numpy(np.ascontiguousarray(a_).view(np.uint8).copy()).cuda()

    def empty(shape, dtype):
        return torch.empty(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")

    d_roots, d_options = dev(roots), dev(options)
    shapes = product_shapes(B * W, S * k)
    out = {q: empty(*shapes[q]) for q in ("nominal", "cycle_ok")}
    own = {"path": empty((B * W * S,), np.uint8), "score": empty((B * W,), np.float64), "penalty": empty((B * W,), np.float64),
           "state": empty((B * W,), _capi.PLAN_STATE_DTYPE), "n_live": empty((B,), np.int32)}

    def beam():
        p.plan_beam_device(d_roots.data_ptr(), B, d_options.data_ptr(), M, own["path"].data_ptr(), beam=bp, d_n_live_ptr=own["n_live"].data_ptr(),
                           d_score_ptr=own["score"].data_ptr(), d_penalty_ptr=own["penalty"].data_ptr(), d_state_ptr=own["state"].data_ptr(),
                           products={q: out[q].data_ptr() for q in out}, stream=s.cuda_stream)

    variants = {"beam": (f"B {B} roots, W {W}, M {M}, S {S}, k {k}: chains per segment {chains}", beam)}
    if not a.beam_only:
        big = max(chains)
        reps = -(-big // B)
        d_poses = dev(np.tile(roots, reps)[:big])
        d_strides = dev(np.tile(options, -(-big // M))[:big])
        d_start = dev(make_plan_states(p.params, poses=np.tile(roots, reps)[:big], strides=np.tile(options, -(-big // M))[:big]))
        d_state = empty((big,), _capi.PLAN_STATE_DTYPE)
        rs = product_shapes(big, k)
        bufs = {q: empty(*rs[q]) for q in ("nominal", "default", "cycle_ok")}
        rout = {q: bufs[q].data_ptr() for q in bufs}

        def resume():
            for seg, n in enumerate(chains):
                p.plan_resume_device(d_poses.data_ptr(), n, k, rout, d_state_in_ptr=d_start.data_ptr() if seg else 0,
                                     d_state_out_ptr=d_state.data_ptr(), d_strides_ptr=d_strides.data_ptr(), stream=s.cuda_stream)

        variants["resume"] = (f"{S} launches of {p.describe_plan(resume=True)}", resume)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(a.steps):
                fn()
            e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1e3  # us per call

    for _, fn in variants.values():  # warm-up: every kernel loaded, the memory pool grown, the device settled
        for _ in range(3):
            block(fn)
    times = {q: [] for q in variants}
    for _ in range(a.blocks):
        for q, (_, fn) in variants.items():
            times[q].append(block(fn))
    print(f"headline map, {a.blocks} blocks of {a.steps} calls per variant, device events, us per call")
    med = {}
    for q, (name, _) in variants.items():
        t = np.array(times[q])
        med[q] = float(np.median(t))
        print(f"  {q:8s} median {med[q]:9.2f}  min {t.min():9.2f}  max {t.max():9.2f}   {name}")
    if "resume" in med:
        print(f"  ratio beam / resume {med['beam'] / med['resume']:.4f}   (block spread of resume: max / min "
              f"{max(times['resume']) / min(times['resume']):.4f}, of beam {max(times['beam']) / min(times['beam']):.4f})")
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--roots", type=int, default=64)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--options", type=int, default=8)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--beam-only", action="store_true")
    run(ap.parse_args())
