"""The checked beam (fpe_plan_beam_checked_device) beside the composed sequence it replaces and the unchecked beam.

    python3 profiles/probe_beam_checked.py --config headline [--steps 20] [--blocks 4] [--roots 64 --width 8 --options 8 --segments 4 --cycles 2]
        ONE process, device events, the profiler off; 3 warm-up blocks, then blocks of --steps back-to-back calls, the variants
        alternating block by block, median / min / max of the per-call time over the blocks:
          checked    fpe_plan_beam_checked_device, all three checks on, every check output requested, the lane mapping of the check
                     kernel chosen by the engine; checked_w1 / checked_w4: the same with one / four wavefronts per candidate forced
                     (fpe_set_tuning "beam_check_waves")
          composed   fpe_plan_beam_device plus S calls of fpe_check_plan_device, each on as many chains x k cycles as that segment
                     plans (unchanged code: what a caller did before — without the pruning acting on the checks); the products
                     those calls read are the candidates' own, planned ahead of the timing with fpe_plan_resume_device from the
                     survivors of checked beams of 1 .. S - 1 segments, with the feet those carried as start feet
          unchecked  fpe_plan_beam_device alone, for information
        and the ratio checked / composed beside composed's own block spread.
    python3 profiles/probe_beam_checked.py --config headline --only checked --steps 10 --blocks 2
        one variant alone (run under rocprofv3 --kernel-trace --stats for the per-kernel split).

Configurations (synth.make_config): "headline" 1000 x 1000 cells at 2 cm; "cfg5" 4000 x 4000 cells at 0.5 cm.
Launches per segment: checked 5 (expand, resume, check-and-score, select, keep) = unchecked 5; composed 6.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(a):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd import _capi, synth
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_check_params, make_strides, product_shapes

    trav, elev, res, poses, _, extra = synth.make_config(a.config)
    p = FootholdPlanner(0)
    if "search_radius" in extra:
        p.params["searchRadius"] = extra["search_radius"]
    if "max_leg_search_radius" in extra:
        p.set_max_leg_search_radius(extra["max_leg_search_radius"])
    p.gridmapCallback(trav, elev, res)
    B, W, M, S, k = a.roots, a.width, a.options, a.segments, a.cycles
    roots = poses[:B]
    step0, drift0 = float(p.params["stepLength"][0]), float(p.params["lateralDrift"][0])
    options = make_strides(step0 * np.linspace(0.6, 1.4, M), drift0 + np.linspace(-0.01, 0.01, M))
    bp = _capi.beam_params_defaults(segments=S, cycles_per_segment=k, width=W)
    checks = make_check_params(trunk=dict(ride_height=0.25), margin=dict(classes=13, reach_cells=8, min_margin=0.5 * res))
    live = [min(W, M ** (s + 1)) for s in range(S)]
    chains = [B * (1 if s == 0 else live[s - 1]) * M for s in range(S)]
    s = torch.cuda.Stream()

    def dev(a_):
        return torch.from_numpy(np.ascontiguousarray(a_).view(np.uint8).copy()).cuda()

    def empty(shape, dtype):
        return torch.zeros(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")

    d_roots, d_options = dev(roots), dev(options)
    shapes = product_shapes(B * W, S * k)
    out = {q: empty(*shapes[q]) for q in ("nominal", "cycle_ok")}
    own = {"path": empty((B * W * S,), np.uint8), "score": empty((B * W,), np.float64), "penalty": empty((B * W,), np.float64),
           "state": empty((B * W,), _capi.PLAN_STATE_DTYPE), "n_live": empty((B,), np.int32)}
    cown = {"swing": empty((B * W,), _capi.SWING_SUMMARY_DTYPE), "trunk": empty((B * W,), _capi.TRUNK_SUMMARY_DTYPE),
            "margin": empty((B * W,), _capi.MARGIN_SUMMARY_DTYPE), "base_penalty": empty((B * W,), np.float64), "hit": empty((B * W,), np.uint8),
            "feet": empty((B * W * 12,), np.float64)}

    def unchecked():
        p.plan_beam_device(d_roots.data_ptr(), B, d_options.data_ptr(), M, own["path"].data_ptr(), beam=bp, d_n_live_ptr=own["n_live"].data_ptr(),
                           d_score_ptr=own["score"].data_ptr(), d_penalty_ptr=own["penalty"].data_ptr(), d_state_ptr=own["state"].data_ptr(),
                           products={q: out[q].data_ptr() for q in out}, stream=s.cuda_stream)

    def checked():
        p.plan_beam_checked_device(d_roots.data_ptr(), B, d_options.data_ptr(), M, own["path"].data_ptr(), beam=bp, checks=checks,
                                   d_n_live_ptr=own["n_live"].data_ptr(), d_score_ptr=own["score"].data_ptr(),
                                   d_penalty_ptr=own["penalty"].data_ptr(), d_state_ptr=own["state"].data_ptr(),
                                   products={q: out[q].data_ptr() for q in out}, check_out={q: t.data_ptr() for q, t in cown.items()},
                                   stream=s.cuda_stream)

    # the composed sequence's check calls run on THE CANDIDATES' OWN products: segment s's candidates are planned once, ahead of the
    # timing, from the survivors of a checked beam of s segments (the beam is greedy per segment: those are the parents the S-segment
    # beam expands), each with the feet its parent carried as start feet
    stance = p.plan(roots, 1, products=("stance",))["stance"]
    seg, d_feet = [], []
    for q, n in enumerate(chains):
        n_prev = 1 if q == 0 else live[q - 1]
        if q == 0:
            states, feet = None, stance.reshape(B, 1, 4, 3)
        else:
            first = p.plan_beam_checked(roots, options, beam=_capi.beam_params_defaults(segments=q, cycles_per_segment=k, width=W), checks=checks,
                                        products=("cycle_ok",))
            states, feet = first["state"][:, :n_prev], first["feet"][:, :n_prev]
        d_poses, d_strides = dev(np.repeat(roots, n_prev * M)), dev(np.tile(options, B * n_prev))
        d_states = dev(np.repeat(np.ascontiguousarray(states).reshape(-1), M)) if states is not None else None
        rs = product_shapes(n, k)
        bufs = {name: empty(*rs[name]) for name in ("nominal", "cycle_ok")}
        p.plan_resume_device(d_poses.data_ptr(), n, k, {name: t.data_ptr() for name, t in bufs.items()},
                             d_state_in_ptr=d_states.data_ptr() if d_states is not None else 0, d_strides_ptr=d_strides.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        seg.append(bufs)
        d_feet.append(dev(np.repeat(np.ascontiguousarray(feet).reshape(B * n_prev, 4, 3), M, axis=0)))
    big = max(chains)
    print(f"  committed cycles of the candidates, per segment: {[round(float((t['cycle_ok'].cpu().numpy() != 0).mean()), 3) for t in seg]}")
    stage = {"swing": empty((big,), _capi.SWING_SUMMARY_DTYPE), "trunk": empty((big,), _capi.TRUNK_SUMMARY_DTYPE),
             "margin": empty((big,), _capi.MARGIN_SUMMARY_DTYPE), "hit": empty((big,), np.uint8)}

    def composed():
        unchecked()
        for q, n in enumerate(chains):
            p.check_plan_device(seg[q]["nominal"].data_ptr(), seg[q]["cycle_ok"].data_ptr(), n, k, {name: t.data_ptr() for name, t in stage.items()},
                                checks=checks, d_start_feet_ptr=d_feet[q].data_ptr(), stream=s.cuda_stream)

    def forced(waves):
        def call():
            p.set_tuning(beam_check_waves=waves)   # (read per call, under the engine's lock)
            checked()
            p.set_tuning(beam_check_waves=0)
        return call

    variants = {"checked": checked, "checked_w1": forced(1), "checked_w4": forced(4), "composed": composed, "unchecked": unchecked}
    if a.only:
        variants = {a.only: variants[a.only]}

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            for _ in range(a.steps):
                fn()
            e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) / a.steps * 1e3  # us per call

    for fn in variants.values():  # warm-up: every kernel loaded, the memory pool grown, the bit planes built, the device settled
        for _ in range(3):
            block(fn)
    times = {q: [] for q in variants}
    for _ in range(a.blocks):
        for q, fn in variants.items():
            times[q].append(block(fn))
    print(f"{a.config}: B {B} roots, W {W}, M {M}, S {S}, k {k}, chains per segment {chains}; {p.describe_plan(resume=True)}")
    print(f"  {a.blocks} blocks of {a.steps} calls per variant, device events, us per call")
    med = {}
    for q in variants:
        t = np.array(times[q])
        med[q] = float(np.median(t))
        print(f"  {q:11s} median {med[q]:9.2f}  min {t.min():9.2f}  max {t.max():9.2f}  spread max / min {t.max() / t.min():.4f}")
    if "checked" in med and "composed" in med:
        print(f"  ratio checked / composed {med['checked'] / med['composed']:.4f}")
    if "checked" in med and "unchecked" in med:
        print(f"  ratio checked / unchecked {med['checked'] / med['unchecked']:.4f}")
    p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("headline", "cfg5"), default="headline")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--roots", type=int, default=64)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--options", type=int, default=8)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--only", choices=("checked", "checked_w1", "checked_w4", "composed", "unchecked"))
    run(ap.parse_args())
