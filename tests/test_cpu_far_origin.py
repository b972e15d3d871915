"""The conditions tests/test_gpu_far_origin.py rests on, checked on the CPU alone: which kernel family the host's switches
select per (matrix row, map position) — the committed table profiles/far_origin_kernels.txt — that the exact-tie fixtures
keep their windows 9.7e5 m out, and that the translated beam and rank cases still exercise what the near ones do
(tests/beam_reference.conditions), so that no far case can pass by showing nothing."""
import numpy as np

from tests import beam_reference as bref
from tests import far_origin as fo
from tests import rank_reference, tie_fixtures
from tests.test_gpu_plan_matrix import ROWS
from tests.test_host_switches import consts, probe  # noqa: F401  (the fixture)

FAR_ROWS = ("w7_mid", "w7_gen", "w8_gen", "w16_seq", "w32_seq", "w48_direct")


def test_positions_lie_on_the_sides_of_the_flip_they_are_named_for(probe):  # noqa: F811
    flip = fo.foot_robust_flip_posx(0.02, 0.02, 200, 180)
    assert fo.BELOW[0] < 0.6 * flip and 1.2 * flip < fo.ABOVE[0] < 1.3 * flip
    # ABOVE stays below the flips of the same foot on finer maps; FAR lies beyond them all and below the guard
    assert fo.ABOVE[0] < 0.9 * fo.foot_robust_flip_posx(0.02, 0.01, 400, 360) < 0.9 * fo.foot_robust_flip_posx(0.02, 0.005, 640, 560)
    assert 2.0 * fo.foot_robust_flip_posx(0.02, 0.005, 640, 560) < abs(fo.FAR[0]) < 1e6 - 10 and abs(fo.FAR[1]) < 1e6 - 10
    assert max(abs(v) for v in fo.FAR_DYADIC) < 1e6 - 10 and all(v * 2 ** 7 == int(v * 2 ** 7) for v in fo.FAR_DYADIC)


def test_kernel_table_is_what_the_host_switches_select(probe):  # noqa: F811
    table = fo.kernel_table()
    assert set(table) == {(r, p) for r in FAR_ROWS for p in fo.POSITIONS}
    for (rid, pname), kernel in table.items():
        r = ROWS[rid]
        c = consts(probe, r.rows, r.cols, r.res, fo.POSITIONS[pname], R=r.R, rf=r.rf, maxleg=r.maxleg)
        assert fo.predicted_kernel(r, c) == kernel, (rid, pname, c)
    # the silent move the table pins: the headline foot on a bit kernel below its flip, on the literal path above
    assert table[("w7_mid", "below")] == "plan_bits_kernel<2, true>" and table[("w7_mid", "above")] == "plan_chained_kernel<8, false>"
    assert all(table[(r, p)].startswith("plan_bits") for r in ("w7_gen", "w8_gen") for p in fo.POSITIONS)


def test_tie_fixtures_keep_their_windows_at_the_dyadic_far_position(probe):  # noqa: F811
    """Every length of tests/tie_fixtures.py is dyadic, so moving the map by FAR_DYADIC moves every cell centre and every foot
    exactly; the host must still prove the windows the fixtures name (or refuse the same tie radii).  The 2^-7 m fixtures
    lose theirs to condition (4) of bits_window_halfwidth — (mag + 2e6) / res < 5e8 fails at mag = 1.9e6, res = 2^-7 — and run
    one wavefront per pose on the direct kernel (fo.tie_kernel_far)."""
    for name in tie_fixtures.NAMES:
        fx = tie_fixtures.make(name)
        pos = (fx["pos"][0] + fo.FAR_DYADIC[0], fx["pos"][1] + fo.FAR_DYADIC[1])
        p = fx["params"]
        c = consts(probe, fx["trav"].shape[0], fx["trav"].shape[1], fx["res"], pos, R=p["searchRadius"][0], rf=p["footRadius"][0],
                   maxleg=fx["maxleg"])
        want = fo.tie_kernel_far(fx)
        if "bit window" in want:
            side = int(want.split(", ")[-1].split(" x ")[0].split()[-1])
            assert c["footRobust"] == 1 and 2 * c["winH"] + 1 == side, (name, c)
        else:
            assert c["winH"] == 0 and (c["footRobust"] == 0 or fx["res"] == 2.0 ** -7), (name, c)
            assert want.startswith("plan_sequential_kernel" if c["tileW"] ** 2 > 1024 else "plan_chained_kernel<8, false>"), (name, c)
        far = fo.moved(fx["poses"], fo.FAR_DYADIC)
        assert np.array_equal(far["position"][:, 0] - fo.FAR_DYADIC[0], fx["poses"]["position"][:, 0])  # exact, both ways
        assert np.array_equal(far["position"][:, 1] - fo.FAR_DYADIC[1], fx["poses"]["position"][:, 1])


def test_far_beam_cases_meet_the_conditions_of_the_near_ones():
    """w_progress * cx is of the order 5e7 out there, with an ulp of 7e-9: the penalties (multiples of 1 and 100 plus 10 x
    squared deviations of 1e-4 and more) still separate the candidates, so the weights stay beam_reference.WEIGHTS.
    Pruning against index order, an exact tie at a survivor (the repeated option), failed and clean candidates."""
    met = {}
    for name in fo.BEAM_NAMES:
        c = fo.beam_case(name)
        assert tuple(c["weights"]) == bref.WEIGHTS
        ref = fo.beam_reference(name)
        cond = bref.conditions(ref, c["roots"]["gait"], c["k"])
        for k, v in cond.items():
            met[k] = met.get(k, False) or v
        assert cond["an_exact_tie_at_a_survivor"] and cond["survivors_are_not_the_first_candidates"], (name, cond)
        scores = np.array([s for root in ref["log"] for sg in root for s in sg["scores"]])
        assert np.isfinite(scores).all() and np.abs(scores).min() > 1e7  # the progress term dominates the magnitude
        # ... and has not made everything tie: the scores, not the indices alone, decide who survives (a root that starts off
        # the map fails every cycle of every candidate and ties throughout, here as near the origin)
        assert sum(len(set(sg["scores"])) >= 3 for root in ref["log"] for sg in root) >= 3, name  # four options, one a repeat
    assert met["a_failed_cycle_and_a_clean_candidate"] and met["a_best_path_mixes_options"] and met["sources_0_1_2"], met


def test_far_rank_case_has_something_to_rank():
    c = fo.rank_case()
    s = c["summary"]
    assert (s["committed"] == c["n"]).any() and (s["committed"] < c["n"]).any() and (s["n_source"][:, 1] > 0).any()
    score, cls, order, n0 = rank_reference.score_and_order(s, None, c["n"])
    assert len(set(score.tolist())) > len(score) // 2 and (order[:8] != np.arange(8)).any()
    assert (s["deviation_sq_sum"] > 0).any() and (s["deviation_sq_sum"] < 1.0).all()  # differences of far coordinates, not the coordinates
