"""Self-checks of the exact-tie fixtures (tests/tie_fixtures.py), on the oracle alone: the fixtures only pin the engine's
`<` / `<=` decisions if ties really decide outcomes, and that is a property of the inputs, not of the engine."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import fpo
from tests import tie_fixtures, util


def _is_half_integer(x, res):
    """x / res is an integer or an integer + 1/2, exactly (rational arithmetic on the f64 values)."""
    return (Fraction(float(x)) / Fraction(float(res)) * 2).denominator == 1


@pytest.mark.parametrize("name", tie_fixtures.NAMES)
def test_every_length_is_an_exact_multiple_of_the_resolution(name):
    fx = tie_fixtures.make(name)
    res, p = fx["res"], fx["params"]
    assert res in (2.0 ** -5, 2.0 ** -6, 2.0 ** -7)
    q = Fraction(float(p["searchRadius"][0])) / Fraction(res)
    assert q.denominator == 1 and q == fx["k"], q
    assert float(p["searchRadius"][0]) / res == float(fx["k"])  # and in f64, as the engine and the oracle divide
    for f in ("stepLength", "skew", "length", "width", "l1"):
        assert (Fraction(float(p[f][0])) / Fraction(res)).denominator == 1, f
    assert (Fraction(float(p["footRadius"][0])) / Fraction(res) * 16).denominator == 1
    for f in ("h", "lateralDrift"):
        v = float(p[f][0])
        assert v == 0.0 or _is_half_integer(v, 2.0 ** -8), f
    assert all(_is_half_integer(c, res) for c in fx["pos"]) and all((Fraction(c) / Fraction(res)).denominator == 1 for c in fx["pos"])
    xy = fx["poses"]["position"][:, :2]
    assert all(_is_half_integer(v, res) for v in xy.ravel())
    # the three placements, one third each: cell centres, cell corners, half a cell off in x only (rows and cols are even:
    # relative to the map position, cell corners are integers and cell centres integers + 1/2)
    rel = (xy - np.asarray(fx["pos"])) / res
    half = rel != np.floor(rel)
    kinds = half[:, 0].astype(int) * 2 + half[:, 1].astype(int)
    n = xy.shape[0]
    assert fx["trav"].shape[0] % 2 == 0 and fx["trav"].shape[1] % 2 == 0
    assert (kinds == 3).sum() == (n + 2) // 3 and (kinds == 0).sum() == (n + 1) // 3 and (kinds == 2).sum() == n // 3, np.bincount(kinds)
    r = fx["poses"]["leg_search_radius"]
    assert all((Fraction(float(v)) / Fraction(res)).denominator == 1 for v in r.ravel())
    assert (r <= p["searchRadius"][0]).all()


@pytest.mark.parametrize("name", tie_fixtures.NAMES)
def test_the_ties_decide_outcomes(name):
    """The oracle at searchRadius = R and at nextafter(R, 0) in f32 (per-leg radii likewise) must choose differently for at
    least 1 % of the legs, in the nominal or the centroid record (heights aside: the centroid method never reads z)."""
    fx = tie_fixtures.make(name)
    omap = fpo.OracleMap(fx["trav"], fx["elev"], fx["res"], fx["pos"])
    at = omap.plan(util.to_oracle_params(fx["params"]), util.to_oracle_poses(fx["poses"]), fx["n"], threads=8)
    p1, poses1 = tie_fixtures.one_ulp_shorter(fx)
    assert float(p1["searchRadius"][0]) < float(fx["params"]["searchRadius"][0])
    below = omap.plan(util.to_oracle_params(p1), util.to_oracle_poses(poses1), fx["n"], threads=8)
    differs = np.zeros(at["nominal"].shape, bool)
    for f in ("valid", "source", "row", "col"):
        differs |= at["nominal"][f] != below["nominal"][f]
    for f in ("code", "row", "col"):
        differs |= at["centroid"][f] != below["centroid"][f]
    frac = differs.mean()
    print(f"{name}: {differs.sum()} of {differs.size} legs ({100 * frac:.1f} %) change with a radius one f32 ulp shorter")
    assert frac >= 0.01, f"{name}: only {differs.sum()} of {differs.size} legs depend on the tie"
    # the fixture is not degenerate: searches happen and some succeed
    assert (at["nominal"]["source"] == 1).any() and at["nominal"]["valid"].any()
