"""Every kernel form of the producer's filter chain against the oracle: one case per form (tests/filter_form_cases.py — the 14
fused forms, the 6 row-run forms as first window, the 4 as second window, the separate normals / roughness kernels and both
walking step kernels), each as the all-layers chain and as the traversability-only chain, at the FROZEN STRICT bar of
tests/test_gpu_filters.py (imported, not restated).  tests/test_cpu_filter_route.py pins that each case selects its form and that
the case's terrain meets the conditions on the inputs; tests/test_gpu_elevation_update.py, section 9, holds the region twins to
the whole-map chain this module holds to the oracle.

The share of cells not bit-identical is 1e-4 with its floor of 4 for every case; SHARE below is the place for a case that needs
the 5e-3 of the fixed noisy maps, with the layer and the count seen — nothing wider: a cell that breaks the bar is to be routed
to the literal walks in the engine (tests/test_gpu_filters.py, module docstring)."""
import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner
from tests import filter_form_cases as fc
from tests.test_gpu_filters import assert_layers_equal, assert_no_threshold_crossing, assert_traversability_only, ulps

pytestmark = pytest.mark.gpu

SHARE = {}  # label -> (5e-3, "layer: count seen"); empty: every case meets 1e-4


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.close()


def tally(eng, ora):
    """Cells not bit-identical per layer (layers that are identical left out)."""
    out = {}
    for name in _capi.FILTER_LAYERS:
        ok = ~np.isnan(ora[name]) & ~np.isnan(eng[name])
        n = int((ulps(eng[name], ora[name])[ok] != 0).sum())
        if n:
            out[name] = n
    return out


@pytest.mark.parametrize("label", list(fc.BY_LABEL))
def test_form_matches_the_oracle(planner, label):
    c = fc.BY_LABEL[label]
    elev, ora = fc.terrain(c), fc.oracle(c)
    n_walk = fc.check_inputs(c, ora)  # (on the oracle alone; tests/test_cpu_filter_route.py runs the same without a device)
    fp = planner.filter_params(**c.radii)
    share = SHARE[label][0] if label in SHARE else 1e-4
    assert share in (1e-4, 5e-3)
    trav, layers = planner.traversability_from_elevation(elev, c.res, position=c.pos, params=fp, want_layers=True)
    only = planner.traversability_from_elevation(elev, c.res, position=c.pos, params=fp)
    ok = ~np.isnan(ora["traversability"]) & ~np.isnan(only)
    print(f"\n{label}: first {c.first} fused {c.fused} second {c.second}; {int(ok.sum())} valid cells, {n_walk} walk; not bit-identical: "
          f"all layers {tally(layers, ora) or 'none'}, traversability only {int((ulps(only, ora['traversability'])[ok] != 0).sum())}")
    assert np.array_equal(trav, layers["traversability"], equal_nan=True)
    same_normal = assert_layers_equal(layers, ora, max_ulp_cells=share)
    for name in ("step_height", "step"):  # max / min / count windows: bit-identical or wrong
        assert np.array_equal(layers[name], ora[name], equal_nan=True), f"{name}: not bit-identical"
    assert_traversability_only(only, layers, ora, same_normal, max_ulp_cells=share)
    assert_no_threshold_crossing(trav, ora["traversability"])
    assert_no_threshold_crossing(only, ora["traversability"], "traversability only: ")
