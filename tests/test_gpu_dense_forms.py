"""Every kernel form, workgroup seam and chunk edge of the open-loop queries (fpe_search_legs, fpe_centroid_legs), the three dense
maps (fpe_foothold_map, fpe_foothold_snap, fpe_centroid_map) and fpe_export_layers against the oracle: one call per case of
tests/dense_form_cases.py, at the bars the dense tests already use (imported, not restated) — flags, sources, offsets and codes
exactly; height and z bit for bit; x and y of the open-loop records bit for bit.  tests/test_cpu_dense_forms.py pins that each
case selects the kernels it names (the constants, the restated selection rules, and profiles/dense_form_kernels.txt, the kernels
an MI355X launched) and that its terrain puts something on either side of every seam and chunk edge.  The oracle's part of a case
is computed once per process (dense_form_cases.oracle)."""
import numpy as np
import pytest

from quadrupedal_foothold_planner_amd.planner import FootholdPlanner
from tests import dense_form_cases as dc
from tests import util
from tests.test_gpu_centroid_map import assert_dense, assert_records_equal
from tests.test_gpu_foothold_snap import assert_snap
from tests.test_gpu_layers import check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_footmap(got, want, cells, roi0):
    rr, cc = cells[:, 0] - roi0[0], cells[:, 1] - roi0[1]
    want_f, want_h = want
    gf, gh = got["flags"][rr, cc], got["height"][rr, cc]
    bad = np.nonzero(gf != want_f)[0]
    assert bad.size == 0, f"{bad.size} flag mismatches, first at {cells[bad[0]]}: {gf[bad[0]]} != {want_f[bad[0]]}"
    bad = np.nonzero(bits(gh) != bits(want_h))[0]
    assert bad.size == 0, f"{bad.size} height mismatches, first at {cells[bad[0]]}: {gh[bad[0]]!r} != {want_h[bad[0]]!r}"


def check(case, got):
    """The case's result against its oracle; -> the number of cells or records compared."""
    want, cells, roi0 = dc.oracle(case), dc.cells(case), dc.region(case)[:2]
    if case.entry == "search_legs":
        util.assert_nominal_equal(got, want, case.label)
        assert np.array_equal(bits(got["z"]), bits(want["z"])), f"{case.label}: z not bit for bit"
        return case.n
    if case.entry == "centroid_legs":
        assert_records_equal(got, want, case.label)
        return case.n
    if case.entry == "foothold_map":
        assert_footmap(got, want, cells, roi0)
    elif case.entry == "foothold_snap":
        assert_snap(got, want, cells, roi0=roi0)
    else:
        assert_dense(got, want, cells, roi0=roi0)
    return len(cells)


@pytest.mark.parametrize("label", [c.label for c in dc.CASES if c.group in ("select", "seam") and c.entry != "export_layers"])
def test_case_matches_the_oracle(planner, label):
    case = dc.BY_LABEL[label]
    dc.upload(planner, case)
    got = dc.call(planner, case)
    n = check(case, got)
    print(f"\n{label}: {' '.join(case.kernels)}; {n} compared with the oracle, no mismatch")
    if case.entry in ("foothold_map", "foothold_snap", "centroid_map"):
        r = dc.region(case)
        assert all(a.shape[:2] == (r[2], r[3]) for a in got.values()) and n == r[2] * r[3]  # every cell, not a sample


def test_export_of_all_ten_layers_of_the_wide_map(planner):
    """fpe_export_layers on the 40 x 1100 map with a start index that wraps in both axes, against the three dense calls (each held to
    the oracle on this map above): tests/test_gpu_layers.py's check_case — both storage orders, every layer alone and all ten, host
    and device form."""
    case = dc.BY_LABEL["seam export_layers 40x1100"]
    dc.upload(planner, case)
    planner.params = dc.params_of(case)
    check_case(planner, case.rows, case.cols, case.start, case.roi)
    out = dc.call(planner, case)
    assert len(out) == 10 and all(a.shape == (case.cols, case.rows) for a in out.values())


@pytest.mark.parametrize("label", [c.label for c in dc.CASES if c.group == "chunk"])
def test_second_chunk_of_the_literal_snap_chain(planner, label):
    """More than 2^18 cells through footsnap_queries_kernel / search_legs_kernel / footsnap_convert_kernel: the chunk that starts at
    c0 = 2^18.  Under literal_discs the whole result equals, byte for byte, the bit path's of the same call without the switch; the
    four rows around the chunk edge and 3 000 random cells are compared with the oracle (the hexagon is literal by construction and
    has the oracle alone)."""
    case = dc.BY_LABEL[label]
    dc.upload(planner, case)
    got = dc.call(planner, case)
    n = check(case, got)
    r0, c0, nr, nc = dc.region(case)
    assert got["source"].shape == (nr, nc) and nr * nc > dc.SNAP_CHUNK
    same = "-"
    if case.tuning:
        proved = dc.call(planner, case, tuning={})
        for k in ("offset", "source", "z"):
            assert np.array_equal(got[k].view(np.uint8), proved[k].view(np.uint8)), f"{label}: {k} differs from the bit path"
        same = nr * nc
    print(f"\n{label}: {' '.join(case.kernels)}; {n} cells compared with the oracle, {same} with the bit path, no mismatch")
