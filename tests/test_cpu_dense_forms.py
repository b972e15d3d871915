"""CPU conditions on the table of tests/dense_form_cases.py (one case per kernel form, workgroup seam and chunk edge of the open-loop
queries, the three dense maps and fpe_export_layers), on the oracle and the host probe alone — what keeps a case of
tests/test_gpu_dense_forms.py from passing by showing nothing:

  * every case's constants (csrc/fpe_host.cpp::derive_constants through tests/probe/host_consts_probe.cpp) select, by the selection
    rules restated here, exactly the kernels the case names;
  * the table's kernels are the code's launch sites, all of them;
  * the seam cases feed foot discs and spiral landings across their workgroup seam in both directions, and show every source byte
    and centroid code; the chunk cases have a second chunk with both kinds of hit on either side of its edge;
  * profiles/dense_form_kernels.txt, the kernels an MI355X launched for every case, equals the table line for line."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dense_form_cases as dc
from tests.test_host_switches import probe  # noqa: F401  (the fixture that builds the probe)

HERE = os.path.dirname(os.path.abspath(__file__))
DBL_EPSILON = 2.220446049250313e-16
K_ON_DEMAND_MAX_FOOT, K_HMAP_MAX_REACH, K_SNAP_MAX_RINGS = 4, 7, 32  # fpe_kernels.hip, fpe_footmap.hpp, fpe_footsnap.hpp


def consts(probe, case):  # noqa: F811
    out = np.zeros(8, np.int32)
    p = dc.params_of(case)
    probe.probe_dense_consts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_float, C.c_int, C.c_void_p]
    probe.probe_dense_consts.restype = None
    probe.probe_dense_consts(p.ctypes.data, case.rows, case.cols, case.res, float(case.pos[0]), float(case.pos[1]),
                             C.c_float(dc.max_search_radius(case)), int(case.tuning.get("literal_discs", 0)), out.ctypes.data)
    names = ("winH", "footRobust", "footReach", "midCellInside", "nFoot", "tileW", "nHW", "nRings")
    k = dict(zip(names, (int(v) for v in out)))
    k["rf"], k["res"] = float(p["footRadius"][0]), case.res
    return k


# ---- the selection rules, restated ------------------------------------------------------------------------------------------------------
def search_form(k):
    """search_group_size and mid_variant (fpe_kernels.hip): 8 lanes per query while the tile has at most 1024 cells; the 3 x 3 variant
    for a proved disc of at most four cells with a foot radius in [0.9, 1] x resolution."""
    if k["tileW"] * k["tileW"] > 1024:
        return "<64,false>"
    mid = k["midCellInside"] != 0 and k["rf"] <= k["res"] and k["footRobust"] != 0 and k["nFoot"] <= K_ON_DEMAND_MAX_FOOT
    return "<8,true>" if mid else "<8,false>"


def footmap_kernels(k, flags=True, height=True):
    """launch_foothold_map: the literal walk without a proved table; else the flags by bit planes where the table has a row-interval
    form (by the table itself where not), then the heights."""
    if not k["footRobust"]:
        return [dc.DIRECT_LITERAL]
    out = []
    if flags:
        out.append(dc.FLAGS_BITS if k["nHW"] > 0 else dc.DIRECT_TABLE)
    if height:
        out.append(dc.HEIGHT)
    return out


def snap_prove(case):
    """snap_prove (fpe_engine.cpp), from its comment: the rectangle's half sides R and R / 2 and the squared radius of the ring filter
    must each lie farther than the rounding bound E from every lattice value they are compared with."""
    res, r = case.res, dc.radius_of(case)
    rings = int(np.ceil(r / res))
    base_x = case.pos[0] + (0.5 * (case.rows * res) - 0.5 * res)
    base_y = case.pos[1] + (0.5 * (case.cols * res) - 0.5 * res)
    ext = max(abs(base_x), abs(base_x + res * -(case.rows - 1)), abs(base_y), abs(base_y + res * -(case.cols - 1))) + r + res
    E = 64.0 * DBL_EPSILON * (1.0 + ext)
    ok = True
    for hr in (r, 0.5 * r):
        a = int(np.floor(hr / res))
        while a >= 0 and a * res >= hr:
            a -= 1
        while (a + 1) * res < hr:
            a += 1
        ok = ok and abs(a * res - hr) > E and abs((a + 1) * res - hr) > E
    E2 = 2.0 * (r + 2.0 * res) * E + E * E
    for n in range(2 * (rings + 1) * (rings + 1) + 1):
        if abs(n * res * res - r * r) <= E2:
            ok = False
    return ok


def snap_kernels(k, case):
    """foothold_snap_bits_ok and the two launch functions of fpe_footsnap.hpp (all three products requested)."""
    bits = (k["footRobust"] != 0 and k["nHW"] > 0 and k["footReach"] <= K_HMAP_MAX_REACH and case.polygon == "rectangle" and snap_prove(case)
            and k["nRings"] <= K_SNAP_MAX_RINGS)
    if bits:
        return footmap_kernels(k, flags=False) + [dc.SNAP_BITS]
    _, _, nr, nc = dc.region(case)
    chunks = (nr * nc + dc.SNAP_CHUNK - 1) // dc.SNAP_CHUNK
    return list(dc.literal("search_legs_kernel" + search_form(k), chunks))


def cmap_kernels(k):
    return [dc.CMAP_ROWS, dc.CMAP_CODE, "cmap_z_kernel" + search_form(k)]


def expected_kernels(probe, case):  # noqa: F811
    k = consts(probe, case)
    if case.entry == "search_legs":
        return ["search_legs_kernel" + search_form(k)]
    if case.entry == "centroid_legs":
        return ["centroid_legs_kernel" + search_form(k)]
    if case.entry == "foothold_map":
        return footmap_kernels(k)
    if case.entry == "foothold_snap":
        return snap_kernels(k, case)
    if case.entry == "centroid_map":
        return cmap_kernels(k)
    assert case.entry == "export_layers"  # run_export_layers: the foothold map, the snap map, the centroid map, one export launch
    fm, sn, cm = (case._replace(entry=e) for e in ("foothold_map", "foothold_snap", "centroid_map"))
    return footmap_kernels(consts(probe, fm)) + snap_kernels(consts(probe, sn), sn) + cmap_kernels(consts(probe, cm)) + [dc.EXPORT]


# ---- selection ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(dc.BY_LABEL))
def test_case_constants_select_the_kernels_the_case_names(probe, label):  # noqa: F811
    case = dc.BY_LABEL[label]
    assert tuple(expected_kernels(probe, case)) == case.kernels, (label, consts(probe, case))


# the constants the cases were chosen for: a proof that moves shows here before a form silently loses its case
STATED = {
    "search_legs 2cm R=0.1 n=1": dict(tileW=19, footRobust=1, nFoot=1, midCellInside=1),
    "search_legs 1cm R=0.1 n=1": dict(tileW=31, footRobust=1, nFoot=9),
    "search_legs 0.5cm R=0.1 n=1": dict(tileW=55),
    "search_legs 2cm R=0.3 n=1": dict(tileW=39, midCellInside=1, footRobust=1, nFoot=1),
    "centroid_map 2cm R=1.94": dict(tileW=19),
    "foothold_map 1cm rf=0.035": dict(footRobust=1, nHW=3, footReach=3),
    "foothold_map 1cm rf=0.062": dict(footRobust=1, nFoot=121, nHW=0, footReach=6),
    "foothold_map 1cm rf=0.065 table overflow": dict(footRobust=0, nFoot=0),
    "foothold_map rf=0.05 res=rf/3 lattice tie": dict(footRobust=0, nFoot=0),
    "foothold_map 2cm rf=0": dict(footRobust=0),
    "foothold_map 1cm rf=0.035 literal_discs": dict(footRobust=0, nHW=3),
    "foothold_snap 1cm rf=0.035 R=0.15": dict(footRobust=1, nHW=3, footReach=3, nRings=16),
    "foothold_snap 2cm R=0.7 rings": dict(footRobust=1, nHW=1, nRings=35),
    "foothold_snap 2^-5 R=0.125 rectangle tie": dict(footRobust=1, nHW=1, nRings=4),
    "foothold_snap 1cm rf=0.062 no row intervals": dict(footRobust=1, nHW=0),
    "seam foothold_map 70x140 1cm rf=0.062": dict(footRobust=1, nHW=0, footReach=6),
}


@pytest.mark.parametrize("label", list(STATED))
def test_the_cases_have_the_constants_they_were_chosen_for(probe, label):  # noqa: F811
    got = consts(probe, dc.BY_LABEL[label])
    assert {k: got[k] for k in STATED[label]} == STATED[label], (label, got)


def test_snap_prove_holds_and_fails_where_the_cases_say():
    """15 x 0.01 is 6e-9 m from f32(0.15): far outside E (1e-14 on these maps); 0.125 = 4 x 2^-5 and 0.0625 = 2 x 2^-5 exactly."""
    assert snap_prove(dc.BY_LABEL["foothold_snap 1cm rf=0.035 R=0.15"])
    assert snap_prove(dc.BY_LABEL["seam foothold_snap 40x1100 region"])
    assert snap_prove(dc.BY_LABEL["foothold_snap 2cm R=0.7 rings"])  # (the ring count alone sends it to the literal chain)
    assert snap_prove(dc.BY_LABEL["chunk foothold_snap 513x513 literal_discs"])  # (the bit path of the same call is the comparison)
    assert not snap_prove(dc.BY_LABEL["foothold_snap 2^-5 R=0.125 rectangle tie"])
    assert abs(15 * 0.01 - float(np.float32(0.15))) > 5e-9


def test_the_table_covers_every_launch_site():
    """The union of the table's kernels is the list of launch sites (dense_form_cases.LAUNCH_SITES, written out there once) and the
    export launch; the open-loop forms each run with a single query and with a partly empty last workgroup."""
    named = {k for c in dc.CASES for k in c.kernels}
    assert named == set(dc.LAUNCH_SITES) | {dc.EXPORT}
    assert len(set(dc.LAUNCH_SITES)) == len(dc.LAUNCH_SITES) == 18
    for entry, forms in (("search_legs", (dc.S8M, dc.S8, dc.S64)), ("centroid_legs", (dc.C8M, dc.C8, dc.C64))):
        for f in forms:
            ns = {c.n for c in dc.CASES if c.entry == entry and c.kernels == (f,)}
            assert {1, 97} <= ns, (f, ns)
    assert 97 % 32 == 1 and 97 % 4 == 1
    # both ways into every kernel pair of launch_foothold_map, the bit path and five ways into the literal snap chain
    assert sum(c.entry == "foothold_map" and c.group == "select" and c.kernels == (dc.DIRECT_LITERAL,) for c in dc.CASES) == 4
    assert sum(c.entry == "foothold_snap" and c.group == "select" and c.kernels[0] == dc.SNAP_QUERIES for c in dc.CASES) == 5


# ---- seams --------------------------------------------------------------------------------------------------------------------------------
SEAM_CASES = [c.label for c in dc.CASES if c.group == "seam" and c.entry != "export_layers"]


def test_the_seam_columns_are_workgroup_seams():
    for c in dc.CASES:
        if c.group != "seam" or c.cols <= 1024:
            continue
        r0, c0, nr, nc = dc.region(c)
        (seam,) = dc.seam_columns(c)
        assert seam == 32 * ((c0 >> 5) + 32) and c0 < seam - 64 and seam + 32 <= c0 + nc, c.label  # 32 words per workgroup from word c0 >> 5
        assert nc > 4 * 256  # cmap_code_kernel: more than four column blocks
    assert dc.SEAMS == (1024, 1056)
    r = dc.BY_LABEL["seam foothold_map 40x1100 region"].roi
    assert r[1] >> 5 == 1 and ((r[1] + r[3] - 1) >> 5) - (r[1] >> 5) + 1 == 34 and r[0] % 8 != 0
    c = dc.BY_LABEL["seam centroid_map 150x300 2cm R=1.0"]
    assert (c.cols + 255) // 256 == 2 and (c.cols + 63) // 64 == 5 and 2 * int(np.ceil(1.0 / c.res)) + 1 > 3 * 32
    c = dc.BY_LABEL["seam foothold_map 70x140 1cm rf=0.062"]
    assert c.rows >= 70 and c.cols >= 140 and (c.rows + 31) // 32 == 3 and (c.cols + 63) // 64 == 3
    c = dc.BY_LABEL["seam export_layers 40x1100"]
    assert c.start != (0, 0) and c.start[0] < c.rows and c.start[1] < c.cols and c.roi is None and len(c.kernels) == 8


@pytest.mark.parametrize("label", SEAM_CASES)
def test_seam_cases_show_what_they_are_for(label):
    case = dc.BY_LABEL[label]
    assert case.compare == "all"
    ora = dc.oracle(case)
    if case.entry == "foothold_map":
        for seam in dc.seam_columns(case):
            left, right = dc.discs_fed_across(case, seam)
            assert left >= 16 and right >= 16, (label, seam, left, right)
        flags, height = ora
        assert len(set(flags.tolist())) >= 4 and np.isfinite(height).all()
    elif case.entry == "foothold_snap":
        off, src, _ = ora
        assert set(src.tolist()) == {0, 1, 2}, label
        for seam in dc.seam_columns(case):
            l2r, r2l = dc.landings_across(case, seam)
            assert l2r >= 4 and r2l >= 4, (label, seam, l2r, r2l)
    else:
        code = ora[0]
        want = set(range(1, 6)) | ({0} if dc.radius_of(case) == float(np.float32(0.1)) else set())
        assert want <= set(code.tolist()), (label, sorted(set(code.tolist())))


# ---- chunks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", [c.label for c in dc.CASES if c.group == "chunk"])
def test_chunk_cases_have_a_second_chunk_with_both_kinds_of_hit_at_its_edge(label):
    case = dc.BY_LABEL[label]
    r0, c0, nr, nc = dc.region(case)
    assert nr * nc > dc.SNAP_CHUNK and case.kernels.count(dc.SNAP_CONVERT) == 2
    cells = dc.cells(case)
    assert len(cells) >= 4 * nc + 3000 - nc  # (the edge may sit in the region's second-last row: then three rows exist around it)
    off, src, _ = dc.oracle(case)
    lin = (cells[:, 0] - r0) * nc + (cells[:, 1] - c0)
    before = (lin < dc.SNAP_CHUNK) & (lin >= dc.SNAP_CHUNK - 2 * nc)
    after = (lin >= dc.SNAP_CHUNK) & (lin < dc.SNAP_CHUNK + 2 * nc)
    for side in (before, after):
        assert (src[side] == 1).any() and (src[side] == 0).any(), label
    assert np.abs(off[src == 1]).max() >= 1  # some spiral hit lands away from its cell


# ---- the kernels that ran ---------------------------------------------------------------------------------------------------------------------
def test_the_traced_kernels_are_the_table():
    """profiles/dense_form_kernels.txt: one call per case behind a marker, under one kernel trace on an MI355X (recipe in
    profiles/dense_form_kernels.py).  Every line equals its case's kernels, in launch order, and every launch site ran."""
    path = os.path.join(HERE, "..", "profiles", "dense_form_kernels.txt")
    lines = [ln for ln in open(path).read().splitlines() if ln and not ln.startswith("#")]
    traced = {}
    for ln in lines:
        label, _, names = ln.rpartition(": ")
        traced[label] = tuple(names.split())
    assert len(traced) == len(lines) and set(traced) == set(dc.BY_LABEL)
    for c in dc.CASES:
        assert traced[c.label] == c.kernels, c.label
    assert {k for names in traced.values() for k in names} == set(dc.LAUNCH_SITES) | {dc.EXPORT}
