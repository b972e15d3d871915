// Test-only wrapper: compiles the engine's host-side derivations (quadrupedal_foothold_planner_amd/csrc/fpe_host.cpp,
// which makes no GPU call) for the HOST, so that CPU tests can read the switches derive_constants sets for
// (parameters, map geometry): which kernel family a map position selects is decided there.
// Not part of the shipped library; built by tests/test_host_switches.py into tests/probe/_build/.
#include "../../quadrupedal_foothold_planner_amd/csrc/fpe_host.cpp"

using namespace fpe;

extern "C" {
// out: winH, footRobust, footReach, midCellInside, nFoot, tileW; cornerEps separately
void probe_plan_consts(const fpe_params* p, int rows, int cols, double res, double px, double py, float maxSearchRadius, int* out,
                       double* cornerEps) {
    const MapGeom g = make_geom(rows, cols, res, px, py);
    PlanConsts c;
    derive_constants(*p, g, maxSearchRadius, Tuning(), c);
    out[0] = c.winH;
    out[1] = c.footRobust;
    out[2] = c.footReach;
    out[3] = c.midCellInside;
    out[4] = c.nFoot;
    out[5] = c.tileW;
    *cornerEps = c.cornerEps;
}

// The constants the open-loop queries and the dense maps select their kernels by (tests/test_cpu_dense_forms.py), with the
// literal_discs switch of fpe_set_tuning as an argument.
// out: winH, footRobust, footReach, midCellInside, nFoot, tileW, nHW, spiral_rings(maxSearchRadius)
void probe_dense_consts(const fpe_params* p, int rows, int cols, double res, double px, double py, float maxSearchRadius, int literalDiscs,
                        int* out) {
    const MapGeom g = make_geom(rows, cols, res, px, py);
    Tuning tuning;
    tuning.literalDiscs = literalDiscs ? 1 : 0;
    PlanConsts c;
    derive_constants(*p, g, maxSearchRadius, tuning, c);
    const int v[8] = {c.winH, c.footRobust, c.footReach, c.midCellInside, c.nFoot, c.tileW, c.nHW, spiral_rings(maxSearchRadius, res)};
    for (int k = 0; k < 8; ++k) out[k] = v[k];
}

// What the filter chain launches for (geometry, filter parameters): filter_route's decision.
// out[0..3]  halos hN, hR, h1, h2
// out[4..7]  first window: kind (0 walking kernel, 1 row runs, 2 rides in the fused launch), TR, TC, HS
// out[8..10] fused: H (0: the separate normals / roughness kernels), TC, HS
// out[11..14] second window, as the first
// out[15] trav_only, out[16] region_ok, out[17] stepFused, out[18] nClasses of the first window's shape, out[19] of the second's
// returns FPE_OK, FPE_E_INVALID_ARG (parameters) or FPE_E_UNSUPPORTED (a radius beyond the tables)
int probe_filter_route(const fpe_filter_params* fp, int rows, int cols, double res, double px, double py, int* out) {
    FilterConsts fc;
    if (filter_consts(*fp, fc) != FPE_OK) return FPE_E_INVALID_ARG;
    const MapGeom g = make_geom(rows, cols, res, px, py);
    if (!filters_supported(fc, g)) return FPE_E_UNSUPPORTED;
    const FilterRoute rt = filter_route(fc, g);
    const int v[20] = {rt.hN, rt.hR, rt.h1, rt.h2, rt.first.kind, rt.first.TR, rt.first.TC, rt.first.HS, rt.fused.H, rt.fused.TC, rt.fused.HS,
                       rt.second.kind, rt.second.TR, rt.second.TC, rt.second.HS, rt.travOnly, rt.regionOk, rt.stepFused, rt.s1.nClasses, rt.s2.nClasses};
    for (int k = 0; k < 20; ++k) out[k] = v[k];
    return FPE_OK;
}
// step_lds_bytes as the kernels carve it
long probe_step_lds_bytes(int H, int nClasses, int TR, int TC) { return static_cast<long>(step_lds_bytes(H, nClasses, TR, TC)); }
}
