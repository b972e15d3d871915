// Test-only wrapper: compiles the engine's host/device-shared geometry header
// (quadrupedal_foothold_planner_amd/csrc/fpe_gridmath.hpp) for the HOST with g++ so that CPU tests
// can check its division-free predictions against the literal forms and against the oracle.
// Not part of the shipped library; built by tests/test_gridmath_host.py into tests/probe/_build/.
#include "../../quadrupedal_foothold_planner_amd/csrc/fpe_gridmath.hpp"

using namespace fpe;

extern "C" {
int probe_index_of(double x, double org, double pos, double res) { return index_of(x, org, pos, res); }
int probe_index_of_fast(double x, double org, double pos, double res) { return index_of_fast(x, org, pos, res, 1.0 / res); }
int probe_polygon(const double* vx, const double* vy, int n, double px, double py, int fast) {
    return fast ? polygon_inside_fast(vx, vy, n, px, py) : polygon_inside(vx, vy, n, px, py);
}
// out: i0, j0, ni, nj for the literal and the fast bounding box
void probe_bbox(int rows, int cols, double res, double px, double py, double cx, double cy, double r, int* lit, int* fast) {
    const MapGeom g = make_geom(rows, cols, res, px, py);
    const BBox a = circle_bbox(g, cx, cy, r), b = circle_bbox_fast(g, cx, cy, r);
    lit[0] = a.i0; lit[1] = a.j0; lit[2] = a.ni; lit[3] = a.nj;
    fast[0] = b.i0; fast[1] = b.j0; fast[2] = b.ni; fast[3] = b.nj;
}
// getSubmapInformation: ok, i0, j0, ni, nj and base position
int probe_submap(int rows, int cols, double res, double px, double py, double x, double y, double lx, double ly, int* out,
                 double* base) {
    const MapGeom g = make_geom(rows, cols, res, px, py);
    const Submap s = submap_info(g, x, y, lx, ly);
    out[0] = s.i0; out[1] = s.j0; out[2] = s.ni; out[3] = s.nj;
    base[0] = s.baseX; base[1] = s.baseY;
    return s.ok ? 1 : 0;
}
// submap_axis on both axes: out = ok_x, i0, ni, ok_y, j0, nj and the two bases
void probe_submap_axes(int rows, int cols, double res, double px, double py, double x, double y, double lx, double ly, int* out,
                       double* base) {
    const MapGeom g = make_geom(rows, cols, res, px, py);
    const SubmapAxis a = submap_axis(g.orgX, g.posX, g.lenX, g.baseX, g.res, g.rinv, g.rows, x, lx);
    const SubmapAxis b = submap_axis(g.orgY, g.posY, g.lenY, g.baseY, g.res, g.rinv, g.cols, y, ly);
    out[0] = a.ok; out[1] = a.i0; out[2] = a.ni;
    out[3] = b.ok; out[4] = b.i0; out[5] = b.ni;
    base[0] = a.base; base[1] = b.base;
}
double probe_cell_pos(int rows, int cols, double res, double px, double py, int axis, int idx) {
    const MapGeom g = make_geom(rows, cols, res, px, py);
    return axis == 0 ? cell_pos(g.baseX, g.res, idx) : cell_pos(g.baseY, g.res, idx);
}
}
