// fpe_bits_lane8.hpp — the bit-window kernels, second piece (included by fpe_bits.hpp, inside namespace fpe; not stand-alone):
// the 8-LANE family — eight lanes per leg, two poses per wavefront, windows of up to 32 rows and columns
// (plan_bits_kernel<NRL, kMid, kProd>: the 3x3-only kernels with their straight-line leg search leg_fast8m, and the generic ones).
#pragma once

namespace {

// ---- 8-lane kernels: the y side of a leg's geometry, hoisted out of the chain ---------------------------------------
// A leg's search centre and boxes have y = (initialPose_[1] + ajustedPose_[1]) + defaultBias.y (cpp:2201, 2411-2418):
// it depends on the gait cycle only, never on earlier results.  Everything derived from it — the column indices of
// the foot-disc box, of the centroid rectangle and of getIndex(centre), the y part of getSubmap's geometry, the
// rectangle polygon's column interval, the squared y distances of the 3x3 disc's columns — is computed for eight
// cycles at a time, one (leg, cycle) entry per lane, with the exact functions; the chain then evaluates x only.

// ---- 3x3-only 8-lane kernels: results and heights leave the chain ----------------------------------------------------
// Nothing a later gait cycle reads depends on a mean height (getPolygonCenter uses x and y only, cpp:2421-2463), and
// the output records are write-only.  The chain therefore only DEPOSITS, per (leg, cycle), the elevations its disc
// loads returned and the few words that identify the results; every eighth cycle the 32 lanes of a pose each take one
// (leg, cycle) unit, run its three ordered height sums (cpp:2520-2554) serially and write its four output records —
// one instruction stream for 32 units instead of one per leg and cycle.
struct Unit {
    float eA[9];  // centre disc (checkFoothold's centre, cpp:2029): elevations in CircleIterator order, [4] = middle cell
    float eB[9];  // default-track disc (cpp:2289-2301)
    float eC;     // centroid result's own cell (one-cell foot disc)
    uint32_t pad0;  // (the eight words below start on a 16-byte boundary: lane 0 deposits them with two 16-byte LDS stores, the three
                    // positions with one 16-byte and one 8-byte store — eleven separate stores before)
    uint32_t visA, visB;  // bit k: cell k visited; bit 31: the height was computed in the chain (direct pass) and is in e[0]
    int nomRow, nomCol;
    uint32_t nomFlags;    // valid | source << 8
    int cenRow, cenCol;
    uint32_t cenCode;     // code | 0x100: the result has a one-cell disc whose elevation is in eC | 0x200: ... to be read by flush_unit
    double cx;    // search centre x (nominal x of a default hit / invalid leg; centroid x of code 0)
    double cenX;  // centroid result x (codes 1-4)
    double defX;  // default track x
    uint32_t pad[2];
};
static_assert(sizeof(Unit) == 144 && sizeof(Unit) % 16 == 0 && offsetof(Unit, visA) == 80 && offsetof(Unit, cx) == 112, "Unit layout");
// three consecutive cells of a layer row / three consecutive floats of Unit::eA / eB, at a 4-byte boundary (leg_fast8m)
typedef float UnitRow3 __attribute__((ext_vector_type(3), aligned(4)));

// 3x3 form: lane s holds cell s + (s >= 4) of the box, every lane the middle cell (disc_issue); else the direct pass.
template <bool kWant>
__device__ __forceinline__ void unit_put_disc(const DevMap& m, const PlanConsts& pc, double cx, double cy, const BBox& bb,
                                              const Grp<8>& g, const DiscLoads& d, float* e, uint32_t& vis, float* scratch) {
    if (!kWant) return;
    if (d.pipelined) {  // wave-uniform: the 3x3 form
        e[g.sub + (g.sub >= 4 ? 1 : 0)] = d.e[0];
        if (g.sub == 0) e[4] = d.eMid;
        const unsigned mk = static_cast<unsigned>(g.ballot(d.vis[0] != 0));
        vis = (mk & 0xFu) | 0x10u | ((mk & 0xF0u) << 1);
    } else {
        bool unused;
        const float z = disc_pass_direct<8, false>(m, pc, cx, cy, bb, g, unused, scratch);
        if (g.sub == 0) e[0] = z;
        vis = 0x80000000u;
    }
}
// getFootholdMeanHeight (cpp:2520-2554) over up to nine deposited cells, in order
__device__ __forceinline__ float unit_mean9(const float* e, uint32_t vis, double h) {
    if (vis & 0x80000000u) return e[0];
    float sum = 0.0f, last = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {  // branch-free: an unvisited cell adds -0.0f (s + (-0.0f) == s for every s) and leaves `last`
        const bool visited = ((vis >> k) & 1u) != 0u;
        const float v = __builtin_isfinite(e[k]) ? e[k] : 0.0f;  // cpp:2532-2537
        const bool inc = visited && v < 10;                      // cpp:2539
        last = visited ? v : last;
        cnt += inc ? 1 : 0;
        sum = sum + (inc ? v : -0.0f);
    }
    return finish_mean(sum, last, cnt, h);
}
// One (leg, cycle) unit per lane: heights and the four output records of that unit.
__device__ __forceinline__ void flush_unit(const DevMap& m, double h, const Unit& uLds, const YEntry& yeLds, int b, int cyc,
                                           int leg, int nCycles, uint32_t okBits, const fpe_plan_out& out) {
    const MapGeom& mg = m.g;
    // the unit and its y entry in registers by one batch of 16-byte LDS reads (read field by field the reads are
    // interleaved with their uses: a dozen serial round trips)
    Unit u;
    YEntry ye;
    __builtin_memcpy(&u, &uLds, sizeof(Unit));
    __builtin_memcpy(&ye, &yeLds, sizeof(YEntry));
    // the centroid result's own cell, when the chain left its elevation to be read here (issued first: the three
    // height sums below cover the round trip)
    float eC = u.eC;
    if (out.centroid && (u.cenCode & 0x200u)) eC = m.elev[static_cast<size_t>(u.cenRow) * mg.cols + u.cenCol];
    if (leg == 0 && out.cycle_ok) out.cycle_ok[static_cast<size_t>(b) * nCycles + cyc] = static_cast<uint8_t>((okBits >> (cyc & 7)) & 1u);
    const float zA = unit_mean9(u.eA, u.visA, h);
    const float zB = out.default_next ? unit_mean9(u.eB, u.visB, h) : 0.0f;
    const int code = static_cast<int>(u.cenCode & 0xFFu);
    float zC = 0.0f;
    if (u.cenCode & 0x300u) {
        const float v = __builtin_isfinite(eC) ? eC : 0.0f;
        const bool inc = v < 10;
        zC = finish_mean(inc ? 0.0f + v : 0.0f, v, inc ? 1 : 0, h);
    } else if (code == 0) {
        zC = zA;  // whole region valid: the height at the centre (cpp:1687)
    }
    const size_t o = (static_cast<size_t>(b) * nCycles + cyc) * 4 + leg;
    const int valid = static_cast<int>(u.nomFlags & 0xFFu), source = static_cast<int>((u.nomFlags >> 8) & 0xFFu);
    const float zN = valid ? zA : 0.0f;  // z at the DEFAULT centre, for a spiral candidate too (cpp:2029)
    if (out.nominal) {
        fpe_foothold f;
        f.row = u.nomRow;
        f.col = u.nomCol;
        f.x = source == 1 ? cell_pos(mg.baseX, mg.res, u.nomRow) : u.cx;  // cpp:2105-2107 / cpp:2016-2017
        f.y = source == 1 ? cell_pos(mg.baseY, mg.res, u.nomCol) : ye.ny;
        f.z = zN;
        f.valid = static_cast<uint8_t>(valid);
        f.source = static_cast<uint8_t>(source);
        f.foot_id = static_cast<uint8_t>(leg);
        f.gait_cycle_id = static_cast<uint8_t>(cyc);
        store_record<true>(out.nominal + o, f);
    }
    store_selected<true>(out, o, u.nomRow, u.nomCol, zN, valid, source, leg, cyc);
    if (out.centroid) {
        fpe_centroid_foothold cf;
        cf.x = code == 0 ? u.cx : (code <= 4 ? u.cenX : 0.0);
        cf.y = code == 0 ? ye.ny : (code == 1 ? ye.yA : (code <= 4 ? ye.yB : 0.0));
        cf.z = zC; cf.row = u.cenRow; cf.col = u.cenCol;
        cf.code = static_cast<uint8_t>(code); cf.pad[0] = cf.pad[1] = cf.pad[2] = 0;
        store_record<true>(out.centroid + o, cf);
    }
    if (out.default_next) {
        store_record<true>(out.default_next + o * 3 + 0, u.defX);
        store_record<true>(out.default_next + o * 3 + 1, ye.ny);
        store_record<true>(out.default_next + o * 3 + 2, static_cast<double>(zB));
    }
}

// ---- generic 8-lane kernels (boxes of up to 32 cells, foot-disc tables): the same deferral --------------------------
// The chain deposits, per (leg, cycle), the MEMBERSHIP of the two discs around known centres (a 32-bit mask over the
// bounding box's cells in CircleIterator order, with the box's origin) and the words that identify the results; it
// issues no elevation load at all.  Every fourth cycle (the LDS of twelve workgroups per CU holds four cycles of units
// and y entries, not eight) lane (leg, s < 4) of a pose takes the unit of cycle base + s, reads the elevations itself
// (seq_mean2: two groups of eight independent loads per batch) and runs the ordered sums (cpp:2520-2554).
constexpr uint32_t kUgValid = 1u << 8, kUgSrcShift = 9, kUgPreA = 1u << 12, kUgPreB = 1u << 13, kUgCTable = 1u << 14, kUgCIsA = 1u << 15;
struct UnitG {
    double cx;    // search centre x (nominal x of a default hit / invalid leg; centroid x of code 0)
    double cenX;  // centroid result x (codes 1-4)
    double defX;  // default track x
    int aI0, aJ0;
    uint32_t visA;  // centre disc (cpp:2029): bit t = cell t of the box visited; kUgPreA: the f32 height itself (direct pass)
    int bI0, bJ0;
    uint32_t visB;  // default-track disc (cpp:2289-2301), kUgPreB likewise
    int nomRow, nomCol, cenRow, cenCol;
    uint32_t flags;  // centroid code | kUgValid | source << 9 | kUg* | aNj << 16 | bNj << 24
    uint32_t pad[3];
};
static_assert(sizeof(UnitG) == 80 && sizeof(UnitG) % 16 == 0, "UnitG layout");

// Membership of a leg's two foot discs — the centre disc around (cxA, cy) and the default-track disc around (cxB, cy):
// same columns, the y side is shared — with lane = BOX ROW: bit q of the lane's word = cell (i0 + sub, j0 + q) is visited
// (inside the box, the map and the disc; CircleIterator::isInside, the expression of cell_in_disc).  Boxes of up to 8 x 8
// cells; one pass over the columns instead of four rounds of eight cells per disc with a division each.
__device__ __forceinline__ void disc_rows8(const MapGeom& mg, double rf2, double cxA, double cxB, double cy, const BBox& ba, const BBox& bbx,
                                           const Grp<8>& g, uint32_t& rowA, uint32_t& rowB) {
    const int iA = ba.i0 + g.sub, iB = bbx.i0 + g.sub;
    const double dxA = cell_pos(mg.baseX, mg.res, iA) - cxA, dxB = cell_pos(mg.baseX, mg.res, iB) - cxB;
    const double dxA2 = dxA * dxA, dxB2 = dxB * dxB;
    const int j0 = ba.j0, nj = ba.nj;  // (both boxes: YEntry::j0d / njd)
    uint32_t a = 0u, b = 0u;
    for (int q = 0; __ballot(q < nj) != 0ull; ++q) {  // wave-uniform trip count
        const double dy = cell_pos(mg.baseY, mg.res, j0 + q) - cy;
        const double dy2 = dy * dy;
        a |= ((dxA2 + dy2) <= rf2) ? (1u << q) : 0u;
        b |= ((dxB2 + dy2) <= rf2) ? (1u << q) : 0u;
    }
    const int lo = max(0, -j0), hi = min(nj - 1, mg.cols - 1 - j0);  // columns inside the box and the map
    const uint32_t colMask = hi >= lo ? ((2u << hi) - (1u << lo)) : 0u;
    rowA = (g.sub < ba.ni && static_cast<unsigned>(iA) < static_cast<unsigned>(mg.rows)) ? (a & colMask) : 0u;
    rowB = (g.sub < bbx.ni && static_cast<unsigned>(iB) < static_cast<unsigned>(mg.rows)) ? (b & colMask) : 0u;
}
// OR over the eight lanes of a group (DPP: two quad permutations and the half-row mirror)
__device__ __forceinline__ uint32_t or_reduce8(uint32_t v) {
    int x = static_cast<int>(v);
    x |= __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    x |= __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    x |= __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true);  // row_half_mirror
    return static_cast<uint32_t>(x);
}
// The box's 32-bit membership mask in CircleIterator order (cell t = a * nj + b) from the row words
__device__ __forceinline__ uint32_t box_mask_from_rows8(uint32_t row, int nj, const Grp<8>& g) {
    return or_reduce8(row << min(g.sub * nj, 31));  // (rows beyond the box hold 0)
}
// checkFoothold's default test (cpp:2012) on the row words: no visited cell of the centre disc has its Df bit set
__device__ __forceinline__ bool default_ok_rows8(uint32_t rowA, const BBox& bb, const uint32_t* rowsDf, int nRows, int iw0, int jw0, const Grp<8>& g) {
    const int ri = bb.i0 - iw0 + g.sub, cj0 = bb.j0 - jw0;
    const uint32_t df = rowsDf[min(max(ri, 0), nRows - 1)];
    // bit q of `sh` = window column cj0 + q of the row (columns outside the 32-bit window: 0, as win_bit)
    const uint32_t sh = (cj0 >= 32 || cj0 <= -32) ? 0u : (cj0 >= 0 ? df >> cj0 : df << -cj0);
    const bool fail = static_cast<unsigned>(ri) < static_cast<unsigned>(nRows) && (rowA & sh) != 0u;
    return g.any(rowA != 0u) && !g.any(fail);
}
__device__ __forceinline__ void unitg_put_disc(const DevMap& m, const PlanConsts& pc, double cx, double cy, const BBox& bb, const Grp<8>& g,
                                               const DiscLoads& d, uint32_t& vis, bool& pre, float* scratch) {
    if (d.pipelined) {  // wave-uniform
        if (d.mid) {    // 3x3 form: lane s holds cell s + (s >= 4), the middle cell is always visited
            const unsigned mk = static_cast<unsigned>(g.ballot(d.vis[0] != 0));
            vis = (mk & 0xFu) | 0x10u | ((mk & 0xF0u) << 1);
        } else {
            vis = 0u;
#pragma unroll
            for (int r = 0; r < kDiscRounds; ++r) vis |= (static_cast<uint32_t>(g.ballot(d.vis[r] != 0)) & 0xFFu) << (8 * r);
        }
        pre = false;
    } else {
        bool unused;
        vis = __float_as_uint(disc_pass_direct<8, false>(m, pc, cx, cy, bb, g, unused, scratch));
        pre = true;
    }
}
// Two lanes per (leg, cycle) unit: lane half 0 takes the centre disc and the centroid result's disc and writes the
// nominal / selected / centroid records, half 1 the default-track disc, the default_next record and the cycle's
// validity.  One instruction stream for both (the arguments differ per lane, not the code).
__device__ __forceinline__ void flush_unit_g(const DevMap& m, const PlanConsts& pc, const int8_t* footDa, const int8_t* footDb,
                                             const UnitG& uLds, const YEntry& yeLds, int b, int cyc, int leg, int half, int nCycles,
                                             uint32_t okBits, const fpe_plan_out& out, int cycBase = 0) {
    // cycBase (the resume kernels: fpe_plan_state.cycle): added to the records' gait_cycle_id; every index stays the call's own `cyc`
    const MapGeom& mg = m.g;
    UnitG u;
    __builtin_memcpy(&u, &uLds, sizeof(UnitG));
    const double ny = yeLds.ny, yA = yeLds.yA, yB = yeLds.yB;
    const bool h1 = half != 0;
    const bool pre = (u.flags & (h1 ? kUgPreB : kUgPreA)) != 0u;
    const uint32_t visW = h1 ? u.visB : u.visA;
    const bool wantBox = !pre && (h1 ? out.default_next != nullptr : true);
    const bool wantC = !h1 && (u.flags & kUgCTable) != 0u && out.centroid != nullptr;
    const int nj = max(static_cast<int>(h1 ? (u.flags >> 24) : ((u.flags >> 16) & 0xFFu)), 1);
    float sBox, sC;
    seq_mean2_visited(m.elev, mg.rows, mg.cols, h1 ? u.bI0 : u.aI0, h1 ? u.bJ0 : u.aJ0, nj, wantBox ? visW : 0u, wantC, u.cenRow, u.cenCol, footDa,
                      footDb, pc.nFoot, pc.h, sBox, sC);
    const float zBox = pre ? __uint_as_float(visW) : sBox;
    const size_t o = (static_cast<size_t>(b) * nCycles + cyc) * 4 + leg;
    if (h1) {
        if (leg == 0 && out.cycle_ok) out.cycle_ok[static_cast<size_t>(b) * nCycles + cyc] = static_cast<uint8_t>((okBits >> (cyc & 7)) & 1u);
        if (out.default_next) {
            store_record<true>(out.default_next + o * 3 + 0, u.defX);
            store_record<true>(out.default_next + o * 3 + 1, ny);
            store_record<true>(out.default_next + o * 3 + 2, static_cast<double>(zBox));
        }
        return;
    }
    const float zA = zBox;
    const float zC = wantC ? sC : ((u.flags & kUgCIsA) ? zA : 0.0f);  // code 0, whole region valid: the height at the centre (cpp:1687)
    const int code = static_cast<int>(u.flags & 0xFFu);
    const int valid = (u.flags & kUgValid) ? 1 : 0, source = static_cast<int>((u.flags >> kUgSrcShift) & 3u);
    const float zN = valid ? zA : 0.0f;  // z at the DEFAULT centre, for a spiral candidate too (cpp:2029)
    if (out.nominal) {
        fpe_foothold f;
        f.row = u.nomRow;
        f.col = u.nomCol;
        f.x = source == 1 ? cell_pos(mg.baseX, mg.res, u.nomRow) : u.cx;  // cpp:2105-2107 / cpp:2016-2017
        f.y = source == 1 ? cell_pos(mg.baseY, mg.res, u.nomCol) : ny;
        f.z = zN;
        f.valid = static_cast<uint8_t>(valid);
        f.source = static_cast<uint8_t>(source);
        f.foot_id = static_cast<uint8_t>(leg);
        f.gait_cycle_id = static_cast<uint8_t>(cycBase + cyc);
        store_record<true>(out.nominal + o, f);
    }
    store_selected<true>(out, o, u.nomRow, u.nomCol, zN, valid, source, leg, cycBase + cyc);
    if (out.centroid) {
        fpe_centroid_foothold cf;
        cf.x = code == 0 ? u.cx : (code <= 4 ? u.cenX : 0.0);
        cf.y = code == 0 ? ny : (code == 1 ? yA : (code <= 4 ? yB : 0.0));
        cf.z = zC; cf.row = u.cenRow; cf.col = u.cenCol;
        cf.code = static_cast<uint8_t>(code); cf.pad[0] = cf.pad[1] = cf.pad[2] = 0;
        store_record<true>(out.centroid + o, cf);
    }
}

constexpr int kYCentreMid = 4;  // YEntry::flags, 3x3-only kernels: jc == j0d + 1
// PC: the plan constants of the caller (rf, cornerEps, winH: PlanConsts, or YFillConsts of the 3x3-only kernels)
struct YFillConsts {
    double rf, cornerEps;
    int winH;
};
template <class PC>
__device__ __forceinline__ void fill_yentry(const MapGeom& mg, const PC& pc, const LegStatic& ls, double ny, YEntry& e) {
    const double ly = ls.lk.ly;  // centroid rectangle width (cpp:1617)
    const double r = static_cast<double>(ls.Rf);
    int flags = fabs(ny) <= 1e6 ? 2 : 0;
    e.ny = ny;
    // foot-disc box (CircleIterator::findSubmapParameters, y axis), getIndex(centre), centroid rectangle
    // (getSubmapInformation, y axis: corners centre +- 0.5 * ly).
    // Predicted, as in the x pass of the chain (PlanConsts::cornerEps): a corner strictly inside the map whose quotient
    // is farther than cornerEps from an integer has the index -trunc(quotient) and stays within the map, whatever
    // boundPositionToRange's rewrite and the index division do to the last bits.  When any lane of the wavefront is
    // too close to a cell boundary or to the map's edge, the wavefront evaluates the reference's own expressions (a
    // real branch: the if-converted form would pay five divisions per entry).
    const double xs0[5] = {ny + pc.rf, ny - pc.rf, ny, ny + 0.5 * ly, ny - 0.5 * ly};
    int idx[5];
    bool safe = true;
    const double colsD = static_cast<double>(mg.cols);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double qf = ((xs0[k] - mg.orgY) - mg.posY) * mg.rinv;
        const double kk = trunc(qf);
        const double fr = fabs(qf - kk);
        safe = safe & (fr > pc.cornerEps) & (fr < 1.0 - pc.cornerEps);
        if (k != 2) safe = safe & (qf < -pc.cornerEps) & (qf > pc.cornerEps - colsD);
        idx[k] = -static_cast<int>(kk);
    }
    bool cornersWithin = true;  // checkIfPositionWithinMap of the centroid rectangle's bounded corners (y axis)
    if (FPE_RARE_IF((std::is_same<PC, YFillConsts>::value), __ballot(!safe) != 0ull)) {  // (weighted in the 3x3-only kernels)
        const double tly = bound_axis(xs0[0], mg.orgY, mg.posY, mg.lenY);
        const double bry = bound_axis(xs0[1], mg.orgY, mg.posY, mg.lenY);
        const double tlr = bound_axis(xs0[3], mg.orgY, mg.posY, mg.lenY);
        const double brr = bound_axis(xs0[4], mg.orgY, mg.posY, mg.lenY);
        const double xs[5] = {tly, bry, ny, tlr, brr};
#pragma unroll
        for (int k = 0; k < 5; ++k) idx[k] = index_of(xs[k], mg.orgY, mg.posY, mg.res);
        cornersWithin = within_axis(tlr, mg.orgY, mg.posY, mg.lenY) && within_axis(brr, mg.orgY, mg.posY, mg.lenY);
    }
    e.j0d = idx[0];
    e.njd = idx[1] - idx[0] + 1;
    e.jc = idx[2];
    const int j0r = idx[3];
    const int j1r = idx[4];
    e.j0r = j0r;
    e.njr = j1r - j0r + 1;
    bool okY = cornersWithin && j0r >= 0 && j0r < mg.cols && j1r < mg.cols;  // top-left in range, region fits the buffer (getSubmap)
    const double cornerY = cell_pos(mg.baseY, mg.res, j0r) - (-(0.5 * mg.res));
    const double subLenY = static_cast<double>(e.njr) * mg.res;
    const double subOrgY = 0.5 * subLenY;
    const double subPosY = cornerY - subOrgY;
    okY = okY && within_axis(ny, subOrgY, subPosY, subLenY);
    e.sbaseY = subPosY + (subOrgY - 0.5 * mg.res);
    const int rightCol = e.njr - 1;
    e.yA = cell_pos(e.sbaseY, mg.res, (rightCol + 1) >> 1);
    e.yB = cell_pos(e.sbaseY, mg.res, rightCol >> 1);
    if (okY) flags |= 1;
    // 3x3-only kernels (leg_fast8m): getIndex(centre) is the column behind the disc box's first one — with a three-column box, its middle
    if constexpr (std::is_same<PC, YFillConsts>::value) flags |= (idx[2] == idx[0] + 1) ? kYCentreMid : 0;
    e.flags = flags;
    // reference rectangle polygon (getSearchPolygon, cpp:2496-2517): y limits centre -+ 0.5 * r
    {
        const double yhi = ny + 0.5 * r, ylo = ny - 0.5 * r;
        double qh = floor((mg.baseY - yhi) * mg.rinv), ql = floor((mg.baseY - ylo) * mg.rinv);
        qh = fmin(fmax(qh, -1.0e9), 1.0e9);
        ql = fmin(fmax(ql, -1.0e9), 1.0e9);
        const int eh = static_cast<int>(qh), el = static_cast<int>(ql);
        const bool p0 = cell_pos(mg.baseY, mg.res, eh) < yhi, p1 = cell_pos(mg.baseY, mg.res, eh + 1) < yhi;
        const bool q1 = cell_pos(mg.baseY, mg.res, el + 1) >= ylo, q0 = cell_pos(mg.baseY, mg.res, el) >= ylo;
        e.jA = p0 ? eh : (p1 ? eh + 1 : eh + 2);
        e.jB = q1 ? el + 1 : (q0 ? el : el - 1);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double dy = cell_pos(mg.baseY, mg.res, e.j0d + k) - ny;
        e.dy2[k] = dy * dy;
    }
    const int jw0 = e.jc - pc.winH;
    e.rmask = range_word(e.j0r - jw0, e.j0r - jw0 + e.njr - 1, 0);
    e.pmask = range_word(e.jA - jw0, e.jB - jw0, 0);
}

// One swing leg of one phase, 8 lanes per leg, y side from the YEntry.  The x side is ONE lane-transposed pass: lane
// q evaluates the index of one box corner — 0/1 foot disc (cx +- rf), 2/3 centroid rectangle (cx +- lx / 2),
// 4 getIndex(cx), 5/6 default-track disc (nx0 +- rf) — by prediction (PlanConsts::cornerEps); when any lane of the
// wavefront is within rounding distance of a cell boundary, or outside the map, the wavefront evaluates the
// reference's own expressions (corner_quantity) instead.
template <int NRL, bool kMid>
__device__ __forceinline__ void leg_phase_bits8(const DevMap& m, const BitMap& bm, const PlanConsts& pc, const SpiralLut& lut,
                                                const LutHead& head, PoseShared& sh, const LegBits& lb, const Grp<8>& g, int leg,
                                                const LegStatic& ls, const YEntry& ye, double ctr0, double ctr1, double ctr2,
                                                double advance, int cyc, const fpe_plan_out& out, LegCommit* lc,
                                                typename std::conditional<kMid, Unit, UnitG>::type* unit) {
    constexpr int G = 8, KW = 1;
    // heights and records are deposited in `unit` and finished by flush_unit (3x3-only kernels, every eighth cycle) /
    // flush_unit_g (generic kernels, every fourth cycle)
    uint32_t ugFlags = 0u, ugVisA = 0u, ugVisB = 0u;  // generic kernels: UnitG fields in the making
    int ugAI0 = 0, ugAJ0 = 0, ugANj = 1, ugBI0 = 0, ugBJ0 = 0, ugBNj = 1;
    const float Rf = ls.Rf;
    const int polyKind = ls.polyKind;
    const LegConst& lk = ls.lk;
    const double biasX = ls.biasX;
    // next default positions of this leg on the three tracks (cpp:2199-2213, 2270-2284)
    const double nx0 = (ctr0 + advance) + biasX;  // cpp:2199, 2414
    const double nx1 = (ctr1 + advance) + biasX;
    const double nx2 = (ctr2 + advance) + biasX;
    const double ny = ye.ny;  // (initialPose_[1] + ajustedPose_[1]) + bias.y, identical on the three tracks (cpp:2201)
    if (polyKind != 0 && g.sub == 0) {  // hexagon vertices from the NOMINAL track's position (build-defined, App. E)
        const double r = static_cast<double>(Rf);
        double* vx = sh.polyX[leg];
        double* vy = sh.polyY[leg];
        const double hx = 0.5 * r;
        const double hy = (0.5 * r) * 0.8660254037844386;
        vx[0] = nx2 + r;   vy[0] = ny;
        vx[1] = nx2 + hx;  vy[1] = ny - hy;
        vx[2] = nx2 - hx;  vy[2] = ny - hy;
        vx[3] = nx2 - r;   vy[3] = ny;
        vx[4] = nx2 - hx;  vy[4] = ny + hy;
        vx[5] = nx2 + hx;  vy[5] = ny + hy;
    }
    LegCtx c;
    c.cyc = cyc;
    c.cx = nx1;  // centre from the CENTROID track (cpp:861-862)
    c.cy = ny;
    c.nv = (polyKind == 0) ? 4 : 6;
    {
        const double r = static_cast<double>(Rf);  // getSearchPolygon's rectangle around the NOMINAL track (cpp:2496-2517)
        c.rect = polyKind == 0;
        c.xhi = nx2 + r;
        c.xlo = nx2 - r;
        c.yhi = ny + 0.5 * r;
        c.ylo = ny - 0.5 * r;
    }
    c.vx = sh.polyX[leg];
    c.vy = sh.polyY[leg];
    c.footDa = sh.footDa;
    c.footDb = sh.footDb;
    c.footOff = sh.footOff;
    c.R2 = lk.R2;
    c.nRings = lk.nRings;
    c.nCand = lk.nCand;
    c.ti0 = c.tj0 = 0;
    c.ici = c.icj = 0;

    NominalOut no;
    CentroidOut co;
    float zDefault = static_cast<float>(static_cast<double>(0.0f) + pc.h);  // value when no cell is visited
    float* scratch = reinterpret_cast<float*>(lb.a);
    const bool wantDefault = out.default_next != nullptr;
    const bool usable = (ye.flags & 2) != 0 && fabs(c.cx) <= 1e6;  // centre_usable(c.cx, c.cy)
    if (!ls.radiusOk || !usable) {
        nominal_invalid(no, c.cx, c.cy, ls.radiusOk ? 2 : 3);
        co.x = co.y = 0.0; co.z = 0.0f; co.row = co.col = -1; co.code = 6;
        if (wantDefault && centre_usable(nx0, ny)) {  // cpp:2289-2301 (leg search skipped: radius / centre unusable)
            const BBox dbox = circle_bbox_fast(m.g, nx0, ny, pc.rf);
            bool unused;
            zDefault = disc_pass_direct<G, false>(m, pc, nx0, ny, dbox, g, unused, scratch);
        }
        if constexpr (kMid) {
            if (g.sub == 0) {
                unit->visA = 0x80000000u;  // the nominal leg is invalid: its height is never used
                unit->eA[0] = 0.0f;
                unit->visB = 0x80000000u;
                unit->eB[0] = zDefault;
                unit->eC = 0.0f;
            }
        } else {
            ugFlags = kUgPreA | kUgPreB;
            ugVisA = __float_as_uint(0.0f);
            ugVisB = __float_as_uint(zDefault);
        }
    } else {
        // ---- x side: one corner quantity per lane ----
        const int q = g.sub;
        const double cq = (q == 5 || q == 6) ? nx0 : c.cx;
        const bool rawq = q == 4 || q == 7;
        const double hq = (q == 2 || q == 3) ? 0.5 * lk.lx : (rawq ? 0.0 : pc.rf);
        const bool minus = q == 1 || q == 3 || q == 6;
        const double xq = rawq ? cq : (minus ? cq - hq : cq + hq);
        int idxq;
        bool withinq = true;
        {
            const double n = (xq - m.g.orgX) - m.g.posX;
            const double qf = n * m.g.rinv;
            const double k = trunc(qf);
            const double fr = fabs(qf - k);
            bool safe = fr > pc.cornerEps && fr < 1.0 - pc.cornerEps;
            // strictly inside the map: boundPositionToRange only rewrites the position (no clamp), within stays true
            if (!rawq) safe = safe && qf < -pc.cornerEps && qf > pc.cornerEps - static_cast<double>(m.g.rows);
            idxq = -static_cast<int>(k);
            if (__ballot(!safe) != 0ull) {  // wave-uniform, rare: the reference's own expressions
                const Box bq{cq, 0.0, hq, 0.0};
                const CornerVal cv = corner_quantity(m.g, minus ? 2 : 0, bq, rawq);
                idxq = cv.idx;
                withinq = cv.within;
            }
        }
        constexpr int kKeep = (~(G - 1)) & 0x1F;
        BBox bb, rbox, dbox;
        bb.i0 = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (0 << 5));
        bb.ni = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (1 << 5)) - bb.i0 + 1;
        rbox.i0 = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (2 << 5));
        rbox.ni = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (3 << 5)) - rbox.i0 + 1;
        c.ici = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (4 << 5));
        dbox.i0 = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (5 << 5));
        dbox.ni = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (6 << 5)) - dbox.i0 + 1;
        bb.j0 = dbox.j0 = ye.j0d;
        bb.nj = dbox.nj = ye.njd;
        rbox.j0 = ye.j0r;
        rbox.nj = ye.njr;
        c.icj = ye.jc;
        const unsigned wbits = static_cast<unsigned>(g.ballot(withinq));
        // getSubmapInformation's tail (submap_from_corners), x part here, y part from the entry
        Submap sm;
        sm.i0 = rbox.i0;
        sm.j0 = rbox.j0;
        sm.ni = rbox.ni;
        sm.nj = rbox.nj;
        {
            const bool okX = (wbits & 0xCu) == 0xCu && sm.i0 >= 0 && sm.i0 < m.g.rows && sm.i0 + sm.ni <= m.g.rows;  // (region fits the buffer)
            const double cornerX = cell_pos(m.g.baseX, m.g.res, sm.i0) - (-(0.5 * m.g.res));
            const double subLenX = static_cast<double>(sm.ni) * m.g.res;
            const double subOrgX = 0.5 * subLenX;
            const double subPosX = cornerX - subOrgX;
            sm.ok = okX && (ye.flags & 1) != 0 && within_axis(c.cx, subOrgX, subPosX, subLenX);
            sm.baseX = sm.ok ? subPosX + (subOrgX - 0.5 * m.g.res) : 0.0;
            sm.baseY = sm.ok ? ye.sbaseY : 0.0;
        }
        const int iw0 = c.ici - pc.winH, jw0 = c.icj - pc.winH;
        // one memory round trip: the window's bit rows and the elevation of the two discs around known centres
        uint4 grp[NRL][KW + 1];
        win_issue<G, NRL, KW>(bm, m.g, g, iw0, jw0, grp);
        DiscLoads dc, dd;
        const bool dfltUsable = wantDefault && fabs(nx0) <= 1e6;
        uint32_t rowA = 0u, rowB = 0u;     // generic kernels: membership of the two discs, lane = box row
        bool rowsA = false, rowsB = false;  // ... when every box of the wavefront has at most 8 x 8 = 32 cells
        if constexpr (kMid) {
            disc_issue<G, false, kMid, kMid>(m, pc, c.cx, c.cy, bb, g, dc, ye.dy2);
            if (dfltUsable) disc_issue<G, false, kMid, kMid>(m, pc, nx0, ny, dbox, g, dd, ye.dy2);
        } else {
            dc.pipelined = dd.pipelined = false;
            dc.mid = dd.mid = false;
            const bool fitA = bb.ni <= 8 && bb.nj <= 8 && bb.ni * bb.nj <= 32;
            const bool fitB = !dfltUsable || (dbox.ni <= 8 && dbox.nj <= 8 && dbox.ni * dbox.nj <= 32);
            rowsA = __ballot(!fitA) == 0ull;
            rowsB = __ballot(!fitB) == 0ull;
            if (rowsA || rowsB) disc_rows8(m.g, pc.rf2, c.cx, nx0, c.cy, bb, dbox, g, rowA, rowB);
        }
        WinRows<NRL, KW> w;
        win_finish<NRL, KW>(jw0, grp, w);
#pragma unroll
        for (int k = 0; k < NRL; ++k) lb.a[g.sub + G * k] = w.Df[k][0];
        const CentroidScan sc = rows_from_bits<G, NRL, KW>(sm, w, g, iw0, jw0);
        bits_sync<G>();
        bool defaultOk;
        if constexpr (kMid) {
            defaultOk = default_ok_bits<G, KW, kMid>(m, pc, c.cx, c.cy, bb, dc, lb.a, lb.rows, iw0, jw0, g);  // cpp:2012
        } else {
            defaultOk = rowsA ? default_ok_rows8(rowA, bb, lb.a, lb.rows, iw0, jw0, g)
                              : default_ok_bits<G, KW, kMid>(m, pc, c.cx, c.cy, bb, dc, lb.a, lb.rows, iw0, jw0, g);
        }
        bits_sync<G>();  // lb doubles as scratch below
        float zCentre = 0.0f;
        if constexpr (kMid) {
            uint32_t visA = 0u, visB = 0u;
            unit_put_disc<true>(m, pc, c.cx, c.cy, bb, g, dc, unit->eA, visA, scratch);
            if (dfltUsable) unit_put_disc<true>(m, pc, nx0, ny, dbox, g, dd, unit->eB, visB, scratch);
            if (g.sub == 0) {
                unit->visA = visA;
                unit->visB = visB;
            }
        } else {
            bool pre;
            if (rowsA) {
                ugVisA = box_mask_from_rows8(rowA, bb.nj, g);
            } else {
                unitg_put_disc(m, pc, c.cx, c.cy, bb, g, dc, ugVisA, pre, scratch);  // (not pipelined: the direct pass)
                if (pre) ugFlags |= kUgPreA;
            }
            ugAI0 = bb.i0; ugAJ0 = bb.j0; ugANj = max(bb.nj, 1);
            if (dfltUsable) {
                if (rowsB) {
                    ugVisB = box_mask_from_rows8(rowB, dbox.nj, g);
                } else {
                    unitg_put_disc(m, pc, nx0, ny, dbox, g, dd, ugVisB, pre, scratch);
                    if (pre) ugFlags |= kUgPreB;
                }
                ugBI0 = dbox.i0; ugBJ0 = dbox.j0; ugBNj = max(dbox.nj, 1);
            } else {
                ugFlags |= kUgPreB;
                ugVisB = __float_as_uint(zDefault);
            }
        }
        constexpr bool kOneCell = kMid;  // the 3x3-only variants are launched for one-cell foot discs
        CentroidPendingBits cp;
        centroid_begin_bits<kOneCell>(m, c, sm, sc, zCentre, cp, ye.yA, ye.yB);                         // cpp:818-821
        if (defaultOk) {
            no.valid = 1;
            no.source = 0;
            no.row = c.ici;
            no.col = c.icj;
            no.x = c.cx;  // cpp:2016-2017
            no.y = c.cy;
            no.z = zCentre;
        } else {
            nominal_invalid(no, c.cx, c.cy, 2);
            int wi = 0, wj = 0;
            bits_sync<G>();
            if (spiral_bits<G, NRL, KW, kMid>(m, pc, lut, head, c, w, lb, g, iw0, jw0, wi, wj, &ye)) {  // cpp:2022
                no.valid = 1;
                no.source = 1;
                no.row = wi;
                no.col = wj;
                no.x = cell_pos(m.g.baseX, m.g.res, wi);  // cpp:2105-2107
                no.y = cell_pos(m.g.baseY, m.g.res, wj);
                no.z = zCentre;  // z at the DEFAULT centre even for a candidate (cpp:2029)
            }
            bits_sync<G>();
        }
        if constexpr (kMid) {
            if (g.sub == 0) unit->eC = cp.e0;
            cp.o.z = 0.0f;
            if (g.sub == 0) unit->cenCode = static_cast<uint32_t>(cp.o.code) | (cp.needDisc != 0 ? 0x100u : 0u);
        } else {
            cp.o.z = 0.0f;
            if (cp.needDisc != 0) ugFlags |= kUgCTable;   // the result's own cell-centred disc (offset table)
            else if (cp.o.code == 0) ugFlags |= kUgCIsA;  // whole region valid: the height at the centre (cpp:1687)
        }
        co = cp.o;
    }
    lc->valid = no.valid;
    lc->v[0][0] = nx0;   lc->v[0][1] = ny;    lc->v[0][2] = static_cast<double>(zDefault);
    lc->v[1][0] = co.x;  lc->v[1][1] = co.y;  lc->v[1][2] = static_cast<double>(co.z);
    lc->v[2][0] = no.x;  lc->v[2][1] = no.y;  lc->v[2][2] = static_cast<double>(no.z);
    if constexpr (!kMid) {
        if (g.sub == 0) {  // what flush_unit_g needs to rebuild this leg's four records
            UnitG u;
            u.cx = c.cx; u.cenX = co.x; u.defX = nx0;
            u.aI0 = ugAI0; u.aJ0 = ugAJ0; u.visA = ugVisA;
            u.bI0 = ugBI0; u.bJ0 = ugBJ0; u.visB = ugVisB;
            u.nomRow = no.row; u.nomCol = no.col; u.cenRow = co.row; u.cenCol = co.col;
            u.flags = static_cast<uint32_t>(co.code) | (no.valid ? kUgValid : 0u) | (static_cast<uint32_t>(no.source) << kUgSrcShift) | ugFlags |
                      (static_cast<uint32_t>(ugANj) << 16) | (static_cast<uint32_t>(ugBNj) << 24);
            u.pad[0] = u.pad[1] = u.pad[2] = 0u;
            *unit = u;
        }
    } else {
        if (g.sub == 0) {  // what flush_unit needs to rebuild this leg's four records
            unit->nomRow = no.row;
            unit->nomCol = no.col;
            unit->nomFlags = static_cast<uint32_t>(no.valid) | (static_cast<uint32_t>(no.source) << 8);
            unit->cenRow = co.row;
            unit->cenCol = co.col;
            if (!(!ls.radiusOk || !usable)) {
                // (cenCode was written above)
            } else {
                unit->cenCode = static_cast<uint32_t>(co.code);
            }
            unit->cx = c.cx;
            unit->cenX = co.x;
            unit->defX = nx0;
        }
    }
}

// The common case of the 3x3-only kernels as straight-line code: every swing leg of the wavefront has a usable centre,
// its two foot-disc boxes are unclamped 3x3 boxes (the middle cell is inside the disc whatever the centre,
// PlanConsts::midCellInside) and the default track is wanted and usable.  No LDS hand-offs besides the spiral's pass
// rows: the default check is evaluated by the lanes that OWN the three window rows of the box against the ballot of
// the membership tests; loads are unconditional; the centroid case logic is a chain of selects.  Any other situation
// (map border, unusable centre, missing products) sends the whole wavefront through leg_phase_bits8 for this phase.
// Constants of the fast path held in VECTOR registers for the whole kernel: as kernel arguments they live in scalar
// memory, and with more uniform state than SGPRs the compiler re-fetches them (s_load + wait) inside the cycle loop.
struct HotConsts {
    double rf, rf2, cornerEps, oneMinusEps, drift;
};
// Lane roles of the x pass.  Lane q of a leg group evaluates the index of ONE box corner — 0/1 centre disc (cx -+ rf),
// 2/3 centroid rectangle (cx -+ lx / 2), 4 getIndex(cx), 5/6 default-track disc (nx0 -+ rf); lane 7 evaluates nothing
// — and, before that, the feet-polygon centre of the track its corner belongs to (centroid track on lanes 0-4, default
// track on 5-6, nominal track on 7), so that indices and positions reach the other lanes in ONE exchange.  The
// per-lane constants live in vector registers, computed once: written as selects on q inside the cycle loop they are
// rebuilt every cycle, and a chain of `q == k` tests is compiled into a switch, i.e. into exec-mask branches.
struct LaneRole {
    double hqS;       // signed half extent of the lane's corner: xq = (track position) + hqS
    double qLo, qHi;  // the predicted quotient of a box corner must lie strictly inside the map (raw lanes: unbounded)
};
__device__ __forceinline__ int lane_track(int q) { return (q == 5 || q == 6) ? 0 : (q == 7 ? 2 : 1); }
__device__ __forceinline__ LaneRole make_lane_role(int q, double rf, double lx, double cornerEps, double rowsD) {
    LaneRole r;
    const double inf = __builtin_huge_val();
    const bool raw = q == 4 || q == 7;
    const double h = (q == 2 || q == 3) ? 0.5 * lx : (raw ? 0.0 : rf);
    const bool minus = q == 1 || q == 3 || q == 6;
    r.hqS = in_vgpr(minus ? -h : h);
    r.qLo = in_vgpr(raw ? -inf : cornerEps - rowsD);
    r.qHi = in_vgpr(raw ? inf : -cornerEps);
    return r;
}
// The first two rounds of the candidate scan (ranks 0-15) WITHOUT the LDS: those sixteen cells lie within two rows and
// columns of the centre (rings 0, 1 and the head of ring 2: SpiralLut::fast16), i.e. in FIVE consecutive window rows, and
// a group's eight lanes own eight consecutive rows per slot — so every one of the five rows has its own lane.  That lane
// looks at the five pass bits around the centre column of ITS row and turns each into the bit (1 << rank) of the
// candidate it stands for (rowTab: the rank per column offset, fetched once per kernel); an OR over the group (three
// DPP steps) gives the sixteen candidates' verdicts, the lowest set bit is the first valid cell in SpiralIterator order
// (cpp:2085-2114), and its offset comes out of two packed 64-bit tables.  Before: the pass rows written to the leg's
// LDS, a fence, two dependent LDS reads, two ballots and a ds_bpermute per search — four LDS round trips that the two
// wavefronts of a SIMD cannot hide (stage trace: 1 150 clocks per search, 88 % of the headline's cycles have one).
struct FastRanks {
    uint32_t rowTab;          // this lane's row: five 5-bit ranks by column offset -2..2 (31: none), 0x1FFFFFF when the lane owns none of the five rows
    int slot;                 // which of the lane's NRL rows it is
    unsigned long long di, dj;  // (offset + 2) of rank q in the 4-bit field q
};
template <int NRL>
__device__ __forceinline__ FastRanks load_fast_ranks(const SpiralLut& lut, const Grp<8>& g, int winH) {
    FastRanks fr;
    fr.slot = 0;
    int d = 99;
#pragma unroll
    for (int k = 0; k < NRL; ++k) {
        const int dk = g.sub + 8 * k - winH;  // row offset from the centre row (window row winH)
        const bool mine = dk >= -2 && dk <= 2;
        fr.slot = mine ? k : fr.slot;
        d = mine ? dk : d;
    }
    const uint32_t w = lut.fast16[min(max(d + 2, 0), 4)];
    fr.rowTab = d == 99 ? 0x1FFFFFFu : w;
    fr.di = *reinterpret_cast<const unsigned long long*>(lut.fast16 + 6);
    fr.dj = *reinterpret_cast<const unsigned long long*>(lut.fast16 + 8);
    asm volatile("" : "+v"(fr.di), "+v"(fr.dj));  // (uniform, but kept in vector registers: the chain has no scalar registers to spare)
    return fr;
}

// The argument segment of plan_bits_kernel<NRL, true, kProd> as a struct (see SeqKernArgs, fpe_bits_seq.hpp; a static_assert behind the
// kernel checks the mirror).  What the cycle loop reads in every cycle — the layer and plane pointers, the map's size, winH —
// the kernel takes from its parameters: scalar registers for the whole chain.  What it reads once per eight cycles (the
// flush: h, the seven product pointers) or in a rare branch (the general leg search: the rank tables, every plan constant) it
// loads through mid_cold_args() where it uses it: held across the chain these were scalar registers the allocator parked in
// lanes of two vector registers and read back, sixteen lane reads per flush and per rare branch for the product pointers alone.
struct MidKernArgs {
    const fpe_pose* poses;
    int B, nCycles;
    DevMap m;
    BitMap bm;
    PlanMidConsts pc;
    SpiralLut lut;
    fpe_plan_out out;
};
// the argument segment through a pointer the optimiser cannot see through: the loads stay where they are written
__device__ __forceinline__ const MidKernArgs* mid_cold_args() {
    typedef const MidKernArgs __attribute__((address_space(4))) * KernArgPtr;
    KernArgPtr ka4 = (KernArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka4));
    return (const MidKernArgs*)ka4;
}
// The PlanConsts view of the block for the general leg search (leg_phase_bits8<NRL, true>, spiral_bits<8, NRL, 1, true> and what
// they call: disc_issue / disc_pass_direct without the threshold check, default_ok_bits, unit_put_disc, centroid_begin_bits
// with a one-cell disc), which the generic kernels share.  Those read rf, rf2, h, winH, cornerEps, nFoot and midCellInside.
// Everything else stays ZERO and must not be read on this path:
//   footReach            0 is also its value for the one-cell disc these kernels are launched for (select_plan_kernel: nFoot == 1,
//                        offset (0, 0)); read by spiral_bits under G == 64 or KW > 1 only
//   nHW, hwList, hwIdx, footDa, footDb   the erosion is compiled out (kOneCellFoot); the offset table is PoseShared's
//   thrDefault, thrCandidate, footRobust, tile*   direct kernels only (every call here has kCheck == false)
//   searchRadius .. defNCand, the stance and step constants   prologue only (the kernel reads them from PlanMidConsts itself)
// A new read of one of these in the shared functions has to add the field to PlanMidConsts and to this view.
__device__ __forceinline__ PlanConsts plan_consts_of(const PlanMidConsts& k) {
    PlanConsts pc{};
    pc.rf = k.rf;
    pc.rf2 = k.rf2;
    pc.h = k.h;
    pc.winH = k.winH;
    pc.cornerEps = k.cornerEps;
    pc.nFoot = 1;
    pc.footReach = 0;
    pc.midCellInside = k.midCellInside;
    return pc;
}

// kPlain: the wavefront's poses are plain (plan_bits_kernel: trot, no radius override, rectangle polygons): ls.Rf and lk.* are the
// uniform plan constants (scalar values: no ballot over them), radiusOk and the rectangle are compile-time facts.
template <int NRL, bool kNoDefault, int kProd, bool kPlain>
__device__ __forceinline__ void leg_fast8m(const DevMap& m, const BitMap& bm, int winH, bool wantDefaultArg, const HotConsts& hc, const LaneRole& role,
                                           const FastRanks& fk,
                                           const LutHead& head, PoseShared& sh, const LegBits& lb, const Grp<8>& g,
                                           int leg, const LegStatic& ls, const YEntry& yeIn, double myCtr, double advance, int cyc,
                                           LegCommit* lc, Unit* unit) {
    constexpr int G = 8, KW = 1;
    const LegConst& lk = ls.lk;
    // the entry's scalar fields in ONE batch of LDS reads (scattered reads would each wait for their own round trip);
    // dy2 stays in LDS (lane-dependent index)
    const YEntry& yeLds = yeIn;
    YEntry ye;
    ye.jc = yeLds.jc; ye.j0d = yeLds.j0d; ye.njd = yeLds.njd; ye.j0r = yeLds.j0r;
    ye.njr = yeLds.njr; ye.jA = yeLds.jA; ye.jB = yeLds.jB; ye.flags = yeLds.flags;
    ye.ny = yeLds.ny; ye.sbaseY = yeLds.sbaseY; ye.yA = yeLds.yA; ye.yB = yeLds.yB;
    ye.rmask = yeLds.rmask; ye.pmask = yeLds.pmask;
    // ---- x side: this lane's track position and corner (cpp:2199, 2414; see leg_phase_bits8) ----
    const double nxq = (myCtr + advance) + ls.biasX;
    const double ny = ye.ny;
    // (kNoDefault: the launch writes no default-track product — compile-time, see specialise_products: the default-track disc is
    // neither loaded nor tested; its lanes of the x pass still run, in the same instructions as the others)
    const bool wantDefault = kNoDefault ? false : wantDefaultArg;
    const double xq = nxq + role.hqS;  // a - h == a + (-h)
    const double qf = ((xq - m.g.orgX) - m.g.posX) * m.g.rinv;
    const double kq = trunc(qf);
    const double fr = fabs(qf - kq);
    const bool safe = (fr > hc.cornerEps && fr < hc.oneMinusEps && qf < role.qHi && qf > role.qLo) || g.sub == 7;
    const int idxq = -static_cast<int>(kq);
    constexpr int kKeep = (~(G - 1)) & 0x1F;
    const int i0d = bcast8_dpp<0>(idxq);
    const int i1d = bcast8_dpp<1>(idxq);
    const int i0r = bcast8_dpp<2>(idxq);
    const int i1r = bcast8_dpp<3>(idxq);
    const int ici = bcast8_dpp<4>(idxq);
    const int i0f = bcast8_dpp<5>(idxq);
    const int i1f = bcast8_dpp<6>(idxq);
    const double cx = bcast8_dpp_f64<0>(nxq);   // centre from the CENTROID track (cpp:861-862)
    const double nx0 = bcast8_dpp_f64<5>(nxq);  // default track
    const double nx2 = bcast8_dpp_f64<7>(nxq);  // nominal track (search polygon)
    const int j0d = ye.j0d, icj = ye.jc;
    // the window rows are requested before anything else looks at the indices (win_issue clamps whatever it is given;
    // the rare path below discards them): the round trip runs under the box tests, the ballot and the submap arithmetic
    const int iw0 = ici - winH, jw0 = icj - winH;
    uint4 grp[NRL][KW + 1];
    win_issue<G, NRL, KW>(bm, m.g, g, iw0, jw0, grp);
    // both foot-disc boxes: 3x3 and clear of the map's outermost rows / columns (not clamped, inside the map)
    // (bitwise: a short-circuit chain is compiled into exec-mask branches)
    const int lowest = kNoDefault ? min(i0d, j0d) : min(min(i0d, i0f), j0d), lastRow = (kNoDefault ? i0d : max(i0d, i0f)) + 4;
    const bool boxF = kNoDefault ? true : ((i1f - i0f) == 2);
    const bool boxes = ((i1d - i0d) == 2) & boxF & (ye.njd == 3) & (lowest >= 1) & (lastRow <= m.g.rows) & (j0d + 4 <= m.g.cols);
    // (kNoDefault: lanes 5-6 evaluate default-track corners nobody reads: their `safe` / magnitude tests do not count)
    const bool dfltLane = (g.sub == 5) | (g.sub == 6);
    const bool laneOk = kNoDefault ? (dfltLane | (safe & (fabs(nxq) <= 1e6))) : (safe & (fabs(nxq) <= 1e6));
    const bool rare = (!kPlain & !ls.radiusOk) | ((ye.flags & (2 | kYCentreMid)) != (2 | kYCentreMid)) | !laneOk | (!kNoDefault & !wantDefault) | !boxes;
    if (FPE_RARE(__ballot(rare) != 0ull)) {  // wave-uniform
        const double ctr0 = swizzle_f64<kKeep | (5 << 5)>(myCtr), ctr1 = swizzle_f64<kKeep | (0 << 5)>(myCtr),
                     ctr2 = swizzle_f64<kKeep | (7 << 5)>(myCtr);
        // (rare: the plan constants, the rank tables and the product pointers from the argument segment, here)
        const MidKernArgs* ka = mid_cold_args();
        const PlanConsts pcR = plan_consts_of(ka->pc);
        const fpe_plan_out outR = specialise_products<kProd>(ka->out);
        leg_phase_bits8<NRL, true>(m, bm, pcR, ka->lut, head, sh, lb, g, leg, ls, yeIn, ctr0, ctr1, ctr2, advance, cyc, outR, lc, unit);
        return;
    }
    // getSubmapInformation's tail, x part (corners strictly inside the map: within); y part from the entry
    Submap sm;
    sm.i0 = i0r;
    sm.j0 = ye.j0r;
    sm.ni = i1r - i0r + 1;
    sm.nj = ye.njr;
    {
        const double cornerX = cell_pos(m.g.baseX, m.g.res, sm.i0) - (-(0.5 * m.g.res));
        const double subLenX = static_cast<double>(sm.ni) * m.g.res;
        const double subOrgX = 0.5 * subLenX;
        const double subPosX = cornerX - subOrgX;
        sm.ok = (ye.flags & 1) != 0 && within_axis(cx, subOrgX, subPosX, subLenX);
        sm.baseX = subPosX + (subOrgX - 0.5 * m.g.res);
        sm.baseY = ye.sbaseY;
    }
    // ---- same round trip: membership (lane = cell t of the 3x3 boxes) and elevation (lane = box row) of both discs ----
    const int t = g.sub + (g.sub >= 4 ? 1 : 0);
    const int a = t >= 6 ? 2 : (t >= 3 ? 1 : 0);
    const int bq = t - 3 * a;
    const double dy2 = yeLds.dy2[bq];
    const double dxA = cell_pos(m.g.baseX, m.g.res, i0d + a) - cx;
    const double dxB = cell_pos(m.g.baseX, m.g.res, i0f + a) - nx0;
    const bool visA = (dxA * dxA + dy2) <= hc.rf2;  // CircleIterator::isInside (cell_in_disc)
    const bool visB = kNoDefault ? false : (dxB * dxB + dy2) <= hc.rf2;
    // The elevations for flush_unit, a box ROW per lane: lane L reads row min(L >> 1, 2) of the centre disc's box (even L) or of
    // the default-track disc's (odd L; kNoDefault: every lane the centre disc's) with ONE 12-byte load — 4-byte aligned; inside
    // the map: `boxes` above, and the rare path has left — and deposits it with one LDS store pair; lanes 6 and 7 repeat lanes 4
    // and 5 (the same value to the same address: no predicate).  By cell — lane = cell t, the middle cell apart — it is four loads,
    // four address sums and four LDS stores a cycle; the <4, true, *> instances, at the cap of 256 vector registers, keep that
    // form (by row: five registers spilled, 24 bytes of scratch).
    // (32-bit cell offsets from the uniform layer base: bits_supported bounds the layer below 2 GiB)
    constexpr bool kByRow = NRL < 4;
    const unsigned colsU = static_cast<unsigned>(m.g.cols);
    const int rowL = min(g.sub >> 1, 2);
    const bool laneB = !kNoDefault && (g.sub & 1) != 0;
    UnitRow3 eRow = {};
    float eA = 0.0f, eMidA = 0.0f, eB = 0.0f, eMidB = 0.0f;
    if constexpr (kByRow) {
        const unsigned boxRowCell = __umul24(static_cast<unsigned>((laneB ? i0f : i0d) + rowL), colsU) + static_cast<unsigned>(j0d);
        eRow = *reinterpret_cast<const UnitRow3*>(reinterpret_cast<const char*>(m.elev) + static_cast<size_t>(boxRowCell << 2));
    } else {
        const unsigned laneCell = __umul24(static_cast<unsigned>(a), colsU) + static_cast<unsigned>(bq);
        const unsigned boxA = __umul24(static_cast<unsigned>(i0d), colsU) + static_cast<unsigned>(j0d);
        const unsigned boxB = __umul24(static_cast<unsigned>(i0f), colsU) + static_cast<unsigned>(j0d);
        eA = load_cell(m.elev, boxA + laneCell);
        eMidA = load_cell(m.elev, boxA + colsU + 1u);
        if constexpr (!kNoDefault) {
            eB = load_cell(m.elev, boxB + laneCell);
            eMidB = load_cell(m.elev, boxB + colsU + 1u);
        }
    }
    // In the shadow of that round trip: whether this lane's row of the five around the centre (FastRanks) lies in the search
    // rectangle, which only a spiral search uses — but most wavefronts have one leg in eight that needs it (88 % of the
    // headline's cycles), and otherwise this would sit on the dependent chain behind the default check.  The rectangle's rows are
    // [min{i : x_i < xhi}, max{i : x_i >= xlo}] (rectangle_index_bounds) and cell centres x_i are non-increasing in i, so row i
    // is one of them iff xlo <= x_i < xhi: the lane tests ITS row's centre, nobody derives the interval's ends (a floor, a
    // clamp and a conversion per end, four corrected estimates over a ballot: fifty instructions a cycle).
    // (one-cell foot disc: what these kernels are launched for, select_plan_kernel)
    bool fastSpiral;  // uniform
    if constexpr (kPlain) fastSpiral = lk.nRings >= 4 && lk.nCand >= 16;  // (the plan's defNRings / defNCand: a scalar test)
    else fastSpiral = __ballot(ls.polyKind != 0 || lk.nRings < 4 || lk.nCand < 16) == 0ull;
    const int iFast = iw0 + g.sub + G * fk.slot;
    const double rS = static_cast<double>(ls.Rf);
    const double xFast = cell_pos(m.g.baseX, m.g.res, iFast);
    // getSearchPolygon around the NOMINAL track (cpp:2496-2517)
    const bool rowInside = (xFast < nx2 + rS) & (xFast >= nx2 - rS);
    WinRows<NRL, KW> w;
    win_finish<NRL, KW>(jw0, grp, w);
    const CentroidScan sc = rows_from_bits<G, NRL, KW>(sm, w, g, iw0, jw0, &ye.rmask);
    // ---- checkDefaultFoothold: the lanes owning the box's three window rows test their Df bits under the members ----
    const unsigned mA = static_cast<unsigned>(g.ballot(visA)), mB = kNoDefault ? 0u : static_cast<unsigned>(g.ballot(visB));
    // the nine membership bits in CircleIterator order (the middle cell is always a member)
    const unsigned visA9 = (mA & 0xFu) | 0x10u | ((mA & 0xF0u) << 1), visB9 = kNoDefault ? 0u : ((mB & 0xFu) | 0x10u | ((mB & 0xF0u) << 1));
    bool fail = false;
    {
        const unsigned sh3 = static_cast<unsigned>(j0d - jw0) & 31u;
#pragma unroll
        for (int k = 0; k < NRL; ++k) {
            const int ar = g.sub + G * k - (i0d - iw0);  // row of the box held in slot k
            const unsigned bitsRow = (visA9 >> (3u * (static_cast<unsigned>(ar) & 3u))) & 7u;
            const unsigned sel = static_cast<unsigned>(ar) < 3u ? bitsRow : 0u;
            fail |= (((w.Df[k][0] >> sh3) & 7u) & sel) != 0u;
        }
    }
    const bool defaultOk = !g.any(fail);  // the middle cell is always visited (cpp:2069-2081: at least one cell)
    // ---- deposits for flush_unit: elevations in CircleIterator order ----
    if constexpr (kByRow) {
        float* eDst = (laneB ? unit->eB : unit->eA) + 3 * rowL;
        eDst[0] = eRow.x;
        eDst[1] = eRow.y;
        eDst[2] = eRow.z;
    } else {
        unit->eA[t] = eA;
        unit->eA[4] = eMidA;  // every lane stores the same value
        if constexpr (!kNoDefault) {
            unit->eB[t] = eB;
            unit->eB[4] = eMidB;
        }
    }
    // ---- centroid method (cpp:1684-1952) as selects ----
    const int bottomRow = sm.ni - 1, rightCol = sm.nj - 1;
    const int minRow = sc.minRow, maxRow = sc.maxRow;
    // (every select below has two ready operands: nested conditionals are compiled into branches)
    const bool top = minRow == 0, bottom = maxRow == bottomRow;
    const bool case1 = top && !bottom;
    const bool case2 = !top && !bottom;
    const bool upper = minRow >= (bottomRow - maxRow);
    const int code23 = upper ? 2 : 3, code51 = bottom ? 5 : 1;
    int code = bottom ? 4 : code23;  // case3 (4) / case2 (2, 3): the first row is not blocked
    code = top ? code51 : code;      // case1 (1) / no case (5)
    code = sc.whole ? 0 : code;
    code = sm.ok ? code : 6;
    const bool useMaxRow = case1 || (case2 && !upper);
    const int rowA = (maxRow + bottomRow + (case1 ? 1 : 0)) >> 1, rowB = (minRow + 1) >> 1;
    const int newRow = useMaxRow ? rowA : rowB;
    const int newCol = (rightCol + (case1 ? 1 : 0)) >> 1;
    const bool whole = code == 0;
    const bool hasCell = static_cast<unsigned>(code - 1) < 4u;
    CentroidOut co;
    co.code = code;
    co.z = 0.0f;
    const double cellX = cell_pos(sm.baseX, m.g.res, newRow);  // cpp:1816
    const double yAB = code == 1 ? ye.yA : ye.yB;
    const double xCell = hasCell ? cellX : 0.0, yCell = hasCell ? yAB : 0.0;
    const int rowCell = hasCell ? sm.i0 + newRow : -1, colCell = hasCell ? sm.j0 + newCol : -1;
    co.x = whole ? cx : xCell;  // cpp:1687
    co.y = whole ? ny : yCell;
    co.row = whole ? ici : rowCell;
    co.col = whole ? icj : colCell;
    // ---- nominal result: the default foothold, else the spiral search (cpp:2012-2029) ----
    NominalOut no;
    no.valid = 1;
    no.source = 0;
    no.row = ici;
    no.col = icj;
    no.x = cx;  // cpp:2016-2017
    no.y = ny;
    no.z = 0.0f;
    if (!defaultOk) {
        nominal_invalid(no, cx, ny, 2);
        const double r = static_cast<double>(ls.Rf);
        int wi = 0, wj = 0;
        bool found = false, searched = false;
        // The usual search as straight-line code: reference rectangle, one-cell foot disc, and the candidates of the
        // first two rounds (ranks 0-15: rings 0-2, whose cells the iterator does not filter when nRings >= 4).  Same
        // evaluation as spiral_bits: x interval as in rectangle_index_bounds, columns from the y entry, pass rows
        // P = ~F | (~C & inside) in the leg's LDS, lowest set ballot bit = first valid cell in spiral order.
        if (fastSpiral) {
            // this lane's row of the five around the centre (FastRanks): pass bits P = ~F | (~C & inside) (cpp:2132-2138)
            unsigned Fs = w.F[0][0], Cs = w.C[0][0];
#pragma unroll
            for (int k = 1; k < NRL; ++k) {
                Fs = fk.slot == k ? w.F[k][0] : Fs;
                Cs = fk.slot == k ? w.C[k][0] : Cs;
            }
            const unsigned inside = rowInside ? ye.pmask : 0u;
            // No cell outside the map among the sixteen: they lie within two rows and columns of the centre cell, and the centre cell
            // is the middle one of the centre disc's 3x3 box — its row because the foot radius is at most one cell and the three
            // corner quotients are clear of the cell boundaries (`safe`), its column by the y entry's flag (kYCentreMid: the y side
            // may have been evaluated ON a cell boundary, by the reference's own expressions) — which `boxes` keeps clear of the
            // map's outermost rows and columns.  So the window may reach over the map's edge here (cells outside pass every test:
            // their F bit is 0) without such a cell being looked at; the general search below masks them itself.
            const unsigned P = ~Fs | (~Cs & inside);
            const unsigned b5 = P >> static_cast<unsigned>(winH - 2);  // bit c = column offset c - 2 from the centre column (winH)
            unsigned m16 = 0u;
#pragma unroll
            for (int c = 0; c < 5; ++c) m16 |= ((b5 >> c) & 1u) << ((fk.rowTab >> (5 * c)) & 31u);  // (rank 31: not a candidate)
            const unsigned all16 = or_reduce8(m16) & 0xFFFFu;
            found = all16 != 0u;
            const unsigned rank4 = static_cast<unsigned>(__builtin_ctz(all16 | 0x10000u) & 15) * 4u;
            wi = ici + static_cast<int>((fk.di >> rank4) & 7ull) - 2;
            wj = icj + static_cast<int>((fk.dj >> rank4) & 7ull) - 2;
            searched = lk.nCand <= 16;  // nothing beyond the sixteen
        }
        if (FPE_RARE(!found && !searched)) {  // other polygons, larger foot discs, small search radii, or no hit in the first two rounds
            LegCtx c;
            c.cyc = cyc;
            c.cx = cx;
            c.cy = ny;
            c.nv = (kPlain || ls.polyKind == 0) ? 4 : 6;
            c.rect = kPlain || ls.polyKind == 0;
            c.xhi = nx2 + r;
            c.xlo = nx2 - r;
            c.yhi = ny + 0.5 * r;
            c.ylo = ny - 0.5 * r;
            c.vx = sh.polyX[leg];
            c.vy = sh.polyY[leg];
            c.footDa = sh.footDa;
            c.footDb = sh.footDb;
            c.footOff = sh.footOff;
            c.R2 = lk.R2;
            c.nRings = lk.nRings;
            c.nCand = lk.nCand;
            c.ti0 = c.tj0 = 0;
            c.ici = ici;
            c.icj = icj;
            if (!kPlain && !c.rect) {  // hexagon vertices from the NOMINAL track's position (build-defined, App. E)
                if (g.sub == 0) {
                    double* vx = sh.polyX[leg];
                    double* vy = sh.polyY[leg];
                    const double hx = 0.5 * r, hy = (0.5 * r) * 0.8660254037844386;
                    vx[0] = nx2 + r;   vy[0] = ny;
                    vx[1] = nx2 + hx;  vy[1] = ny - hy;
                    vx[2] = nx2 - hx;  vy[2] = ny - hy;
                    vx[3] = nx2 - r;   vy[3] = ny;
                    vx[4] = nx2 - hx;  vy[4] = ny + hy;
                    vx[5] = nx2 + hx;  vy[5] = ny + hy;
                }
                bits_sync<G>();
            }
            const MidKernArgs* ka = mid_cold_args();  // (rare: see above)
            const PlanConsts pcR = plan_consts_of(ka->pc);
            found = spiral_bits<G, NRL, KW, true>(m, pcR, ka->lut, head, c, w, lb, g, iw0, jw0, wi, wj, &yeIn);  // cpp:2022
            bits_sync<G>();
        }
        if (found) {
            no.valid = 1;
            no.source = 1;
            no.row = wi;
            no.col = wj;
            no.x = cell_pos(m.g.baseX, m.g.res, wi);  // cpp:2105-2107
            no.y = cell_pos(m.g.baseY, m.g.res, wj);
        }
    }
    if (g.sub == 0) {  // what flush_unit needs to rebuild this leg's four records
        unit->visA = visA9;
        unit->visB = visB9;
        unit->nomRow = no.row;
        unit->nomCol = no.col;
        unit->nomFlags = static_cast<uint32_t>(no.valid) | (static_cast<uint32_t>(no.source) << 8);
        unit->cenRow = co.row;
        unit->cenCol = co.col;
        unit->cenCode = static_cast<uint32_t>(code) | (hasCell ? 0x200u : 0u);  // flush_unit reads the result's own cell
        unit->cx = cx;
        unit->cenX = co.x;
        unit->defX = nx0;
    }
    lc->valid = no.valid;
    lc->v[0][0] = nx0;   lc->v[0][1] = ny;    lc->v[0][2] = 0.0;
    lc->v[1][0] = co.x;  lc->v[1][1] = co.y;  lc->v[1][2] = 0.0;
    lc->v[2][0] = no.x;  lc->v[2][1] = no.y;  lc->v[2][2] = 0.0;
}

}  // namespace

// ---- chained plan on the bit window: 8 lanes per leg, two poses per wavefront ------------------------------------
constexpr int kBitsGenericWaves = 3;  // measured on cfg-4: 2 -> 1.36 ms, 3 -> 1.25 ms (27 spilled VGPRs), 4 -> 1.46 ms (69 spilled)
// Everything of plan_bits_kernel behind the pose loads and the parked constants: the LDS views, the legs' constants, the stance,
// the gate of the first cycle, the cycle loop with its flushes.  kPlain (3x3-only kernels, decided per wavefront by the kernel):
// both poses trot, no leg overrides the search radius, every search polygon is the rectangle — one phase a cycle with all four
// legs swinging (no phase loop, no swing mask), advance = step, and the legs' search constants are the plan's own (uniform).
// kPlain = false is the general code.  Always inlined into the kernel.  kStride (plan_bits_chain_kernel): step and drift are the
// pose's own (sv, and hc.drift filled from it by the kernel) instead of the plan's.  kResume (its resume form, a stride form
// too): with rs.in the prologue takes the pose's committed feet, running drift and cycle index from an earlier call's
// state instead of the stance, and with rs.out the epilogue returns them behind the last flush (fpe_plan_resume*, include/fpe.h).
// (The LDS views and the rank table's head are set up HERE, once per copy, not in the kernel ahead of the verdict: a value both
// copies read has to be computed in front of the branch and stays in its register through either copy, where one copy's own
// value is computed next to its use — with them in the kernel the <4, true, *> instances spilled four vector registers.)
template <int NRL, bool kMid, int kProd, bool kPlain, bool kStride = false, bool kResume = false, class PC>
__device__ __forceinline__ void plan_bits_body(const fpe_pose* pp, int b, bool live, double x0, double y0, double z0, int gait, float rOverride,
                                               int polyKindIn, int nCycles, const DevMap& m, const DevMap& mArg, const BitMap& bm, const PC& pc,
                                               const SpiralLut& lut, const fpe_plan_out& out, const HotConsts& hc, int tid, int slot, int leg,
                                               const StrideVals& sv = StrideVals{}, const ResumeArgs& rs = ResumeArgs{}) {
    static_assert(kMid || !kPlain, "the generic kernels have no plain instance");
    static_assert(!kMid || !kStride, "the 3x3-only kernels have no stride instance");
    static_assert(!kResume || kStride, "a resume instance is a stride instance");
    constexpr int G = 8;
    constexpr bool kNoDefault = kProd == 1;
    constexpr int kPoseThreads = 4 * G;
    constexpr int NR = G * NRL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Grp<G> g(tid);
    const size_t legBytes = 4 * static_cast<size_t>(legbits_words(NR, 1, pc.nHW));
    // cycles between two flushes (units and y entries staged in LDS): eight for the 3x3-only kernels, four for the generic ones
    constexpr int kBatch = kMid ? 8 : 4;
    using UnitT = typename std::conditional<kMid, Unit, UnitG>::type;
    const size_t poseBytes = sizeof(PoseShared) + 4 * legBytes + (sizeof(YEntry) + sizeof(UnitT)) * 4 * kBatch;
    unsigned char* base = smem + static_cast<size_t>(slot) * poseBytes;
    PoseShared& sh = *reinterpret_cast<PoseShared*>(base);
    const LegBits lb = make_legbits(base + sizeof(PoseShared) + static_cast<size_t>(leg) * legBytes, NR, 1);
    YEntry* ytab = reinterpret_cast<YEntry*>(base + sizeof(PoseShared) + 4 * legBytes) + leg * kBatch;  // [cycle % kBatch] of this leg
    UnitT* units = reinterpret_cast<UnitT*>(base + sizeof(PoseShared) + 4 * legBytes + sizeof(YEntry) * 4 * kBatch) + leg * kBatch;

    const LutHead head = load_lut_head(lut, g);
    LegStatic ls;
    {
        if (!kPlain && FPE_RARE_IF(kMid, __ballot(rOverride > 0.0f) != 0ull)) {  // some leg of the wavefront overrides the search radius (build-defined)
            ls = make_leg_static(pc, pp, leg, m.g.res, lut);
        } else {  // the reference's single searchRadius_: constants precomputed on the host
            ls.Rf = pc.searchRadius;
            ls.polyKind = kPlain ? 0 : polyKindIn;
            ls.radiusOk = true;
            const double R = static_cast<double>(pc.searchRadius);
            ls.lk.Rf = pc.searchRadius;
            ls.lk.R2 = R * R;
            ls.lk.nRings = pc.defNRings;
            ls.lk.nCand = pc.defNCand;
            ls.lk.lx = static_cast<double>(pc.searchRadius * 2);
            ls.lk.ly = static_cast<double>(pc.searchRadius);
            // (two selects on the leg's bits: a run-time index into the kernel-argument array is a dependent global load)
            const bool odd = (leg & 1) != 0, high = (leg & 2) != 0;
            const double bxLo = odd ? pc.biasX[1] : pc.biasX[0], bxHi = odd ? pc.biasX[3] : pc.biasX[2];
            const double byLo = odd ? pc.biasY[1] : pc.biasY[0], byHi = odd ? pc.biasY[3] : pc.biasY[2];
            ls.biasX = high ? bxHi : bxLo;
            ls.biasY = high ? byHi : byLo;
        }
    }
    // (loaded values parked here: inside the cycle loop the compiler would wait for "all outstanding loads" at their
    // first use in every iteration)
    if constexpr (kMid) {
        ls.biasX = in_vgpr(ls.biasX);
        ls.biasY = in_vgpr(ls.biasY);
    }
    if constexpr (kMid) {  // launched for one-cell foot discs only: the table is the single offset (0, 0)
        if (tid % kPoseThreads == 0) {
            sh.footDa[0] = 0;
            sh.footDb[0] = 0;
            sh.footOff[0] = 0;
        }
    } else {
        for (int k = tid % kPoseThreads; k < pc.nFoot; k += kPoseThreads) {
            sh.footDa[k] = pc.footDa[k];
            sh.footDb[k] = pc.footDb[k];
            sh.footOff[k] = 0;
        }
    }
    double adjY = 0.0;  // ajustedPose_[1], cpp:759
    int cycBase = 0;    // gait_cycle_id of the call's first cycle
    bool started = true;
    if constexpr (kResume) {
        if (rs.in) {  // (uniform) the state of an earlier call instead of the stance; the padding slot of an odd batch reads pose B-1's
            // chain_resume's text, kept here like the stance below
            started = false;
            const LegState st = load_leg_state(rs.in, b, leg);
            const bool poseFinite = (__ballot(!st.finite) & pose_lane_mask<kPoseThreads>(slot)) == 0ull;  // any non-finite value: the whole state is
            adjY = st.adjY;
            cycBase = st.cycle;
            if (g.sub == 0) {
                for (int t = 0; t < 3; ++t) {
                    sh.cur[t][leg][0] = poseFinite ? st.x[t] : __builtin_nan("");
                    sh.cur[t][leg][1] = st.y[t];
                    sh.cur[t][leg][2] = 0.0;
                }
            }
        }
    }
    // initial stance (cpp:350-378) and first-gait shift (setFirstGait, cpp:2679-2699): chain_stance's text, kept here (through the
    // helpers the instantiations at their register cap were re-allocated: <4, true, *>, <4, false, 1>, the chain forms <3 | 4, 0>)
    if (started && g.sub == 0) {
        double sx = (leg == 0 || leg == 3) ? pc.LbHalf : -pc.LbHalf;
        double sy = (leg <= 1) ? pc.WbHalfNeg : pc.WbHalfPos;
        double sz = 0;
        sx += x0;
        sy += y0;
        sz += z0;
        if (out.stance && live) {
            double* st = out.stance + (static_cast<size_t>(b) * 4 + leg) * 3;
            st[0] = sx;
            st[1] = sy;
            st[2] = sz;
        }
        for (int t = 0; t < 3; ++t) {
            sh.cur[t][leg][0] = sx - (kStride ? sv.stepHalf : pc.stepHalf);
            sh.cur[t][leg][1] = sy;
            sh.cur[t][leg][2] = sz;
        }
    }
    bits_sync<G>();
    // The shifted stance's feet-polygon centre, ONCE: the gate of the first cycle needs it, and so does the first phase of cycle 0 on
    // every lane — sh.cur[0..2] were written identically just above, so whichever track a lane evaluates (myTrack) it would
    // compute this value again, bit for bit.  The tracks diverge with the first commit: every later phase computes its own.
    // Not where the value's two registers, held from here into the loop, do not fit: the <4, true, *> instances sit at the cap of
    // 256 vector registers (three spilled with it, 16 bytes of scratch), the generic ones run at theirs with spills already
    // (<4, false, 2 / 0>: 48 -> 64 / 72 bytes of scratch with it) — those compute the centre at both places, as before.
    constexpr bool kStanceOnce = kMid && NRL < 4;
    double stanceCtr = 0.0;
    if constexpr (kStanceOnce) stanceCtr = polygon_center_x<kMid>(sh.cur[0]);
    if (started && out.pose_status) {
        // getGaitCycleSearchGridMap's getSubmap in the first cycle (opt_gate_cycle0), its four corners on four lanes
        const double gx = (kStanceOnce ? stanceCtr : polygon_center_x<kMid>(sh.cur[0])) + (kStride ? sv.step : pc.step), gy = y0 + 0.0;  // cpp:2327-2329
        Submap gs;
        {
            // lane q & 3: 0 top-left x, 1 top-left y, 2 bottom-right x, 3 bottom-right y — predicted as in the x pass
            // of the chain; the reference's own expressions when any lane is near a cell boundary or the map's edge
            const bool isY = (g.sub & 1) != 0, isBR = (g.sub & 2) != 0;
            const double ctr = isY ? gy : gx, halfExt = isY ? 0.5 * pc.isosWid : 0.5 * pc.isosLen;
            const double org = isY ? m.g.orgY : m.g.orgX, pos = isY ? m.g.posY : m.g.posX;
            const double cells = isY ? static_cast<double>(mArg.g.cols) : static_cast<double>(mArg.g.rows);
            const double vq = isBR ? ctr - halfExt : ctr + halfExt;
            const double qf = ((vq - org) - pos) * m.g.rinv;
            const double kq = trunc(qf);
            const double fr = fabs(qf - kq);
            const bool safe = (fr > pc.cornerEps) & (fr < 1.0 - pc.cornerEps) & (qf < -pc.cornerEps) & (qf > pc.cornerEps - cells);
            if (!FPE_RARE_IF(kMid, __ballot(!safe) != 0ull)) {
                const int idxq = -static_cast<int>(kq);
                constexpr int kKeep = (~(G - 1)) & 0x1F;
                BBox gbb;
                gbb.i0 = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (0 << 5));
                gbb.j0 = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (1 << 5));
                gbb.ni = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (2 << 5)) - gbb.i0 + 1;
                gbb.nj = __builtin_amdgcn_ds_swizzle(idxq, kKeep | (3 << 5)) - gbb.j0 + 1;
                gs = submap_from_corners(m.g, gbb, true, gx, gy);
            } else {
                const Box gb{gx, gy, 0.5 * pc.isosLen, 0.5 * pc.isosWid};
                Corners<G, 8> gc;
                gc.eval(m.g, g, gb, gb, gb, gb, 0x0u);
                gs = submap_from_corners(m.g, gc.template bbox<0>(g), gc.box_within(0), gx, gy);
            }
        }
        if (live && leg == 0 && g.sub == 0)
            out.pose_status[b] = (centre_usable(gx, gy) && gs.ok) ? 0 : static_cast<uint8_t>(FPE_POSE_OPT_SUBMAP_FAILED);
    }

    const int nPhases = (!kPlain && gait == 1) ? 4 : 1;
    const double advance = (!kPlain && gait == 1) ? (kStride ? sv.stepQuarter : pc.stepQuarter) : (kStride ? sv.step : pc.step);
    const int walkOrder = walk_order(pc);
    const unsigned long long poseMask = pose_lane_mask<kPoseThreads>(slot);  // the validation ballot's: the lanes of this lane's pose
    // the track whose feet-polygon centre this lane evaluates: 3x3-only kernels: the track of the lane's corner
    // (LaneRole); generic kernels: lane t evaluates track t
    const int myTrack = kMid ? lane_track(g.sub) : (g.sub < 2 ? g.sub : 2);
    LaneRole role{};
    if constexpr (kMid) role = make_lane_role(g.sub, pc.rf, ls.lk.lx, pc.cornerEps, static_cast<double>(mArg.g.rows));
    FastRanks fr{};
    if constexpr (kMid) fr = load_fast_ranks<NRL>(lut, g, pc.winH);
    const bool wantDefault = out.default_next != nullptr;  // (3x3-only kernels: the one product test of the fast leg search)
    uint32_t okBits = 0u;  // cycleOk of the cycles since the last flush (3x3-only kernels: stored by flush_unit)

    // Issue priority, 3x3-only kernels (two wavefronts per SIMD at the headline's batch): the SIMD's arbiter serves the OLDER of
    // its two wavefronts first, so the older one finishes a sixth ahead (49 k against 59 k clocks, profiles/round3_residency.txt)
    // and the younger one runs its tail alone at half the issue rate.  Three eighths into the chain the younger wavefront (odd
    // hardware wave slot = launched second) raises its priority: the lead the older one built is what the younger one builds
    // from there on, and the two finish together.  Measured (round 4, 50-step A/B, six repetitions): headline 26.8 -> 25.5 us,
    // cfg-2 27.2 -> 26.0 us; switching at 2/8: the same, at 4/8: 25.9, at 1/8: 26.0, from the start (the plain reversal round 3
    // tried): 26.7 = no change; handing the priority back near the end or alternating every one / two cycles: 26.1 - 26.3.
    unsigned hwSlot = 0u;
    if constexpr (kMid) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwSlot));
        hwSlot &= 15u;
    }
    constexpr int kPrioSwapEighths = 3;
    if constexpr (kMid) {
        // 3x3-only kernels: a loop nest by batch of eight cycles — the y fill, the batch's cycles, the flush.  What happens once per
        // batch is placed by the outer loop, not tested in every cycle (in the flat form below: three scalar compares and branches a
        // cycle, the fill's block inside the cycle loop, and the entry / unit / okBits positions re-formed from cyc & 7), and the
        // inner loop walks the y entries and the units by pointer.  Every store, LDS write and bits_sync in the flat form's order.
        const int prioCyc = (hwSlot & 1u) ? (nCycles * kPrioSwapEighths) / 8 : -1;  // the cycle of the hand-over (none: -1)
        for (int c0 = 0; c0 < nCycles; c0 += kBatch) {
            {
                // y side of the batch's cycles: lane (leg, s) fills the entry of cycle c0 + s.  ajustedPose_[1] is the
                // reference's running sum (cpp:1578): cycle c0 + s has seen s more additions of the drift
                double a = adjY, mine = adjY;
#pragma unroll
                for (int k = 1; k < kBatch; ++k) {
                    a += hc.drift;
                    if (g.sub == k) mine = a;
                }
                const YFillConsts yc{hc.rf, hc.cornerEps, pc.winH};  // (its constants from the vector registers they are parked in)
                fill_yentry(m.g, yc, ls, (y0 + mine) + ls.biasY, ytab[g.sub]);  // cpp:2201, 2414
                bits_sync<G>();
            }
            const int nb = min(kBatch, nCycles - c0);  // (the last batch may be short)
            const YEntry* yeP = ytab;
            UnitT* unit = units;
            for (int s = 0; s < nb; ++s, ++yeP, ++unit) {
                const int cyc = c0 + s;
                if (FPE_RARE(cyc == prioCyc)) __builtin_amdgcn_s_setprio(2);
                const YEntry& ye = *yeP;
                bool cycleOk = true;
                for (int ph = 0; ph < nPhases; ++ph) {  // (the phases: see the flat form below)
                    const unsigned mask = (!kPlain && gait == 1) ? (1u << ((walkOrder >> (2 * ph)) & 3)) : 0xFu;
                    const bool active = kPlain || ((mask >> leg) & 1u) != 0u;  // (plain: every leg swings in the one phase)
                    double myCtr = stanceCtr;
                    if (!FPE_RARE(kStanceOnce && cyc == 0 && ph == 0)) myCtr = polygon_center_x<true>(sh.cur[myTrack]);  // (wave-uniform branch)
                    LegCommit lc;
                    lc.valid = 1;  // non-swing legs do not vote
                    if (active)
                        leg_fast8m<NRL, kNoDefault, kProd, kPlain>(m, bm, pc.winH, wantDefault, hc, role, fr, head, sh, lb, g, leg, ls, ye, myCtr, advance, cyc,
                                                                   &lc, unit);
                    const bool phaseOk = (__ballot(lc.valid == 0) & poseMask) == 0ull;
                    if (phaseOk && active && g.sub == 0) {
#pragma unroll
                        for (int t = 0; t < 3; ++t) {
                            sh.cur[t][leg][0] = lc.v[t][0];
                            sh.cur[t][leg][1] = lc.v[t][1];
                        }
                    }
                    bits_sync<G>();
                    cycleOk = cycleOk && phaseOk;
                }
                adjY += hc.drift;  // cpp:1578
                okBits |= (cycleOk ? 1u : 0u) << s;  // (bit cyc & 7, as flush_unit reads it)
            }
            {
                // heights, output records and cycle validity of the batch's cycles: lane (leg, s) takes the unit of cycle c0 + s
                // (once per eight cycles: h and the product pointers from the argument segment, see MidKernArgs)
                const MidKernArgs* ka = mid_cold_args();
                const double hF = ka->pc.h;
                const fpe_plan_out outF = specialise_products<kProd>(ka->out);
                if (live && g.sub < nb) flush_unit(m, hF, units[g.sub], ytab[g.sub], b, c0 + g.sub, leg, nCycles, okBits, outF);
                okBits = 0u;
                bits_sync<G>();  // the units and the y entries are rewritten next
            }
        }
    } else {
        // generic kernels: the flat loop over the cycles (as a nest these kernels, at their cap of 168 vector registers, spill more:
        // <3, false, 2> 12 -> 28 bytes of scratch, <4, false, 2> 48 -> 56, the stride form <3> 8 -> 28)
        for (int cyc = 0; cyc < nCycles; ++cyc) {
            if ((cyc & (kBatch - 1)) == 0) {
                // y side of the next kBatch cycles: lane (leg, s) fills the entry of cycle cyc + s.  ajustedPose_[1] is the
                // reference's running sum (cpp:1578): cycle cyc + s has seen s more additions of the drift
                double a = adjY, mine = adjY;
#pragma unroll
                for (int k = 1; k < kBatch; ++k) {
                    a += hc.drift;
                    if (g.sub == k) mine = a;
                }
                if (g.sub < kBatch) fill_yentry(m.g, pc, ls, (y0 + mine) + ls.biasY, ytab[g.sub]);  // cpp:2201, 2414
                bits_sync<G>();
            }
            const YEntry& ye = ytab[cyc & (kBatch - 1)];
            bool cycleOk = true;
            for (int ph = 0; ph < nPhases; ++ph) {
                const unsigned mask = (!kPlain && gait == 1) ? (1u << ((walkOrder >> (2 * ph)) & 3)) : 0xFu;
                const bool active = kPlain || ((mask >> leg) & 1u) != 0u;  // (plain: every leg swings in the one phase)
                // feet-polygon centres (getPolygonCenter, cpp:2191, 2265): every lane computes ONE track's centre from the
                // committed feet in LDS; the values reach the group's other lanes by swizzle (no LDS hand-off, no barrier)
                double myCtr = stanceCtr;
                if (!kStanceOnce || cyc != 0 || ph != 0) myCtr = polygon_center_x(sh.cur[myTrack]);  // (wave-uniform branch)
                // footholdValidation_ (cpp:1323) is a ballot over the pose's lanes; the committed positions go from
                // registers straight to PoseShared::cur (cpp:1332-1576)
                LegCommit lc;
                lc.valid = 1;  // non-swing legs do not vote
                if (active) {
                    constexpr int kKeep = (~(G - 1)) & 0x1F;
                    const double ctr0 = swizzle_f64<kKeep | (0 << 5)>(myCtr), ctr1 = swizzle_f64<kKeep | (1 << 5)>(myCtr),
                                 ctr2 = swizzle_f64<kKeep | (2 << 5)>(myCtr);
                    leg_phase_bits8<NRL, false>(m, bm, pc, lut, head, sh, lb, g, leg, ls, ye, ctr0, ctr1, ctr2, advance, cyc, out, &lc,
                                                units + (cyc & (kBatch - 1)));
                }
                const bool phaseOk = (__ballot(lc.valid == 0) & poseMask) == 0ull;
                if (phaseOk && active && g.sub == 0) {
#pragma unroll
                    for (int t = 0; t < 3; ++t) {  // x and y only: no later cycle reads a committed z (getPolygonCenter, cpp:2421-2463)
                        sh.cur[t][leg][0] = lc.v[t][0];
                        sh.cur[t][leg][1] = lc.v[t][1];
                    }
                }
                bits_sync<G>();
                cycleOk = cycleOk && phaseOk;
            }
            adjY += hc.drift;  // cpp:1578
            okBits |= (cycleOk ? 1u : 0u) << (cyc & 7);
            if ((cyc & (kBatch - 1)) == kBatch - 1 || cyc == nCycles - 1) {
                // heights, output records and cycle validity of the last (up to) kBatch cycles: two lanes per unit (kBatch * 2 == G),
                // lanes (leg, 2 s) and (leg, 2 s + 1) take the unit of cycle base + s
                const int c0 = cyc & ~(kBatch - 1);
                const int us = g.sub >> 1;
                if (live && c0 + us <= cyc)
                    flush_unit_g(m, pc, sh.footDa, sh.footDb, units[us], ytab[us], b, c0 + us, leg, g.sub & 1, nCycles, okBits, out, cycBase);
                okBits = 0u;
                bits_sync<G>();  // the units and the y entries are rewritten next
            }
        }
    }
    if constexpr (kResume) {  // the state behind the last flush (the last phase's commit is behind its bits_sync)
        if (rs.out && live && g.sub == 0) store_leg_state(rs.out, b, leg, sh.cur, adjY, cycBase + nCycles);
    }
}

// The head of every 8-lane kernel: the lane's pose slot and leg, and the loads of its pose.  The pose first: its address needs
// nothing but the preloaded arguments, and everything else waits for it.  The padding pose of the last block runs the chain on pose
// B-1 (with ITS stride and state, in the chain forms) and stores nothing.
struct PoseSlot8 {
    int tid, slot, leg, b;
    bool live;
    const fpe_pose* pp;
    double x0, y0, z0;
    int gait;
    float rOverride;
    int polyKindIn;
};
__device__ __forceinline__ PoseSlot8 load_pose_slot8(const fpe_pose* __restrict__ poses, int B) {
    constexpr int G = 8, kPoseThreads = 4 * G;
    PoseSlot8 p;
    p.tid = static_cast<int>(threadIdx.x);
    p.slot = p.tid / kPoseThreads;
    p.leg = (p.tid / G) & 3;
    p.b = blockIdx.x * 2 + p.slot;
    p.live = p.b < B;
    if (!p.live) p.b = B - 1;
    p.pp = poses + p.b;
    p.x0 = p.pp->position[0], p.y0 = p.pp->position[1], p.z0 = p.pp->position[2];
    p.gait = p.pp->gait;
    p.rOverride = p.pp->leg_search_radius[p.leg];
    p.polyKindIn = p.pp->leg_polygon_kind[p.leg];
    return p;
}
// ... and the constants of the leg search parked in vector registers (HotConsts; the drift is the caller's: the plan's or the pose's)
template <class PC>
__device__ __forceinline__ HotConsts park_hot_consts(const PC& pc) {
    HotConsts hc;
    hc.rf = in_vgpr(pc.rf);
    hc.rf2 = in_vgpr(pc.rf2);
    hc.cornerEps = in_vgpr(pc.cornerEps);
    hc.oneMinusEps = in_vgpr(1.0 - pc.cornerEps);
    return hc;
}

template <int NRL, bool kMid, int kProd>
// (the pose pointer and the counts lead the argument list: scalar arguments at the head of the kernarg segment are
// preloaded into SGPRs at wave launch, -amdgpu-kernarg-preload-count, so the pose loads can be issued at once)
__global__ __launch_bounds__(64, kMid ? 2 : kBitsGenericWaves) void plan_bits_kernel(const fpe_pose* __restrict__ poses, int B, int nCycles,
                                                          DevMap mArg, BitMap bm, typename std::conditional<kMid, PlanMidConsts, PlanConsts>::type pc,
                                                          SpiralLut lut, fpe_plan_out outArg) {
    const fpe_plan_out out = specialise_products<kProd>(outArg);
    const PoseSlot8 p = load_pose_slot8(poses, B);
    __builtin_amdgcn_sched_barrier(0);  // (the loads above stay ahead of the kernel-argument fetches below)
    // the map geometry parked in VGPRs (park_geometry) — in the 3x3-only variants; the generic ones run at their register cap (168
    // VGPRs at three wavefronts per SIMD), where the twenty registers cost more in spills than the scalar operands do in moves
    // (measured: cfg-4 0.713 -> 0.664 ms without)
    DevMap m = mArg;
    if constexpr (kMid) park_geometry(m);
    HotConsts hc = park_hot_consts(pc);
    hc.drift = kMid ? in_vgpr(pc.drift) : pc.drift;  // (the generic variants run at their register cap: nothing extra parked)
    // 3x3-only kernels: one verdict per wavefront.  PLAIN = both pose slots trot, no leg overrides its search radius, every
    // search polygon is the rectangle: the reference planner's only case (one gait, one searchRadius_, getSearchPolygon).  The
    // padding slot of an odd batch runs pose B-1 again and votes as that pose does.  Each verdict has its own copy of the rest
    // of the kernel, inlined (as a callee the chain ran at 33.7 us instead of 24.7); the kernel's name and arguments stay.
    if constexpr (kMid) {
        if (__ballot(p.gait == 1 || p.rOverride > 0.0f || p.polyKindIn != 0) == 0ull) {
            plan_bits_body<NRL, kMid, kProd, true>(p.pp, p.b, p.live, p.x0, p.y0, p.z0, p.gait, p.rOverride, p.polyKindIn, nCycles, m, mArg, bm, pc, lut, out, hc,
                                                   p.tid, p.slot, p.leg);
            return;
        }
    }
    plan_bits_body<NRL, kMid, kProd, false>(p.pp, p.b, p.live, p.x0, p.y0, p.z0, p.gait, p.rOverride, p.polyKindIn, nCycles, m, mArg, bm, pc, lut, out, hc, p.tid,
                                            p.slot, p.leg);
}

static_assert(kernargs_mirror<decltype(plan_bits_kernel<2, true, 2>)>(
                  {offsetof(MidKernArgs, poses), offsetof(MidKernArgs, B), offsetof(MidKernArgs, nCycles), offsetof(MidKernArgs, m),
                   offsetof(MidKernArgs, bm), offsetof(MidKernArgs, pc), offsetof(MidKernArgs, lut), offsetof(MidKernArgs, out)},
                  offsetof(MidKernArgs, out) + sizeof(MidKernArgs::out)),
              "MidKernArgs must mirror the parameters of plan_bits_kernel<NRL, true, kProd>");

// The chain forms of the generic 8-lane kernel: the same body behind plan_bits_kernel's own argument list and a TRAILING pack S, as
// plan_chained_kernel's.  Generic variants only: a chain call on a 3x3-only configuration runs this kernel (the two are pinned
// equivalent under no_mid_variant).
// Stride form (fpe_plan_strides*): S = {const fpe_stride*} — the step and the drift of each pose slot read from strides[b], one
// 16-byte record per pose, loaded next to the pose.
// Resume form (fpe_plan_resume*): S = {const fpe_stride*, const fpe_plan_state*, fpe_plan_state*}, each of which may be null
// (strides: the plan's own step and drift, one uniform branch; state_in: the stance prologue; state_out: nothing returned).  A pose's
// 208-byte state is loaded beside its pose and its stride.
template <int NRL, int kProd, class... S>
__global__ __launch_bounds__(64, kBitsGenericWaves) void plan_bits_chain_kernel(const fpe_pose* __restrict__ poses, int B, int nCycles, DevMap mArg, BitMap bm,
                                                                               PlanConsts pc, SpiralLut lut, fpe_plan_out outArg, S... chainArg) {
    constexpr bool kResume = sizeof...(S) == 3;
    static_assert(sizeof...(S) == 1 || kResume, "trailing arguments: the strides, or the strides and the two states");
    const fpe_plan_out out = specialise_products<kProd>(outArg);
    const PoseSlot8 p = load_pose_slot8(poses, B);
    StrideVals sv;
    if constexpr (kResume) sv = load_stride_or_plan(stride_arg(chainArg...), p.b, pc);
    else sv = load_stride(stride_arg(chainArg...), p.b);
    __builtin_amdgcn_sched_barrier(0);  // (the loads above stay ahead of the kernel-argument fetches below)
    HotConsts hc = park_hot_consts(pc);
    hc.drift = sv.drift;  // per pose slot: the y-table fill and the per-cycle sum add the pose's own drift
    plan_bits_body<NRL, false, kProd, false, true, kResume>(p.pp, p.b, p.live, p.x0, p.y0, p.z0, p.gait, p.rOverride, p.polyKindIn, nCycles, mArg, mArg, bm, pc, lut,
                                                            out, hc, p.tid, p.slot, p.leg, sv, resume_args(chainArg...));
}
