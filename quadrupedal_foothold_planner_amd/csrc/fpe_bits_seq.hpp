// fpe_bits_seq.hpp — the bit-window kernels, third piece (included by fpe_bits.hpp, inside namespace fpe; not stand-alone):
// the ONE-WAVEFRONT-PER-POSE ("seq") family — lane = window row, 64- or 96-bit rows, the swing legs of a phase searched one
// after the other (plan_bits_seq_kernel<NRL, KW, kProd, kGroup>).
#pragma once

namespace {

// One-wavefront-per-pose kernels: what a leg's four output records are made of, staged in LDS by the leg's lane 0 and
// finished for a few cycles at a time by one lane per (cycle, leg): full records side by side instead of eight
// single-lane store instructions per leg — and, since round 3, the MEAN HEIGHTS leave the chain as well.  Nothing a later
// phase reads depends on a height (the feet-polygon centre uses x and y, cpp:2421-2463; records are write-only), so the
// chain only deposits which cells of each CircleIterator bounding box were visited (two 64-bit ballots per disc) and
// where the box lies; flush_seqrec2 reads those elevations itself and runs the reference's ordered f32 sums
// (cpp:2520-2554), up to 32 units side by side instead of one leg at a time (compaction into LDS, three serial sums,
// three divisions per leg-phase: 15-19 % of a leg's clocks on cfg-3 / cfg-5).
struct SeqRecBase {
    double nomX, nomY, cenX, cenY, defX, defY;
    float nomZ, cenZ, defZ;  // final values of the heights that were NOT deferred (see flags)
    int32_t nomRow, nomCol, cenRow, cenCol;
    uint32_t flags;  // nominal valid | source << 8 | centroid code << 16 | kSeqDefer* << 24
};
struct SeqRec : SeqRecBase {
    int32_t aI0, aJ0, aNj;  // centre disc: bounding box origin and width (cells in row-major order t = a * nj + b)
    int32_t bI0, bJ0, bNj;  // default-track disc
    uint32_t pad[2];
    unsigned long long visA[2], visB[2];  // bit t of word t / 64: cell t of the box is a member inside the map
};
static_assert(sizeof(SeqRecBase) == 80 && sizeof(SeqRec) == 144 && sizeof(SeqRec) % 16 == 0, "SeqRec layout");
constexpr uint32_t kSeqDeferA = 1u << 24;  // zA = mean height of the centre disc, to be computed by flush_seqrec2
constexpr uint32_t kSeqDeferB = 1u << 25;  // zB (default track)
constexpr uint32_t kSeqDeferC = 1u << 26;  // zC = mean height of the cell-centred disc of (cenRow, cenCol) (offset table)
constexpr uint32_t kSeqCIsA = 1u << 27;    // zC = zA (whole region valid: the height at the centre, cpp:1687)

// One swing leg of one phase on the bit window: the three tracks' next positions, the centroid method
// (cpp:1605-1997) and checkFoothold (cpp:2001-2036) around the centroid track's position, the mean heights.
// The legs of a phase are searched in sequence: the leg's record is staged in recs[leg] (the commit reads the next
// positions from the record itself, flush_seqrec2 writes the records of a few cycles at a time) and its validity goes
// to validOut (the flag is uniform, the vote stays in registers).
// `recs` is never null — seq_run_pose always stages — but it is an address inside the workgroup's LDS, of which the
// compiler cannot know that: the two tests of it below, the staging into PoseShared::nxt and the direct stores behind
// them are run-time branches IN the four seq_run_pose instantiations today (73 to 181 lines of each one's assembly,
// never executed).  They stay as they are because this function was cut down from the shared leg search under the
// condition that no kernel's instructions change; taking them out is a change of those kernels, to be measured as one.
template <int NRL, int KW>
__device__ __forceinline__ void seq_leg_phase(const DevMap& m, const BitMap& bm, const PlanConsts& pc, const SpiralLut& lut,
                                              const LutHead& head, PoseShared& sh, const LegBits& lb, const Grp<64>& g, int leg,
                                              const LegStatic& ls, double y0, double adjY, double advance, int cyc, int nCycles,
                                              int b, const fpe_plan_out& out, SeqRec* recs, int& validOut) {
    constexpr int G = 64;
    const float Rf = ls.Rf;
    const int polyKind = ls.polyKind;
    const LegConst& lk = ls.lk;
    const double biasX = ls.biasX, biasY = ls.biasY;
    // next default positions of this leg on the three tracks (cpp:2199-2213, 2270-2284)
    const double Ny = y0 + adjY;                         // cpp:2201
    const double nx0 = (sh.ctr[0] + advance) + biasX;  // cpp:2199, 2414
    const double nx1 = (sh.ctr[1] + advance) + biasX;
    const double nx2 = (sh.ctr[2] + advance) + biasX;
    const double ny = Ny + biasY;                        // identical on the three tracks
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
    if (polyKind != 0) bits_sync<G>();  // the vertices are read by the other lanes of the wavefront
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
    // the mean heights are deferred to flush_seqrec2 (SeqRec)
    uint32_t deferFlags = 0u;
    unsigned long long visA0 = 0ull, visA1 = 0ull, visB0 = 0ull, visB1 = 0ull;
    int aI0 = 0, aJ0 = 0, aNj = 1, bI0 = 0, bJ0 = 0, bNj = 1;
    if (!ls.radiusOk || !centre_usable(c.cx, c.cy)) {
        nominal_invalid(no, c.cx, c.cy, ls.radiusOk ? 2 : 3);
        co.x = co.y = 0.0; co.z = 0.0f; co.row = co.col = -1; co.code = 6;
        if (wantDefault && centre_usable(nx0, ny)) {  // cpp:2289-2301 (leg search skipped: radius / centre unusable)
            const BBox dbox = circle_bbox_fast(m.g, nx0, ny, pc.rf);
            bool unused;
            zDefault = disc_pass_direct<G, false>(m, pc, nx0, ny, dbox, g, unused, scratch);
        }
    } else {
        // corner lanes: box 0 = centre foot disc, box 1 = centroid rectangle, box 2 = default-track disc,
        // box 3 = getIndex(centre)
        const Box b0{c.cx, c.cy, pc.rf, pc.rf}, b1{c.cx, c.cy, 0.5 * lk.lx, 0.5 * lk.ly};
        const Box b2{nx0, ny, pc.rf, pc.rf};
        Corners<G, 16> cs;
        cs.eval(m.g, g, b0, b1, b2, b0, 0x8u);
        const BBox bb = cs.template bbox<0>(g);
        const BBox rbox = cs.template bbox<1>(g);
        const BBox dbox = cs.template bbox<2>(g);
        c.ici = cs.template get<12>(g);
        c.icj = cs.template get<13>(g);
        const Submap sm = submap_from_corners(m.g, rbox, cs.box_within(1), c.cx, c.cy);
        const int iw0 = c.ici - pc.winH, jw0 = c.icj - pc.winH;
        // one memory round trip: the window's bit rows and the elevation of the two discs around known centres
        uint4 grp[NRL][KW + 1];
        win_issue<G, NRL, KW>(bm, m.g, g, iw0, jw0, grp);
        DiscLoads dc, dd;
        disc_issue<G, false, false, false>(m, pc, c.cx, c.cy, bb, g, dc);
        const bool dfltUsable = wantDefault && centre_usable(nx0, ny);
        if (dfltUsable) disc_issue<G, false, false, false>(m, pc, nx0, ny, dbox, g, dd);
        WinRows<NRL, KW> w;
        win_finish<NRL, KW>(jw0, grp, w);
#pragma unroll
        for (int k = 0; k < NRL; ++k)
#pragma unroll
            for (int q = 0; q < KW; ++q)
                if (g.sub + G * k < lb.rows) lb.a[(g.sub + G * k) * KW + q] = w.Df[k][q];
        const CentroidScan sc = rows_from_bits<G, NRL, KW>(sm, w, g, iw0, jw0);
        bits_sync<G>();
        const bool defaultOk = default_ok_bits<G, KW, false>(m, pc, c.cx, c.cy, bb, dc, lb.a, lb.rows, iw0, jw0, g);  // cpp:2012
        bits_sync<G>();  // lb doubles as scratch below
        bool unused;
        float zCentre = 0.0f;
        // membership of the two discs around known centres as ballots over the bounding boxes' cells (t = round * 64 +
        // lane, row-major: CircleIterator order); a box beyond the two rounds (never with bits_supported's bound on
        // the foot radius) is walked here
        if (dc.pipelined) {
            visA0 = g.ballot(dc.vis[0] != 0);
            visA1 = g.ballot(dc.vis[1] != 0);
            aI0 = bb.i0; aJ0 = bb.j0; aNj = max(bb.nj, 1);
            deferFlags |= kSeqDeferA;
        } else {
            zCentre = disc_pass_direct<G, false>(m, pc, c.cx, c.cy, bb, g, unused, scratch);
        }
        if (dfltUsable) {
            if (dd.pipelined) {
                visB0 = g.ballot(dd.vis[0] != 0);
                visB1 = g.ballot(dd.vis[1] != 0);
                bI0 = dbox.i0; bJ0 = dbox.j0; bNj = max(dbox.nj, 1);
                deferFlags |= kSeqDeferB;
            } else {
                zDefault = disc_pass_direct<G, false>(m, pc, nx0, ny, dbox, g, unused, scratch);
            }
        }
        CentroidPendingBits cp;
        centroid_begin_bits<false>(m, c, sm, sc, zCentre, cp);                                                // cpp:818-821
        if (defaultOk) {
            no.valid = 1;
            no.source = 0;
            no.row = c.ici;
            no.col = c.icj;
            no.x = c.cx;  // cpp:2016-2017
            no.y = c.cy;
        } else {
            nominal_invalid(no, c.cx, c.cy, 2);
            int wi = 0, wj = 0;
            bits_sync<G>();
            const bool spFound = spiral_bits<G, NRL, KW>(m, pc, lut, head, c, w, lb, g, iw0, jw0, wi, wj);
            if (spFound) {  // cpp:2022
                no.valid = 1;
                no.source = 1;
                no.row = wi;
                no.col = wj;
                no.x = cell_pos(m.g.baseX, m.g.res, wi);  // cpp:2105-2107
                no.y = cell_pos(m.g.baseY, m.g.res, wj);
            }
            bits_sync<G>();
        }
        if (cp.needDisc != 0) deferFlags |= kSeqDeferC;          // the result's own cell-centred disc (offset table)
        else if (cp.o.code == 0) {                               // whole region valid: the height at the centre (cpp:1687)
            if (deferFlags & kSeqDeferA) deferFlags |= kSeqCIsA;
            else cp.o.z = zCentre;
        }
        if (no.valid) no.z = zCentre;  // z at the DEFAULT centre, for a spiral candidate too (cpp:2029)
        co = cp.o;
    }
    validOut = no.valid;
    if (g.sub == 0) {
        if (!recs) {  // (never: see above; with staged records the commit reads the next positions from the record itself)
            sh.nxt[0][leg][0] = nx0;   sh.nxt[0][leg][1] = ny;    sh.nxt[0][leg][2] = static_cast<double>(zDefault);
            sh.nxt[1][leg][0] = co.x;  sh.nxt[1][leg][1] = co.y;  sh.nxt[1][leg][2] = static_cast<double>(co.z);
            sh.nxt[2][leg][0] = no.x;  sh.nxt[2][leg][1] = no.y;  sh.nxt[2][leg][2] = static_cast<double>(no.z);
        }
        if (recs) {  // staged: flush_seqrec2 writes the records of a few cycles at a time
            SeqRec r;
            r.nomX = no.x; r.nomY = no.y; r.cenX = co.x; r.cenY = co.y; r.defX = nx0; r.defY = ny;
            r.nomZ = no.z; r.cenZ = co.z; r.defZ = zDefault;
            r.nomRow = no.row; r.nomCol = no.col; r.cenRow = co.row; r.cenCol = co.col;
            r.flags = static_cast<uint32_t>(no.valid) | (static_cast<uint32_t>(no.source) << 8) | (static_cast<uint32_t>(co.code) << 16) | deferFlags;
            r.aI0 = aI0; r.aJ0 = aJ0; r.aNj = aNj;
            r.bI0 = bI0; r.bJ0 = bJ0; r.bNj = bNj;
            r.pad[0] = r.pad[1] = 0u;
            r.visA[0] = visA0; r.visA[1] = visA1;
            r.visB[0] = visB0; r.visB[1] = visB1;
            recs[leg] = r;
        } else {  // (never: see above)
            const size_t o = (static_cast<size_t>(b) * nCycles + cyc) * 4 + leg;
            if (out.nominal) store_foothold(out.nominal + o, no, leg, cyc);
            store_selected<false>(out, o, no.row, no.col, no.z, no.valid, no.source, leg, cyc);
            if (out.centroid) {
                fpe_centroid_foothold cf;
                cf.x = co.x; cf.y = co.y; cf.z = co.z; cf.row = co.row; cf.col = co.col;
                cf.code = static_cast<uint8_t>(co.code); cf.pad[0] = cf.pad[1] = cf.pad[2] = 0;
                store_record<false>(out.centroid + o, cf);
            }
            if (out.default_next) {
                store_record<false>(out.default_next + o * 3 + 0, static_cast<double>(nx0));
                store_record<false>(out.default_next + o * 3 + 1, static_cast<double>(ny));
                store_record<false>(out.default_next + o * 3 + 2, static_cast<double>(zDefault));
            }
        }
    }
}

// The staged records of one (cycle, leg) unit, two lanes per unit: lane half 0 takes the centre disc and the
// centroid result's disc and writes the nominal / selected / centroid records, half 1 the default-track disc and the
// default_next record.  One instruction stream for both halves (the arguments differ per lane, not the code).
__device__ __forceinline__ void flush_seqrec2(const DevMap& m, const PlanConsts& pc, const int8_t* footDa, const int8_t* footDb, const SeqRec& rLds,
                                              int b, int cyc, int leg, int half, int nCycles, const fpe_plan_out& out, int cycBase = 0) {
    // cycBase (the resume form: fpe_plan_state.cycle): added to the records' gait_cycle_id; the index stays the call's own `cyc`
    SeqRec r;
    __builtin_memcpy(&r, &rLds, sizeof(SeqRec));
    const size_t o = (static_cast<size_t>(b) * nCycles + cyc) * 4 + leg;
    const bool h1 = half != 0;
    const bool defer = (r.flags & (h1 ? kSeqDeferB : kSeqDeferA)) != 0u && (h1 ? out.default_next != nullptr : true);
    const bool wantC = !h1 && (r.flags & kSeqDeferC) != 0u && out.centroid != nullptr;
    float sBox, sC;
    constexpr int kBoxCellsPerBatch = 12;  // measured: 8 -> 12: cfg-3 -1.3 %, cfg-5 -1.5 %; 13, 14 the same; 16 worse on cfg-3
    seq_mean2<kBoxCellsPerBatch, 8>(m.elev, m.g.rows, m.g.cols, h1 ? r.bI0 : r.aI0, h1 ? r.bJ0 : r.aJ0, max(h1 ? r.bNj : r.aNj, 1), defer ? (h1 ? r.visB[0] : r.visA[0]) : 0ull,
              defer ? (h1 ? r.visB[1] : r.visA[1]) : 0ull, wantC, r.cenRow, r.cenCol, footDa, footDb, pc.nFoot, pc.h, sBox, sC);
    if (h1) {
        if (out.default_next) {
            store_record<true>(out.default_next + o * 3 + 0, r.defX);
            store_record<true>(out.default_next + o * 3 + 1, r.defY);
            store_record<true>(out.default_next + o * 3 + 2, static_cast<double>(defer ? sBox : r.defZ));
        }
        return;
    }
    const uint8_t valid = static_cast<uint8_t>(r.flags & 0xFFu), source = static_cast<uint8_t>((r.flags >> 8) & 0xFFu);
    const float zA = defer ? sBox : r.nomZ;
    const float zC = wantC ? sC : ((r.flags & kSeqCIsA) ? zA : r.cenZ);
    const float zN = defer ? (valid ? zA : 0.0f) : r.nomZ;  // z at the DEFAULT centre, for a spiral candidate too (cpp:2029)
    if (out.nominal) {
        fpe_foothold f;
        f.row = r.nomRow; f.col = r.nomCol; f.x = r.nomX; f.y = r.nomY; f.z = zN;
        f.valid = valid; f.source = source;
        f.foot_id = static_cast<uint8_t>(leg); f.gait_cycle_id = static_cast<uint8_t>(cycBase + cyc);
        store_record<true>(out.nominal + o, f);
    }
    store_selected<true>(out, o, r.nomRow, r.nomCol, zN, valid, source, leg, cycBase + cyc);
    if (out.centroid) {
        fpe_centroid_foothold cf;
        cf.x = r.cenX; cf.y = r.cenY; cf.z = zC; cf.row = r.cenRow; cf.col = r.cenCol;
        cf.code = static_cast<uint8_t>((r.flags >> 16) & 0xFFu); cf.pad[0] = cf.pad[1] = cf.pad[2] = 0;
        store_record<true>(out.centroid + o, cf);
    }
}

}  // namespace

// ---- chained plan on the bit window, sequential-legs form (large windows): one wavefront per pose, lane = window
// row, KW words per row; the swing legs of a phase are searched one after the other (see plan_sequential_kernel) ----
constexpr int kSeqWaves = 4;  // wavefronts per SIMD the register allocation aims at
// The kernel's argument list as a struct: HIP lays a kernel's arguments out one after the other, each at its natural alignment —
// a C struct of the same members in the same order — so this is a VIEW of plan_bits_seq_kernel's argument segment, through which a
// leg search can read its constants again (kSeqReloadArgs, below) instead of keeping them in scalar registers across the
// whole chain.  (The kernel keeps its separate arguments: taking this struct as its one argument cost <1, 2> 0.6 %.)  A static_assert
// behind the kernel checks the mirror against its signature.
struct SeqKernArgs {
    DevMap m;
    BitMap bm;
    PlanConsts pc;
    SpiralLut lut;
    const fpe_pose* poses;
    int B, nCycles;
    fpe_plan_out out;
    int recSlots;
    int slotBytes;
    const fpe_stride* strides;  // the one trailing argument of the kernel's stride form (not in the segment otherwise: never read there)
    const fpe_plan_state* stateIn;  // ... and, behind it, the two more of its resume form (likewise)
    fpe_plan_state* stateOut;
};
// The argument reload pays on the 96-bit-row instantiations only — measured, round 6, A/B in one call, twice:
// cfg-5 (<2, 3>) 0.3060 -> 0.3017 ms and its 32 B of vector scratch gone; cfg-3 (<1, 2>) 0.6075 -> 0.6211 ms although three quarters of
// its leg search's spill reads disappear with it (see the leg loop): the lane reads were never what bound that kernel.
template <int KW>
constexpr bool kSeqReloadArgs = KW >= 3;
// One pose's chain, from its stance to its last gait cycle: a FUNCTION the kernel calls once per wavefront, not inlined.  Round 6:
// as a callee the body reads everything uniform from the kernel's ARGUMENT SEGMENT (scalar loads through `kaIn`) instead of holding the
// arguments in scalar registers the allocator spills to vector lanes (no spilled scalars in the kernel, 60-150 before: cfg-3 0.6046 ->
// 0.5959 ms), and the kernel can put SIXTEEN poses in one workgroup (one workgroup per CU instead of sixteen: cfg-5 0.3023 -> 0.2959 ms;
// plan_bits_seq_kernel below).  A/B in one call, three repetitions: profiles/round6_seq_floor.txt.
// kStride (the kernel's stride form): the step and the drift are the pose's own, scalar loads of strides[b] through the argument
// segment's trailing pointer.  kResume (the kernel's resume form, a stride form too): a null `strides` means the plan's own pair, and
// the chain's state comes from stateIn (null: the stance prologue) and goes to stateOut (null: nowhere) — fpe_plan_resume*.
template <int NRL, int KW, int kProd, bool kStride = false, bool kResume = false>
__device__ __attribute__((noinline)) void seq_run_pose(const SeqKernArgs __attribute__((address_space(4))) * kaIn, int slotOffIn, int bInV, int tid, unsigned hwidIn,
                                                       const LutHead& head) {
    constexpr int G = 64;
    constexpr int NR = G * NRL;
    // (a function's arguments arrive in VECTOR registers: the uniform ones go back to scalars here, or every address and index derived
    // from them would be vector arithmetic — and the argument-segment pointer could not feed scalar loads at all)
    typedef const SeqKernArgs __attribute__((address_space(4))) * KernArgPtrS;
    const unsigned long long kaBits = reinterpret_cast<unsigned long long>(kaIn);
    const KernArgPtrS kaArg = reinterpret_cast<KernArgPtrS>((static_cast<unsigned long long>(static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(kaBits >> 32)))) << 32) |
                                                              static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(kaBits))));
    const int slotOff = __builtin_amdgcn_readfirstlane(slotOffIn), b = __builtin_amdgcn_readfirstlane(bInV);
    const unsigned hwid = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(hwidIn)));
    const SeqKernArgs* kaG = (const SeqKernArgs*)kaArg;
    const DevMap& m = kaG->m;
    const BitMap& bm = kaG->bm;
    const PlanConsts& pc = kaG->pc;
    const SpiralLut& lut = kaG->lut;
    const fpe_pose* __restrict__ poses = kaG->poses;
    const int nCycles = kaG->nCycles, recSlots = kaG->recSlots;
    const fpe_plan_out out = specialise_products<kProd>(kaG->out);
    // (the workgroup's LDS by its own symbol: a pointer PARAMETER would be a generic one, and every LDS access a flat instruction)
    extern __shared__ __attribute__((aligned(16))) unsigned char smemAll[];
    unsigned char* const smem = smemAll + slotOff;
    const Grp<G> g(tid);
    PoseShared& sh = *reinterpret_cast<PoseShared*>(smem);
    // per-leg constants of the pose, computed once (lane = leg) instead of once per leg and phase: a division and a
    // dependent rank-table load each
    LegStatic* lsTab = reinterpret_cast<LegStatic*>(smem + sizeof(PoseShared));
    constexpr size_t kLsBytes = (4 * sizeof(LegStatic) + 15) & ~static_cast<size_t>(15);
    // rows actually allocated: the window's 2 winH + 1 (not 64 * NRL) — LDS bounds the occupancy of these kernels
    const LegBits lb = make_legbits(smem + sizeof(PoseShared) + kLsBytes, min(2 * pc.winH + 1, NR), KW);
    // staged output records: recSlots (a power of two, sized by the launch to keep the LDS within the occupancy budget)
    // cycles of four legs behind the row arrays
    using Rec = SeqRec;
    Rec* recBase = reinterpret_cast<Rec*>(
        smem + ((sizeof(PoseShared) + kLsBytes + 4 * static_cast<size_t>(legbits_words(min(2 * pc.winH + 1, NR), KW, pc.nHW)) + 15) & ~static_cast<size_t>(15)));

    const fpe_pose* pp = poses + b;
    const double x0 = pp->position[0], y0 = pp->position[1], z0 = pp->position[2];
    const int gait = pp->gait;
    static_assert(!kResume || kStride, "a resume instance is a stride instance");
    StrideVals sv{};
    if constexpr (kResume) sv = load_stride_or_plan(kaG->strides, b, pc);
    else if constexpr (kStride) sv = load_stride(kaG->strides, b);
    // lane = leg: lanes 0-3 write, every lane loads the state of leg tid & 3 (the finite verdict is a ballot over the wavefront)
    double adjY = 0.0;  // ajustedPose_[1], cpp:759
    int cycBase = 0;    // gait_cycle_id of the call's first cycle
    bool started = true;
    if constexpr (kResume) {
        const fpe_plan_state* stateIn = kaG->stateIn;
        if (stateIn) {  // (uniform) the state of an earlier call instead of the stance
            started = false;
            // chain_resume's text with lane = leg, kept here (through the helper the resume forms ran outside the parent's band)
            const LegState st = load_leg_state(stateIn, b, tid & 3);  // (every lane loads: the verdict is a ballot)
            const bool poseFinite = __ballot(!st.finite) == 0ull;
            adjY = st.adjY;
            cycBase = __builtin_amdgcn_readfirstlane(st.cycle);
            if (tid < 4) {
                lsTab[tid] = make_leg_static(pc, pp, tid, m.g.res, lut);
                for (int t = 0; t < 3; ++t) {
                    sh.cur[t][tid][0] = poseFinite ? st.x[t] : __builtin_nan("");
                    sh.cur[t][tid][1] = st.y[t];
                    sh.cur[t][tid][2] = 0.0;
                }
            }
        }
    }
    for (int k = tid; k < pc.nFoot; k += G) {
        sh.footDa[k] = pc.footDa[k];
        sh.footDb[k] = pc.footDb[k];
        sh.footOff[k] = 0;
    }
    // initial stance and first-gait shift, lane = leg: chain_stance's text, kept here (through the helper the benchmarked plain
    // instantiations compile to other instructions: the body reads its constants through the argument segment)
    if (started && tid < 4) {
        const int leg = tid;
        lsTab[leg] = make_leg_static(pc, pp, leg, m.g.res, lut);
        double sx = (leg == 0 || leg == 3) ? pc.LbHalf : -pc.LbHalf;
        double sy = (leg <= 1) ? pc.WbHalfNeg : pc.WbHalfPos;
        double sz = 0;
        sx += x0;
        sy += y0;
        sz += z0;
        if (out.stance) {
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
    pose_sync<16>();
    if (started && out.pose_status && tid == 0) out.pose_status[b] = opt_gate_cycle0<kStride>(m.g, pc, polygon_center_x(sh.cur[0]), y0, sv);

    const int nPhases = (gait == 1) ? 4 : 1;
    const double advance = (gait == 1) ? (kStride ? sv.stepQuarter : pc.stepQuarter) : (kStride ? sv.step : pc.step);
    const int walkOrder = walk_order(pc);

    const int cycLag = (static_cast<int>(hwid & 3u) * nCycles) / 16;  // launch order of this wavefront on its SIMD (HW_ID.WAVE_ID: 0 oldest .. 3) x a sixteenth of the cycles
    for (int cyc = 0; cyc < nCycles; ++cyc) {
        {
            // Issue priority by PROGRESS (s_setprio, four levels): the SIMD's arbiter serves the oldest wavefront first, so the
            // four poses of a SIMD finish one after the other and the last one runs alone at a third of the four-wavefront issue
            // rate (profiles/round3_residency.txt: lifetimes 1.2 / 1.4 / 1.6 / 1.9 M clocks by launch order).  A wavefront that
            // is behind gets the higher priority: the four advance together and finish together.  Measured: cfg-3 0.727 -> 0.640 ms,
            // cfg-5 0.375 -> 0.325 ms; the reverse mapping reproduces the default.  (The 8-lane kernels: headline neutral — its two
            // wavefronts per SIMD start and advance together anyway —, cfg-4 +3 %: new workgroups would starve the ones about to
            // finish; not used there.)
            // The levels change where a half, a quarter and an eighth of the cycles remain: wavefronts re-synchronise at every
            // boundary (the one ahead waits at the lower level), and the free run after the last boundary — oldest first again —
            // is the last eighth only.  Measured against four equal quarters: cfg-3 0.644 -> 0.625 ms, cfg-5 0.328 -> 0.325 ms;
            // boundaries per leg search instead of per cycle, later boundaries (1/4, 1/8, 1/16) and a rotating offset that
            // emulates sixteen levels were all slower.
            // (the younger wavefronts of the SIMD keep their level a little longer — cycLag, from the hardware wave slot = launch
            // order, see above the loop: within a level the arbiter serves the oldest first.  cfg-3 0.623 -> 0.608 ms, cfg-5 the
            // same; lags of 1 / 32, 3 / 32 and 4 / 32 of the cycles per slot: less or nothing)
            const int cycEff = max(cyc - cycLag, 0);
            const int rem8 = ((nCycles - cycEff) * 8 + nCycles - 1) / nCycles;  // remaining cycles in eighths, rounded up: 8 .. 1
            const int q = rem8 > 4 ? 0 : (rem8 > 2 ? 1 : (rem8 > 1 ? 2 : 3));
            if (q == 0) __builtin_amdgcn_s_setprio(3);
            else if (q == 1) __builtin_amdgcn_s_setprio(2);
            else if (q == 2) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        bool cycleOk = true;
        for (int ph = 0; ph < nPhases; ++ph) {
            const unsigned mask = (gait == 1) ? (1u << ((walkOrder >> (2 * ph)) & 3)) : 0xFu;
            // feet-polygon centres: lane t computes track t (getPolygonCenter, cpp:2191, 2265)
            if (tid < 3) sh.ctr[tid] = polygon_center_x(sh.cur[tid]);
            pose_sync<16>();
            int allValid = 1;  // non-swing legs do not vote
            for (int leg = 0; leg < 4; ++leg) {
                if (!((mask >> leg) & 1u)) continue;
                const LegStatic ls = lsTab[leg];
                int legValid = 1;
                constexpr bool kReload = kSeqReloadArgs<KW>;
                if constexpr (kReload) {
                // Round 6: the leg search reads the map's geometry, the plan constants, the table and output pointers from the
                // ARGUMENT SEGMENT again (scalar loads through a pointer the optimiser cannot see through: nothing is hoisted out
                // of the chain) instead of holding ~130 scalar registers of them across 128 leg searches.  The register allocator
                // had spilled those to lanes of three vector registers in the prologue and read them back with v_readlane inside
                // the leg search — 226 static lane reads of its 1 197 vector instructions in <1, 2, 0>, 276 of 1 529 in <2, 3, 0>
                // (profiles/round6_seq_floor.txt) — in kernels whose VECTOR unit is what is busy (0.86 of the SIMD's time at four
                // wavefronts).  With the reload 53 / 57 remain, the kernels hold 67 / 69 spilled scalars instead of 142 / 152 and
                // <2, 3, 0> no vector scratch — and the time says what those reads were worth: cfg-5 -1.3 %, cfg-3 +2 % (the scalar
                // loads' waits now sit INSIDE the leg search, in front of its first uses); hence the per-instantiation switch above.
                typedef const SeqKernArgs __attribute__((address_space(4))) * KernArgPtr;
                KernArgPtr ka4 = (KernArgPtr)kaArg;
                asm volatile("" : "+s"(ka4));
                const SeqKernArgs* ka = (const SeqKernArgs*)ka4;
                const fpe_plan_out outL = specialise_products<kProd>(ka->out);
                // (the LDS carve-up likewise: a few scalar operations on two of the constants instead of six held registers)
                const int rowsL = min(2 * ka->pc.winH + 1, NR);
                const LegBits lbL = make_legbits(smem + sizeof(PoseShared) + kLsBytes, rowsL, KW);
                Rec* const recL = reinterpret_cast<Rec*>(
                    smem + ((sizeof(PoseShared) + kLsBytes + 4 * static_cast<size_t>(legbits_words(rowsL, KW, ka->pc.nHW)) + 15) & ~static_cast<size_t>(15)));
                seq_leg_phase<NRL, KW>(ka->m, ka->bm, ka->pc, ka->lut, head, sh, lbL, g, leg, ls, y0, adjY, advance, cyc, ka->nCycles, b, outL,
                                       recL + 4 * (cyc & (ka->recSlots - 1)), legValid);
                } else {
                seq_leg_phase<NRL, KW>(m, bm, pc, lut, head, sh, lb, g, leg, ls, y0, adjY, advance, cyc, nCycles, b, out, recBase + 4 * (cyc & (recSlots - 1)),
                                       legValid);
                }
                allValid &= legValid;
            }
            pose_sync<16>();
            // footholdValidation_ = AND of the swing legs' flags (cpp:1323); commit or skip (cpp:1332-1576)
            const bool phaseOk = allValid != 0;
            if (phaseOk && tid < 24) {
                // x and y of the three tracks' next positions, straight from the staged record (its first six doubles: nominal,
                // centroid, default track); no later cycle reads a committed z (getPolygonCenter, cpp:2421-2463)
                const int leg = tid / 6, e = tid - leg * 6;
                if ((mask >> leg) & 1u) {
                    const double* rd = reinterpret_cast<const double*>(recBase + 4 * (cyc & (recSlots - 1)) + leg);
                    sh.cur[2 - (e >> 1)][leg][e & 1] = rd[e];
                }
            }
            pose_sync<16>();
            cycleOk = cycleOk && phaseOk;
        }
        if (tid == 0 && out.cycle_ok) out.cycle_ok[static_cast<size_t>(b) * nCycles + cyc] = cycleOk ? 1 : 0;
        adjY += kStride ? sv.drift : pc.drift;  // cpp:1578
        {   // the staged records of the last recSlots cycles: lane = (cycle slot, leg)
            const int slot = cyc & (recSlots - 1);
            if (slot == recSlots - 1 || cyc == nCycles - 1) {
                pose_sync<16>();
                // (the flush reads its constants and pointers from the argument segment as well where the leg loop does)
                constexpr bool kReloadF = kSeqReloadArgs<KW>;
                typedef const SeqKernArgs __attribute__((address_space(4))) * KernArgPtr;
                KernArgPtr kf4 = (KernArgPtr)kaArg;
                if constexpr (kReloadF) asm volatile("" : "+s"(kf4));
                const SeqKernArgs* kf = (const SeqKernArgs*)kf4;
                const DevMap& mF = kReloadF ? kf->m : m;
                const PlanConsts& pcF = kReloadF ? kf->pc : pc;
                const fpe_plan_out outF = kReloadF ? specialise_products<kProd>(kf->out) : out;
                const int nCycF = kReloadF ? kf->nCycles : nCycles, slotsF = kReloadF ? kf->recSlots : recSlots;
                Rec* const recF = kReloadF ? reinterpret_cast<Rec*>(smem + ((sizeof(PoseShared) + kLsBytes +
                                                                            4 * static_cast<size_t>(legbits_words(min(2 * pcF.winH + 1, NR), KW, pcF.nHW)) + 15) &
                                                                           ~static_cast<size_t>(15)))
                                           : recBase;
                {  // deferred heights: two lanes per (cycle, leg) unit
                    const int un = tid >> 1, c = (cyc - slot) + (un >> 2);
                    if (un < 4 * slotsF && c <= cyc) flush_seqrec2(mF, pcF, sh.footDa, sh.footDb, recF[un], b, c, un & 3, tid & 1, nCycF, outF, cycBase);
                }
                pose_sync<16>();  // the slots are rewritten next
            }
        }
    }
    if constexpr (kResume) {  // the state behind the last flush (the last phase's commit is behind its pose_sync)
        fpe_plan_state* stateOut = kaG->stateOut;
        if (stateOut && tid < 4) store_leg_state(stateOut, b, tid, sh.cur, adjY, cycBase + kaG->nCycles);
    }
}

// The kernel: kGroup wavefronts — poses — per workgroup, each runs seq_run_pose on its own slot of the workgroup's LDS.  kGroup 16 (one
// workgroup of 1 024 threads per CU; the launch's choice for batches of at least 64 poses on the 96-bit-row windows) or 1.
// Stride form (fpe_plan_strides*): S = {const fpe_stride*}, ONE trailing argument behind slotBytes, which the callee reads through
// SeqKernArgs::strides.  S empty (the default): the kernel and its argument segment as they always were.
// Resume form (fpe_plan_resume*): S = {const fpe_stride*, const fpe_plan_state*, fpe_plan_state*}, read through SeqKernArgs likewise.
template <int NRL, int KW, int kProd, int kGroup, class... S>
__global__ __launch_bounds__(64 * kGroup, kGroup == 1 ? kSeqWaves : 1) void plan_bits_seq_kernel(DevMap m, BitMap bm, PlanConsts pc, SpiralLut lut,
                                                                                                const fpe_pose* __restrict__ poses, int B, int nCycles, fpe_plan_out outArg,
                                                                                                int recSlots, int slotBytes, S... strideArg) {
    static_assert(sizeof...(S) <= 1 || sizeof...(S) == 3, "optional trailing arguments: the strides, or the strides and the two states");
    const int tid = static_cast<int>(threadIdx.x) & 63, wv = static_cast<int>(threadIdx.x) >> 6;
    const int b = static_cast<int>(blockIdx.x) * kGroup + wv;
    if (b >= B) return;
    const Grp<64> g(tid);
    const LutHead head = load_lut_head(lut, g);
    unsigned hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    (void)m; (void)bm; (void)poses; (void)nCycles; (void)outArg; (void)recSlots;
    ((void)strideArg, ...);
    typedef const SeqKernArgs __attribute__((address_space(4))) * KernArgPtr0;
    seq_run_pose<NRL, KW, kProd, sizeof...(S) != 0, sizeof...(S) == 3>((KernArgPtr0)__builtin_amdgcn_kernarg_segment_ptr(), wv * slotBytes, b, tid, hwid, head);
}
static_assert(kernargs_mirror<decltype(plan_bits_seq_kernel<1, 2, 0, 1>)>(
                  {offsetof(SeqKernArgs, m), offsetof(SeqKernArgs, bm), offsetof(SeqKernArgs, pc), offsetof(SeqKernArgs, lut),
                   offsetof(SeqKernArgs, poses), offsetof(SeqKernArgs, B), offsetof(SeqKernArgs, nCycles), offsetof(SeqKernArgs, out),
                   offsetof(SeqKernArgs, recSlots)},
                  offsetof(SeqKernArgs, recSlots) + sizeof(SeqKernArgs::recSlots)),
              "SeqKernArgs must mirror plan_bits_seq_kernel's parameters");
static_assert(kernargs_mirror<decltype(plan_bits_seq_kernel<1, 2, 0, 1, const fpe_stride*>)>(
                  {offsetof(SeqKernArgs, m), offsetof(SeqKernArgs, bm), offsetof(SeqKernArgs, pc), offsetof(SeqKernArgs, lut),
                   offsetof(SeqKernArgs, poses), offsetof(SeqKernArgs, B), offsetof(SeqKernArgs, nCycles), offsetof(SeqKernArgs, out),
                   offsetof(SeqKernArgs, recSlots), offsetof(SeqKernArgs, slotBytes), offsetof(SeqKernArgs, strides)},
                  offsetof(SeqKernArgs, strides) + sizeof(SeqKernArgs::strides)),
              "SeqKernArgs must mirror the parameters of plan_bits_seq_kernel's stride form");
static_assert(kernargs_mirror<decltype(plan_bits_seq_kernel<1, 2, 0, 1, const fpe_stride*, const fpe_plan_state*, fpe_plan_state*>)>(
                  {offsetof(SeqKernArgs, m), offsetof(SeqKernArgs, bm), offsetof(SeqKernArgs, pc), offsetof(SeqKernArgs, lut),
                   offsetof(SeqKernArgs, poses), offsetof(SeqKernArgs, B), offsetof(SeqKernArgs, nCycles), offsetof(SeqKernArgs, out),
                   offsetof(SeqKernArgs, recSlots), offsetof(SeqKernArgs, slotBytes), offsetof(SeqKernArgs, strides),
                   offsetof(SeqKernArgs, stateIn), offsetof(SeqKernArgs, stateOut)},
                  offsetof(SeqKernArgs, stateOut) + sizeof(SeqKernArgs::stateOut)),
              "SeqKernArgs must mirror the parameters of plan_bits_seq_kernel's resume form");
