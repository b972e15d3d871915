// fpe_plan_sequential_body.hpp — the text of plan_sequential_kernel, a piece of the kernel translation unit (inside namespace fpe,
// not stand-alone) that fpe_kernels.hip includes TWICE: FPE_SEQUENTIAL_STRIDE 0 defines plan_sequential_kernel exactly as it always
// was, 1 defines plan_sequential_stride_kernel (fpe_plan_strides*) — the same kernel with `strides` as its one trailing argument and
// the step and the drift of the pose read from strides[b]; 2 defines plan_sequential_resume_kernel (fpe_plan_resume*) — strides (null:
// the plan's own), state_in (null: the stance prologue) and state_out (null: not returned) behind the list.  A kernel that is no template cannot take the flag as a parameter, and
// a shared inlined body changed the register allocation of the existing kernel; the same text compiled twice does not.
// (no include guard)
#if FPE_SEQUENTIAL_STRIDE == 2
__global__ __launch_bounds__(64, 4) void plan_sequential_resume_kernel(DevMap m, PlanConsts pc, SpiralLut lut,
                                                                       const fpe_pose* __restrict__ poses, int B, int nCycles,
                                                                       fpe_plan_out out, const fpe_stride* __restrict__ strides,
                                                                       const fpe_plan_state* stateIn, fpe_plan_state* stateOut) {
#elif FPE_SEQUENTIAL_STRIDE
__global__ __launch_bounds__(64, 4) void plan_sequential_stride_kernel(DevMap m, PlanConsts pc, SpiralLut lut,
                                                                       const fpe_pose* __restrict__ poses, int B, int nCycles,
                                                                       fpe_plan_out out, const fpe_stride* __restrict__ strides) {
#else
__global__ __launch_bounds__(64, 4) void plan_sequential_kernel(DevMap m, PlanConsts pc, SpiralLut lut,
                                                                const fpe_pose* __restrict__ poses, int B, int nCycles,
                                                                fpe_plan_out out) {
#endif
    constexpr int G = 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = static_cast<int>(threadIdx.x);
    const Grp<G> g(tid);
    PoseShared& sh = *reinterpret_cast<PoseShared*>(smem);
    uint8_t* tile = smem + sizeof(PoseShared);
    const int b = blockIdx.x;
    if (b >= B) return;
    const bool live = true;

    const fpe_pose* pp = poses + b;
    const double x0 = pp->position[0], y0 = pp->position[1], z0 = pp->position[2];
    const int gait = pp->gait;
#if FPE_SEQUENTIAL_STRIDE == 2
    constexpr bool kStride = true;
    const StrideVals sv = load_stride_or_plan(strides, b, pc);
#elif FPE_SEQUENTIAL_STRIDE
    constexpr bool kStride = true;
    const StrideVals sv = load_stride(strides, b);
#else
    constexpr bool kStride = false;
    const StrideVals sv{};
#endif
    const LutHead head = load_lut_head(lut, g);
    for (int k = tid; k < pc.nFoot; k += G) {
        sh.footDa[k] = pc.footDa[k];
        sh.footDb[k] = pc.footDb[k];
        sh.footOff[k] = static_cast<int16_t>(pc.footDa[k] * pc.tileW + pc.footDb[k]);
    }
    double adjY = 0.0;  // ajustedPose_[1], cpp:759
#if FPE_SEQUENTIAL_STRIDE == 2
    int cycBase = 0;  // gait_cycle_id of the call's first cycle
    const bool started = stateIn == nullptr;
    if (!started) {  // (uniform) the committed feet, the running drift and the cycle index of an earlier call instead of the stance
        const LegState st = load_leg_state(stateIn, b, tid & 3);  // lane = leg (every lane loads: the verdict is a ballot)
        const bool poseFinite = __ballot(!st.finite) == 0ull;
        adjY = st.adjY;
        cycBase = st.cycle;
        if (tid < 4) {
            for (int t = 0; t < 3; ++t) {
                sh.cur[t][tid][0] = poseFinite ? st.x[t] : __builtin_nan("");
                sh.cur[t][tid][1] = st.y[t];
                sh.cur[t][tid][2] = 0.0;
            }
        }
    }
#else
    constexpr int cycBase = 0;
    constexpr bool started = true;
#endif
    // initial stance (cpp:350-378) and first-gait shift (setFirstGait, cpp:2679-2699): lane = leg
    if (started && tid < 4) {
        const int leg = tid;
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
    const int walkOrder = pc.RF_FIRST ? ((0) | (2 << 2) | (3 << 4) | (1 << 6)) : ((3) | (1 << 2) | (0 << 4) | (2 << 6));

    for (int cyc = 0; cyc < nCycles; ++cyc) {
        bool cycleOk = true;
        for (int ph = 0; ph < nPhases; ++ph) {
            const unsigned mask = (gait == 1) ? (1u << ((walkOrder >> (2 * ph)) & 3)) : 0xFu;
            // feet-polygon centres: lane t computes track t (getPolygonCenter, cpp:2191, 2265)
            if (tid < 3) {
                sh.ctr[tid] = polygon_center_x(sh.cur[tid]);
            }
            if (tid < 4) sh.valid[tid] = 1;  // non-swing legs do not vote
            pose_sync<16>();
            for (int leg = 0; leg < 4; ++leg) {
                if (!((mask >> leg) & 1u)) continue;
                const LegStatic ls = make_leg_static(pc, pp, leg, m.g.res, lut);
                leg_phase<G>(m, pc, lut, head, sh, tile, g, leg, ls, y0, adjY, advance, cyc, nCycles, b, live, out, nullptr, cycBase);
            }
            pose_sync<16>();
            // footholdValidation_ = AND of the swing legs' flags (cpp:1323); commit or skip (cpp:1332-1576)
            const bool phaseOk = (sh.valid[0] & sh.valid[1] & sh.valid[2] & sh.valid[3]) != 0;
            if (phaseOk && tid < 36) {
                const int leg = tid / 9, e = tid - leg * 9;
                if ((mask >> leg) & 1u) {
                    const int t = e / 3, k = e - t * 3;
                    sh.cur[t][leg][k] = sh.nxt[t][leg][k];
                }
            }
            pose_sync<16>();
            cycleOk = cycleOk && phaseOk;
        }
        if (tid == 0 && out.cycle_ok) out.cycle_ok[static_cast<size_t>(b) * nCycles + cyc] = cycleOk ? 1 : 0;
        adjY += kStride ? sv.drift : pc.drift;  // cpp:1578
    }
#if FPE_SEQUENTIAL_STRIDE == 2
    if (stateOut && tid < 4) store_leg_state(stateOut, b, tid, sh.cur, adjY, cycBase + nCycles);  // (behind the last commit's pose_sync)
#endif
}

