// fpe_plan_launch.hpp — host side of every chained-plan kernel (included into fpe_kernels.hip behind fpe_bits.hpp, inside namespace
// fpe): WHICH kernel a call launches (select_plan_kernel), the instantiation list of each family (visit_*), and the three things
// done with an instantiation — launching it, raising its dynamic-LDS limit, printing its name.  The selection is a value
// (PlanKernel, fpe_launch.hpp): the engine asks it whether a form is launchable, describe_plan_kernel formats it, launch_plan and
// set_max_lds hand it to the same visitor, so no second copy of a rule can drift from the launch.
#pragma once

// ---- what is done with an instantiation ---------------------------------------------------------------------------------
// The arguments of a chained-plan launch, in no kernel's order: launch_as puts them into each family's own.
struct PlanCall {
    const DevMap& m;
    const BitMap* bm;
    const PlanConsts& pc;
    const SpiralLut& lut;
    const fpe_pose* poses;
    int B, nCycles;
    const fpe_plan_out& out;
    const PlanChain& chain;
    hipStream_t stream;
};
// The launch, through the kernel's own type.  The kernel's parameter list picks the overload — that is, the family's argument
// order — and its trailing parameters S (none, the strides, or the strides and both states) pick the chain's pointers by type, so
// the compiler checks every argument against the kernel's parameters.  An instantiation whose S does not match the form is refused.
template <class T>
static T chain_arg(const PlanChain& c) {
    if constexpr (std::is_same<T, const fpe_stride*>::value) return c.strides;
    else if constexpr (std::is_same<T, const fpe_plan_state*>::value) return c.stateIn;
    else return c.stateOut;
}
template <class... S>
static bool takes_form(PlanForm f) {
    return sizeof...(S) == (f == PlanForm::Plain ? 0 : f == PlanForm::Stride ? 1 : 3);
}
// 8 lanes per leg; C: the 3x3-only kernels take their own constants block, filled from this call's constants
template <class C, class... S>
static hipError_t launch_as(void (*kern)(const fpe_pose*, int, int, DevMap, BitMap, C, SpiralLut, fpe_plan_out, S...), const PlanKernel& k, const PlanCall& c) {
    if (!takes_form<S...>(k.form)) return hipErrorInvalidValue;
    C consts;
    if constexpr (std::is_same<C, PlanMidConsts>::value) consts = plan_mid_consts(c.pc);
    else consts = c.pc;
    hipLaunchKernelGGL(kern, dim3(k.grid), dim3(k.block), k.ldsBytes, c.stream, c.poses, c.B, c.nCycles, c.m, *c.bm, consts, c.lut, c.out,
                       chain_arg<S>(c.chain)...);
    return hipGetLastError();
}
// one wavefront per pose, bit window
template <class... S>
static hipError_t launch_as(void (*kern)(DevMap, BitMap, PlanConsts, SpiralLut, const fpe_pose*, int, int, fpe_plan_out, int, int, S...), const PlanKernel& k,
                            const PlanCall& c) {
    if (!takes_form<S...>(k.form)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(k.grid), dim3(k.block), k.ldsBytes, c.stream, c.m, *c.bm, c.pc, c.lut, c.poses, c.B, c.nCycles, c.out, k.recSlots,
                       k.slotBytes, chain_arg<S>(c.chain)...);
    return hipGetLastError();
}
// direct
template <class... S>
static hipError_t launch_as(void (*kern)(DevMap, PlanConsts, SpiralLut, const fpe_pose*, int, int, fpe_plan_out, S...), const PlanKernel& k, const PlanCall& c) {
    if (!takes_form<S...>(k.form)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(k.grid), dim3(k.block), k.ldsBytes, c.stream, c.m, c.pc, c.lut, c.poses, c.B, c.nCycles, c.out, chain_arg<S>(c.chain)...);
    return hipGetLastError();
}

// What a visitor below does with the instantiation it finds: raise its dynamic-LDS limit, launch it, both, or neither (the
// question is only whether it exists).
struct PlanUse {
    const PlanKernel& k;
    size_t ldsLimit = 0;             // nonzero: hipFuncAttributeMaxDynamicSharedMemorySize
    const PlanCall* call = nullptr;  // non-null: launch
    hipError_t err = hipSuccess;
    template <class K>
    void operator()(K* kern) {
        if (ldsLimit) err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ldsLimit));
        if (call && err == hipSuccess) err = launch_as(kern, k, *call);
    }
};

// ---- the instantiations, once per family --------------------------------------------------------------------------------
// Each visitor hands `use` the typed kernel that use.k stands for and returns true, or returns false where no such instantiation
// is compiled.  What is not named here is not in the code object.  (Plain functions, and the direct family first: the kernels are
// instantiated in the order they are named, and the code generated for one is not independent of what came before it.)
static bool visit_direct(PlanUse& use) {
    const PlanKernel& k = use.k;
    const int G = k.group;
    if (k.form != PlanForm::Plain) {  // at the automatic group sizes only, and never a 3x3-only variant
        if (k.mid || (G != 8 && G != 65)) return false;
        if (k.form == PlanForm::Resume) {
            if (G == 65) use(plan_sequential_kernel<const fpe_stride*, const fpe_plan_state*, fpe_plan_state*>);
            else use(plan_chained_kernel<8, false, const fpe_stride*, const fpe_plan_state*, fpe_plan_state*>);
        } else {
            if (G == 65) use(plan_sequential_kernel<const fpe_stride*>);
            else use(plan_chained_kernel<8, false, const fpe_stride*>);
        }
    } else if (G == 65 && !k.mid) use(plan_sequential_kernel<>);
    else if (G == 4 && !k.mid) use(plan_chained_kernel<4>);
    else if (G == 8 && k.mid) use(plan_chained_kernel<8, true>);
    else if (G == 8) use(plan_chained_kernel<8>);
    else if (G == 16 && !k.mid) use(plan_chained_kernel<16>);
    else if (G == 64 && !k.mid) use(plan_chained_kernel<64>);
    else return false;
    return true;
}

// plan_bits_chain_kernel<NRL, 0, S...>: the stride and resume forms of the 8-lane family
template <class... S>
static void visit_lane8_chain(PlanUse& use) {
    if (use.k.nrl == 2) use(plan_bits_chain_kernel<2, 0, S...>);
    else if (use.k.nrl == 3) use(plan_bits_chain_kernel<3, 0, S...>);
    else use(plan_bits_chain_kernel<4, 0, S...>);
}
static bool visit_lane8(PlanUse& use) {
    const PlanKernel& k = use.k;
    if (k.nrl < 2 || k.nrl > 4 || k.prod < 0 || k.prod > 2) return false;
    if (k.form != PlanForm::Plain) {  // generic variants, any-combination product mask
        if (k.mid || k.prod != 0) return false;
        if (k.form == PlanForm::Resume) visit_lane8_chain<const fpe_stride*, const fpe_plan_state*, fpe_plan_state*>(use);
        else visit_lane8_chain<const fpe_stride*>(use);
        return true;
    }
    switch (100 * k.nrl + 10 * k.mid + k.prod) {  // plan_bits_kernel<NRL, MID, PROD>
    case 212: use(plan_bits_kernel<2, true, 2>); break;
    case 211: use(plan_bits_kernel<2, true, 1>); break;
    case 210: use(plan_bits_kernel<2, true, 0>); break;
    case 202: use(plan_bits_kernel<2, false, 2>); break;
    case 201: use(plan_bits_kernel<2, false, 1>); break;
    case 200: use(plan_bits_kernel<2, false, 0>); break;
    case 312: use(plan_bits_kernel<3, true, 2>); break;
    case 311: use(plan_bits_kernel<3, true, 1>); break;
    case 310: use(plan_bits_kernel<3, true, 0>); break;
    case 302: use(plan_bits_kernel<3, false, 2>); break;
    case 301: use(plan_bits_kernel<3, false, 1>); break;
    case 300: use(plan_bits_kernel<3, false, 0>); break;
    case 412: use(plan_bits_kernel<4, true, 2>); break;
    case 411: use(plan_bits_kernel<4, true, 1>); break;
    case 410: use(plan_bits_kernel<4, true, 0>); break;
    case 402: use(plan_bits_kernel<4, false, 2>); break;
    case 401: use(plan_bits_kernel<4, false, 1>); break;
    case 400: use(plan_bits_kernel<4, false, 0>); break;
    default: return false;
    }
    return true;
}

// plan_bits_seq_kernel<NRL, KW, kProd, GRP, S...>: sixteen poses per workgroup on the 96-bit rows only
static bool visit_seq(PlanUse& use) {
    const PlanKernel& k = use.k;
    const int shape = (k.nrl == 1 && k.kw == 2 && k.group == 1) ? 0 : (k.nrl == 2 && k.kw == 3 && k.group == 16) ? 1 : (k.nrl == 2 && k.kw == 3 && k.group == 1) ? 2 : -1;
    if (shape < 0 || k.prod < 0 || k.prod > 1 || (k.form != PlanForm::Plain && k.prod != 0)) return false;
    if (k.form == PlanForm::Resume) {
        if (shape == 0) use(plan_bits_seq_kernel<1, 2, 0, 1, const fpe_stride*, const fpe_plan_state*, fpe_plan_state*>);
        else if (shape == 1) use(plan_bits_seq_kernel<2, 3, 0, 16, const fpe_stride*, const fpe_plan_state*, fpe_plan_state*>);
        else use(plan_bits_seq_kernel<2, 3, 0, 1, const fpe_stride*, const fpe_plan_state*, fpe_plan_state*>);
    } else if (k.form == PlanForm::Stride) {
        if (shape == 0) use(plan_bits_seq_kernel<1, 2, 0, 1, const fpe_stride*>);
        else if (shape == 1) use(plan_bits_seq_kernel<2, 3, 0, 16, const fpe_stride*>);
        else use(plan_bits_seq_kernel<2, 3, 0, 1, const fpe_stride*>);
    } else if (k.prod == 1) {
        if (shape == 0) use(plan_bits_seq_kernel<1, 2, 1, 1>);
        else if (shape == 1) use(plan_bits_seq_kernel<2, 3, 1, 16>);
        else use(plan_bits_seq_kernel<2, 3, 1, 1>);
    } else {
        if (shape == 0) use(plan_bits_seq_kernel<1, 2, 0, 1>);
        else if (shape == 1) use(plan_bits_seq_kernel<2, 3, 0, 16>);
        else use(plan_bits_seq_kernel<2, 3, 0, 1>);
    }
    return true;
}

// ---- the selection ------------------------------------------------------------------------------------------------------
// bits: the bit-window path applies (bits_supported, and the caller holds the planes).  B and productShape (product_shape) refine
// the instantiation within its family — the product mask, the sixteen-pose workgroups, the grid — and do not change the family,
// so a caller that asks only whether a form exists, or prints the kernel's name, passes 0 for both.
PlanKernel select_plan_kernel(const PlanConsts& pc, const MapGeom& g, bool bits, int B, int productShape, PlanForm form) {
    PlanKernel k{};
    k.family = PlanFamily::None;
    k.form = form;
    // the stride and resume forms are compiled without the 3x3-only variants and with the any-combination product mask only
    const bool plain = form == PlanForm::Plain;
    if (bits) {
        const BitsShape sp = bits_shape(pc.winH);
        k.nrl = sp.nrl, k.kw = sp.kw, k.winSide = 2 * pc.winH + 1;
        if (sp.lanes == 8) {  // two poses per wavefront
            k.family = PlanFamily::Lane8;
            k.mid = plain && mid_variant(pc, g.res) && pc.nFoot == 1;  // rf < res: the candidate disc is the candidate's own cell
            k.prod = plain ? productShape : 0;
            k.grid = (B + 1) / 2, k.block = 64;
            k.ldsBytes = 2 * (sizeof(PoseShared) + 16 * legbits_words(8 * k.nrl, 1, pc.nHW) +
                              (k.mid ? (sizeof(YEntry) + sizeof(Unit)) * 32 : (sizeof(YEntry) + sizeof(UnitG)) * 16));
        } else if (sp.lanes == 64) {
            k.family = PlanFamily::Seq;
            // (the all-seven shape takes the generic instantiation here: compiled on its own it spills more — cfg-5 +2 %, cfg-3 0)
            k.prod = plain && productShape == 1 ? 1 : 0;
            const size_t base = (sizeof(PoseShared) + ((4 * sizeof(LegStatic) + 15) & ~static_cast<size_t>(15)) +
                                 4 * legbits_words(2 * pc.winH + 1 < 64 * k.nrl ? 2 * pc.winH + 1 : 64 * k.nrl, k.kw, pc.nHW) + 15) &
                                ~static_cast<size_t>(15);
            k.recSlots = 8;  // cycles of staged records: as many as keep sixteen poses per CU (10 KiB each)
            while (k.recSlots > 1 && base + k.recSlots * 4 * sizeof(SeqRec) > 10240) k.recSlots >>= 1;
            const size_t slot = (base + k.recSlots * 4 * sizeof(SeqRec) + 15) & ~static_cast<size_t>(15);
            k.slotBytes = static_cast<int>(slot);
            // sixteen poses per workgroup — one workgroup per CU — where it was measured to pay: the 96-bit-row windows (cfg-5 -2 %; the
            // 64-bit-row kernel of cfg-3 +2 %), batches that fill at least four CUs, slots that fit sixteen times into the LDS
            k.group = (k.kw >= 3 && B >= 64 && 16 * slot <= 160 * 1024) ? 16 : 1;
            k.grid = (B + k.group - 1) / k.group, k.block = 64 * k.group;
            k.ldsBytes = k.group * slot;
        }
    } else {
        const int G = plan_group_size(pc);
        k.family = G == 65 ? PlanFamily::Sequential : PlanFamily::Chained;
        k.group = G;
        k.mid = plain && G == 8 && mid_variant(pc, g.res);
        k.grid = G == 4 ? (B + 3) / 4 : G == 8 ? (B + 1) / 2 : B, k.block = G == 64 ? 256 : 64;
        k.ldsBytes = plan_lds_bytes(pc);
        // the stride and resume forms exist at the automatic group sizes only: the instantiation list says which
        PlanUse exists{k};
        if (!visit_direct(exists)) k.family = PlanFamily::None;
    }
    return k;
}

hipError_t launch_plan(const DevMap& m, const BitMap* bm, const PlanConsts& pc, const SpiralLut& lut, const fpe_pose* d_poses, int B,
                       int nCycles, const fpe_plan_out& d_out, const PlanChain& chain, hipStream_t stream) {
    const PlanKernel k = select_plan_kernel(pc, m.g, bm != nullptr, B, product_shape(d_out), chain.form());
    const PlanCall call{m, bm, pc, lut, d_poses, B, nCycles, d_out, chain, stream};
    PlanUse use{k, 0, &call};
    bool found = false;
    if (k.family == PlanFamily::Lane8) {
        found = visit_lane8(use);
    } else if (k.family == PlanFamily::Seq) {
        if (k.ldsBytes > 64 * 1024) use.ldsLimit = k.ldsBytes;  // (the other families' limits: engine creation, set_max_lds)
        found = visit_seq(use);
    } else if (k.family != PlanFamily::None) {
        found = visit_direct(use);
    }
    return found ? use.err : hipErrorInvalidValue;
}

// Every direct plan instantiation may take up to `bytes` of dynamic LDS (engine creation).
static hipError_t set_max_lds_plan(size_t bytes) {
    for (const PlanForm form : {PlanForm::Plain, PlanForm::Stride, PlanForm::Resume})
        for (const int G : {4, 8, 16, 64, 65})
            for (const bool mid : {false, true}) {
                PlanKernel k{};
                k.family = G == 65 ? PlanFamily::Sequential : PlanFamily::Chained;
                k.form = form, k.group = G, k.mid = mid;
                PlanUse use{k, bytes};
                if (visit_direct(use) && use.err != hipSuccess) return use.err;
            }
    return hipSuccess;
}

// Which kernel a chained plan launches (evidence for bench.py / profiles): the family-level part of the selection, with
// "stride" / "resume" behind the name for the kernel a stride call (fpe_plan_strides*) or a resume call (fpe_plan_resume* with
// either state) launches.
void describe_plan_kernel(const PlanKernel& k, char* buf, size_t n) {
    const char* what = k.form == PlanForm::Resume ? "resume" : k.form == PlanForm::Stride ? "stride" : "";
    const char* sp = *what ? " " : "";
    const char* mid = k.mid ? "true" : "false";
    switch (k.family) {
    case PlanFamily::Lane8:
        snprintf(buf, n, "plan_bits_kernel<%d, %s>%s%s (8 lanes per leg, %d x %d bit window%s)", k.nrl, mid, sp, what, k.winSide, k.winSide,
                 k.mid ? ", 3x3-only fast path" : "");
        break;
    case PlanFamily::Seq:
        snprintf(buf, n, "plan_bits_seq_kernel<%d, %d>%s%s (one wavefront per pose, %d x %d bit window, %d-bit rows)", k.nrl, k.kw, sp, what,
                 k.winSide, k.winSide, 32 * k.kw);
        break;
    case PlanFamily::Sequential:
        snprintf(buf, n, "plan_sequential_kernel%s%s (direct, one wavefront per pose)", sp, what);
        break;
    case PlanFamily::Chained:
        snprintf(buf, n, "plan_chained_kernel<%d, %s>%s%s (direct)", k.group, mid, sp, what);
        break;
    case PlanFamily::None:
        snprintf(buf, n, "no %s kernel for plan_group %d", what, k.group);
        break;
    }
}
