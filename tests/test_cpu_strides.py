"""Per-pose strides (fpe_stride, fpe_plan_strides*, fpe_plan_rank_strides*; include/fpe.h) without a GPU: the C side of the new ABI,
the per-pose oracle helper against the oracle's own batch plan, and the condition the GPU tests rest on — their mixed-stride inputs
tell an engine that ignores the strides, or reads the batch neighbour's, from a correct one."""
import numpy as np
import pytest

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi
from tests import abi_c
from tests import stride_reference as sref
from tests import util

C_PROTOTYPES = {
    "fpe_plan_strides": "int (*)(fpe_handle, const fpe_params*, const fpe_pose*, const fpe_stride*, int32_t, int32_t, const fpe_plan_out*)",
    "fpe_plan_strides_device": "int (*)(fpe_handle, const fpe_params*, const fpe_pose*, const fpe_stride*, int32_t, int32_t, "
                               "const fpe_plan_out*, void*)",
    "fpe_plan_rank_strides": "int (*)(fpe_handle, const fpe_params*, const fpe_rank_params*, const fpe_pose*, const fpe_stride*, int32_t, "
                             "int32_t, int32_t, const fpe_rank_out*)",
    "fpe_plan_rank_strides_device": "int (*)(fpe_handle, const fpe_params*, const fpe_rank_params*, const fpe_pose*, const fpe_stride*, "
                                    "int32_t, int32_t, int32_t, const fpe_plan_out*, const fpe_rank_out*, void*)",
    "fpe_describe_plan_strides": "int (*)(fpe_handle, const fpe_params*, char*, int32_t)",
}


def test_stride_abi_is_plain_c_and_leaves_the_version_alone(tmp_path):
    """fpe_stride is 16 bytes (offsets 0 / 4 / 8), the five entry points assign to plain-C function pointers under warnings as
    errors, FPE_ABI_VERSION still prints 5, and every new symbol is in the binding's table and in the library."""
    decls = "".join(f"  {proto.replace('(*)', f'(*p{k})')} = {name}; (void)p{k};\n" for k, (name, proto) in enumerate(C_PROTOTYPES.items()))
    body = ("  fpe_stride st = {0.09f, 0, -0.007};\n  (void)st;\n"
            '  printf("%zu %zu %zu %zu %d %zu\\n", sizeof(fpe_stride), offsetof(fpe_stride, step_length), offsetof(fpe_stride, reserved), '
            "offsetof(fpe_stride, lateral_drift), FPE_ABI_VERSION, sizeof(fpe_pose));")
    assert abi_c.compile_and_run(tmp_path, body, decls).split() == ["16", "0", "4", "8", "5", "64"]
    D = _capi.STRIDE_DTYPE
    assert D.itemsize == 16 and [D.fields[f][1] for f in ("step_length", "reserved", "lateral_drift")] == [0, 4, 8]
    assert D.fields["step_length"][0] == np.dtype("<f4") and D.fields["lateral_drift"][0] == np.dtype("<f8")
    assert _capi.STRUCTS["fpe_stride"] is D and _capi.ABI_VERSION == 5
    L = _capi.lib()
    assert L.fpe_abi_version() == 5
    for name in C_PROTOTYPES:
        assert name in _capi.PROTOTYPES and hasattr(L, name), name


@pytest.mark.parametrize("row_id", ["w7_gen", "w16_seq"])
def test_helper_with_uniform_strides_is_the_oracles_batch_plan(row_id):
    """Every stride equal to the parameters' pair: B one-pose oracle calls reproduce OracleMap.plan on the whole batch, byte for byte."""
    c = sref.case(row_id)
    omap = fpo.OracleMap(c["trav"], c["elev"], c["row"].res)
    op, opo = util.to_oracle_params(c["params"]), util.to_oracle_poses(c["poses"])
    whole = omap.plan(op, opo, 9, threads=4)
    whole["pose_status"] = omap.pose_status(op, opo)
    got = sref.reference(row_id, 9, "uniform")
    for k in sref.PLAN_KEYS:
        assert got[k].dtype == whole[k].dtype and got[k].shape == whole[k].shape, k
        assert got[k].tobytes() == whole[k].tobytes(), k


def _differs(a, b):
    """per pose: some element differs (NaN == NaN)"""
    B = a.shape[0]
    return util._neq(a, b).reshape(B, -1).any(axis=1)


@pytest.mark.parametrize("n", sref.CYCLES)
@pytest.mark.parametrize("row_id", list(sref.CASE_B))
def test_gpu_inputs_tell_strides_apart(row_id, n):
    """The condition behind tests/test_gpu_strides.py, on the oracle: (a) every pose whose stride is not the parameters' pair has a
    default_next x that differs from the uniform-stride plan — an engine that ignores the strides fails on each of them; (b) at least
    a quarter of the poses have some nominal record that differs when the pose is planned with the stride of its batch neighbour
    b ^ 1 instead of its own — an engine that reads the other pose slot's stride fails too."""
    c = sref.case(row_id)
    mixed, uniform, swapped = (sref.reference(row_id, n, kind) for kind in ("mixed", "uniform", "swapped"))
    own = (c["mixed"]["step_length"] != c["params"]["stepLength"][0]) | (c["mixed"]["lateral_drift"] != c["params"]["lateralDrift"][0])
    assert own.sum() >= c["B"] - (c["B"] + 4) // 5
    moved = _differs(mixed["default"][..., 0], uniform["default"][..., 0])
    assert moved[own].all(), np.nonzero(own & ~moved)[0]
    nominal_differs = np.zeros(c["B"], bool)
    for f in ("row", "col", "valid", "source", "x", "y"):
        nominal_differs |= _differs(mixed["nominal"][f], swapped["nominal"][f])
    assert nominal_differs.sum() * 4 >= c["B"], int(nominal_differs.sum())
