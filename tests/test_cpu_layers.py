"""CPU-only checks of the message-layer export (fpe_export_layers*, include/fpe.h): the layer names follow the header's ids, the
library exports both entry points, and the binding refuses unknown names itself.  (Layouts and prototypes: tests/test_cpu_abi.py.)"""
import ctypes as C

import pytest

from quadrupedal_foothold_planner_amd import _capi
from tests import abi_c

NAMES = ("fpe_export_layers", "fpe_export_layers_device")
IDS = ("FOOTHOLD_FLAGS", "FOOTHOLD_HEIGHT", "SNAP_DI", "SNAP_DJ", "SNAP_SOURCE", "SNAP_Z", "CENTROID_CODE", "CENTROID_DI",
       "CENTROID_DJ", "CENTROID_Z")


def test_layer_ids_follow_the_header(tmp_path):
    out = abi_c.compile_and_run(tmp_path, '  printf("' + " ".join(["%d"] * (len(IDS) + 1)) + '\\n", '
                                + ", ".join("FPE_LAYER_" + n for n in IDS) + ", FPE_LAYER_COUNT);")
    assert list(map(int, out.split())) == list(range(len(IDS))) + [len(IDS)]
    assert _capi.LAYER_NAMES == tuple(n.lower() for n in IDS) and _capi.LAYER_COUNT == len(IDS)


def test_build_produces_a_library_that_exports_both_symbols():
    from quadrupedal_foothold_planner_amd import build as fbuild

    path = fbuild.build_engine()
    assert set(NAMES) <= set(_capi.EXPORTED_SYMBOLS)
    L = C.CDLL(path)
    for name in NAMES:
        assert hasattr(L, name), name
    assert _capi.lib() is not None


def test_unknown_layer_names_raise_before_the_library_is_called():
    """_layer_request needs no engine: an unknown name is a ValueError of the binding."""
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

    p = object.__new__(FootholdPlanner)  # no engine behind it: anything that reached the library would fail on the missing handle
    with pytest.raises(ValueError, match="unknown layers"):
        p.export_layers(layers=("snap_z", "no_such_layer"))
    with pytest.raises(ValueError, match="unknown layers"):
        p.export_layers_device({"heights": 1})
    p._h = None  # (what close() leaves: __del__ then has nothing to destroy)
