"""CPU-only check of the dense foothold map's entry points (fpe_foothold_map*, include/fpe.h): the binding names them and the library
exports them.  (Layouts and prototypes: tests/test_cpu_abi.py.)"""
from quadrupedal_foothold_planner_amd import _capi


def test_foothold_map_symbols_are_exported():
    assert {"fpe_foothold_map", "fpe_foothold_map_device"} <= set(_capi.EXPORTED_SYMBOLS)
    L = _capi.lib()
    assert hasattr(L, "fpe_foothold_map") and hasattr(L, "fpe_foothold_map_device")
