"""CPU-only checks of the open-loop centroid method and the dense centroid map's C ABI (fpe_centroid_legs*, fpe_centroid_map*,
include/fpe.h): the header additions compile as plain C, the ctypes mirrors have the C layout, and the library exports the four
entry points."""
import ctypes as C
import os
import subprocess

import numpy as np

from quadrupedal_foothold_planner_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpe_centroid_legs", "fpe_centroid_legs_device", "fpe_centroid_map", "fpe_centroid_map_device")


def _compile_and_run(tmp_path, body, decls=""):
    """C99 with warnings as errors over the whole program (`decls` is checked for syntax only: it may name the library's
    functions), then the program without `decls` built and run (no library, no GPU)."""
    inc = "-I" + os.path.join(ROOT, "include")
    head = '#include "fpe.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
    full = tmp_path / "cmap_decls.c"
    full.write_text(head + decls + body + "\n  return 0;\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", inc, str(full)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = tmp_path / "cmap.c"
    src.write_text(head + body + "\n  return 0;\n}\n")
    exe = tmp_path / "cmap"
    r = subprocess.run(["gcc", "-std=c99", inc, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_centroid_declarations_are_plain_c(tmp_path):
    """Both structs and the four prototypes compile as C99 with warnings as errors; the ABI version is unchanged."""
    decls = ("  int (*f)(fpe_handle, const fpe_params*, const fpe_centroid_query*, int32_t, fpe_centroid_foothold*) = "
             "fpe_centroid_legs;\n"
             "  int (*g)(fpe_handle, const fpe_params*, const fpe_centroid_query*, int32_t, fpe_centroid_foothold*, void*) = "
             "fpe_centroid_legs_device;\n"
             "  int (*h)(fpe_handle, const fpe_params*, const int32_t*, float, const fpe_centroid_map_out*) = fpe_centroid_map;\n"
             "  int (*k)(fpe_handle, const fpe_params*, const int32_t*, float, const fpe_centroid_map_out*, void*) = "
             "fpe_centroid_map_device;\n"
             "  (void)f; (void)g; (void)h; (void)k;\n")
    out = _compile_and_run(tmp_path, "  fpe_centroid_map_out o = {0, 0, 0};\n  fpe_centroid_query q = {0.0, 0.0, 0.0f, 0};\n"
                                     "  (void)o; (void)q;\n"
                                     '  printf("%d\\n", FPE_ABI_VERSION);', decls)
    assert out.split() == ["5"]
    assert _capi.ABI_VERSION == 5


def test_centroid_query_layout_matches_the_mirrors(tmp_path):
    out = _compile_and_run(tmp_path, '  printf("%zu %zu %zu %zu %zu\\n", sizeof(fpe_centroid_query), '
                                     "offsetof(fpe_centroid_query, cx), offsetof(fpe_centroid_query, cy), "
                                     "offsetof(fpe_centroid_query, search_radius), offsetof(fpe_centroid_query, pad));")
    size, o_cx, o_cy, o_r, o_pad = map(int, out.split())
    assert size == 24
    M = _capi.CentroidQuery
    assert [name for name, _ in M._fields_] == ["cx", "cy", "search_radius", "pad"]
    assert (C.sizeof(M), M.cx.offset, M.cy.offset, M.search_radius.offset, M.pad.offset) == (size, o_cx, o_cy, o_r, o_pad)
    D = _capi.CENTROID_QUERY_DTYPE
    assert D.itemsize == size
    assert [D.fields[k][1] for k in ("cx", "cy", "search_radius", "pad")] == [o_cx, o_cy, o_r, o_pad]
    assert D.fields["search_radius"][0] == np.dtype("<f4")


def test_centroid_map_out_layout_matches_the_ctypes_mirror(tmp_path):
    out = _compile_and_run(tmp_path, '  printf("%zu %zu %zu %zu\\n", sizeof(fpe_centroid_map_out), '
                                     "offsetof(fpe_centroid_map_out, code), offsetof(fpe_centroid_map_out, offset), "
                                     "offsetof(fpe_centroid_map_out, z));")
    size, o_code, o_off, o_z = map(int, out.split())
    M = _capi.CentroidMapOut
    assert [name for name, _ in M._fields_] == ["code", "offset", "z"]  # the header's field order
    assert (C.sizeof(M), M.code.offset, M.offset.offset, M.z.offset) == (size, o_code, o_off, o_z)


def test_centroid_symbols_are_exported():
    assert set(NAMES) <= set(_capi.EXPORTED_SYMBOLS)
    L = _capi.lib()
    for name in NAMES:
        assert hasattr(L, name), name
