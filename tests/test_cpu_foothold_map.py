"""CPU-only checks of the dense foothold map's C ABI (fpe_foothold_map*, include/fpe.h): the header additions compile as
plain C, the ctypes mirror of fpe_foothold_map_out has the C layout, and the library exports both entry points."""
import ctypes as C
import os
import subprocess

from quadrupedal_foothold_planner_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile_and_run(tmp_path, body, decls=""):
    """C99 with warnings as errors over the whole program (`decls` is checked for syntax only: it may name the library's
    functions), then the program without `decls` built and run (no library, no GPU)."""
    inc = "-I" + os.path.join(ROOT, "include")
    head = '#include "fpe.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
    full = tmp_path / "fmap_decls.c"
    full.write_text(head + decls + body + "\n  return 0;\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", inc, str(full)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = tmp_path / "fmap.c"
    src.write_text(head + body + "\n  return 0;\n}\n")
    exe = tmp_path / "fmap"
    r = subprocess.run(["gcc", "-std=c99", inc, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_foothold_map_declarations_are_plain_c(tmp_path):
    """The struct, the flag bits and both prototypes compile as C99 with warnings as errors."""
    decls = ("  int (*f)(fpe_handle, const fpe_params*, const int32_t*, const fpe_foothold_map_out*) = fpe_foothold_map;\n"
             "  int (*g)(fpe_handle, const fpe_params*, const int32_t*, const fpe_foothold_map_out*, void*) = fpe_foothold_map_device;\n"
             "  (void)f; (void)g;\n")
    out = _compile_and_run(tmp_path, "  fpe_foothold_map_out o = {0, 0};\n  (void)o;\n"
                                     '  printf("%u %u %u %d\\n", FPE_FMAP_DEFAULT_OK, FPE_FMAP_CANDIDATE_OK, FPE_FMAP_UNKNOWN, FPE_ABI_VERSION);',
                           decls)
    assert out.split() == ["1", "2", "4", "5"]
    assert (_capi.FMAP_DEFAULT_OK, _capi.FMAP_CANDIDATE_OK, _capi.FMAP_UNKNOWN) == (1, 2, 4)
    assert _capi.ABI_VERSION == 5


def test_foothold_map_out_layout_matches_the_ctypes_mirror(tmp_path):
    out = _compile_and_run(tmp_path, '  printf("%zu %zu %zu\\n", sizeof(fpe_foothold_map_out), offsetof(fpe_foothold_map_out, flags), '
                                     "offsetof(fpe_foothold_map_out, height));")
    size, off_flags, off_height = map(int, out.split())
    M = _capi.FootholdMapOut
    assert [name for name, _ in M._fields_] == ["flags", "height"]  # the header's field order
    assert (C.sizeof(M), M.flags.offset, M.height.offset) == (size, off_flags, off_height)


def test_foothold_map_symbols_are_exported():
    assert {"fpe_foothold_map", "fpe_foothold_map_device"} <= set(_capi.EXPORTED_SYMBOLS)
    L = _capi.lib()
    assert hasattr(L, "fpe_foothold_map") and hasattr(L, "fpe_foothold_map_device")
