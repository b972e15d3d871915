"""The C side of the ABI tests: include/fpe.h is a C boundary, so what the tests claim about it is checked by gcc as C99 with
warnings as errors, and what they read out of it (sizes, offsets, constants) is printed by a program gcc built from it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = "-I" + os.path.join(ROOT, "include")
STRICT = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", INC]


def compile_and_run(tmp_path, body, decls=""):
    """C99 with warnings as errors over the whole program (`decls` is checked for syntax only: it may name the library's
    functions), then the program without `decls` built and run (no library, no GPU); returns what it printed."""
    head = '#include "fpe.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
    full = tmp_path / "abi_decls.c"
    full.write_text(head + decls + body + "\n  return 0;\n}\n")
    r = subprocess.run(STRICT + [str(full)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = tmp_path / "abi.c"
    src.write_text(head + body + "\n  return 0;\n}\n")
    exe = tmp_path / "abi"
    r = subprocess.run(["gcc", "-std=c99", INC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout
