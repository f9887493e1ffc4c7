"""V-trace over the transition ring (include/procgen2_vec.h pgv_transitions_vtrace) without a GPU: the symbol and its binding,
pgv_vtrace as a C compiler lays it out, and the rule of procgen2_amd/csrc/pg_vtrace.h compiled for the CPU
(tests/cpp/test_vtrace.cpp), once more under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import pytest

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pgv_transitions_vtrace"


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libMaze.so"])
def test_symbol_exported_and_bound(engine_lib, libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pglib.LIB_DIR, libname)], capture_output=True, text=True, check=True).stdout
    assert NAME in {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "procgen2_vec.h")).read()
    assert re.search(r"PGV_API int32_t %s\(" % NAME, header) and NAME in pglib.EXPORTED_VEC_SYMBOLS
    fn = getattr(engine_lib, NAME)
    assert fn.restype is pglib.c_int32 and fn.argtypes[1] is pglib.c_int64 and fn.argtypes[2] is pglib.c_int32
    q = pglib.vtrace(0.99, 1.0, None, None)
    assert fn(None, 0, 1, ctypes.byref(q)) != 0 and NAME.encode() in engine_lib.pgv_last_error()  # a NULL handle


def test_struct_as_a_c_compiler_lays_it_out(tmp_path):
    fields = [f if f != "lam" else "lambda" for f, _ in pglib.Vtrace._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "procgen2_vec.h"\nint main(void) { printf("%zu", sizeof(pgv_vtrace));\n' +
                   "".join('printf(" %%zu", offsetof(pgv_vtrace, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(pglib.Vtrace)] + [getattr(pglib.Vtrace, f).offset for f, _ in pglib.Vtrace._fields_]
    assert got[0] == 72 and pglib.Vtrace.values.offset == 32


@pytest.mark.parametrize("name,flags,args", [("plain", ["-O2"], []),
                                             ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["7"])])
def test_step_on_the_host(tmp_path, name, flags, args):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc")] + flags +
                   [os.path.join(ROOT, "tests", "cpp", "test_vtrace.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0 and all(s in out.stdout for s in ("OK patterns", "OK clips", "ALL OK")), out.stdout + out.stderr
