"""Frame codes (include/procgen2_vec.h pgv_frame_codes_enable) without a GPU: the three symbols' binding, the three structs as
a C compiler lays them out, and the rules of procgen2_amd/csrc/pg_frame_codes.h compiled for the CPU
(tests/cpp/test_frame_codes.cpp)."""
import ctypes
import os
import subprocess

import pytest

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pgv_frame_codes_enable", "pgv_frame_codes_get", "pgv_frame_codes"]
STRUCTS = [("pgv_frame_codes_config", pglib.FrameCodesConfig, 24), ("pgv_frame_code_table", pglib.FrameCodeTable, 56),
           ("pgv_frame_code_query", pglib.FrameCodeQuery, 56)]


def test_symbols_bound(engine_lib):
    args = [pglib.FrameCodesConfig(24, 64, 0, 8, None), pglib.FrameCodeTable(56), pglib.frame_code_query("add")]
    for name, arg in zip(NAMES, args):
        fn = getattr(engine_lib, name)
        rest = (None, None, 0) if name == "pgv_frame_codes" else ()
        assert name in pglib.EXPORTED_VEC_SYMBOLS and fn.restype is pglib.c_int32
        assert fn(None, *rest, ctypes.byref(arg)) != 0 and engine_lib.pgv_last_error().startswith(name.encode() + b":")  # a NULL handle


@pytest.mark.parametrize("cname,mirror,size", STRUCTS)
def test_structs_as_a_c_compiler_lays_them_out(tmp_path, cname, mirror, size):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "procgen2_vec.h"\nint main(void) { printf("%%zu", sizeof(%s));\n' % cname +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in mirror._fields_) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f, _ in mirror._fields_] and got[0] == size


def test_rules_on_the_host(tmp_path):
    exe = str(tmp_path / "rules")
    subprocess.run(["g++", "-std=gnu++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_frame_codes.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and all(s in out.stdout for s in ("OK weight", "OK word", "OK key", "OK probe", "ALL OK")), out.stdout + out.stderr
