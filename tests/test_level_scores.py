"""Level replay scores (include/procgen2_vec.h pgv_level_scores_enable) without a GPU: the three symbols' binding, the
three structs as a C compiler lays them out, and the rule of procgen2_amd/csrc/pg_level_scores.h compiled for the CPU
(tests/cpp/test_level_scores.cpp), once more under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import pytest

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pgv_level_scores_enable", "pgv_level_scores_get", "pgv_level_scores_update"]
STRUCTS = [("pgv_level_scores_config", pglib.LevelScoresConfig, 16), ("pgv_level_score_table", pglib.LevelScoreTable, 56),
           ("pgv_level_score_update", pglib.LevelScoreUpdate, 40)]


def test_symbols_bound(engine_lib):
    args = [pglib.LevelScoresConfig(16, 0, 4, 2), pglib.LevelScoreTable(56), pglib.level_score_update(None)]
    for name, arg in zip(NAMES, args):
        fn = getattr(engine_lib, name)
        rest = (0, 1) if name.endswith("update") else ()
        assert name in pglib.EXPORTED_VEC_SYMBOLS and fn.restype is pglib.c_int32
        assert fn(None, *rest, ctypes.byref(arg)) != 0 and name.encode() in engine_lib.pgv_last_error()  # a NULL handle


@pytest.mark.parametrize("cname,mirror,size", STRUCTS)
def test_structs_as_a_c_compiler_lays_them_out(tmp_path, cname, mirror, size):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "procgen2_vec.h"\nint main(void) { printf("%%zu", sizeof(%s));\n' % cname +
                   "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in mirror._fields_) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f, _ in mirror._fields_] and got[0] == size


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "san"])
def test_rule_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "rule")
    subprocess.run(["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc")] + flags +
                   [os.path.join(ROOT, "tests", "cpp", "test_level_scores.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and all(s in out.stdout for s in ("OK fix", "OK accept", "OK walk", "OK finish", "ALL OK")), out.stdout + out.stderr
