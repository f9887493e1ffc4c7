"""Prioritised sampling (include/procgen2_vec.h pgv_priorities_enable) without a GPU: the new symbols and their bindings, the
struct as a C compiler lays it out, and what a NULL env is told."""
import ctypes
import os
import subprocess

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pgv_priorities_enable", "pgv_priorities", "pgv_priorities_max", "pgv_priorities_set", "pgv_priorities_sample")


def test_priority_calls_bound_and_refuse_a_null_env(engine_lib):
    L = engine_lib
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pglib.EXPORTED_VEC_SYMBOLS
    assert L.pgv_priorities_sample.argtypes[1] is pglib.c_int32 and L.pgv_priorities_set.argtypes[3] is pglib.c_int32
    for getter in (L.pgv_priorities, L.pgv_priorities_max):
        assert getter.restype is pglib.c_void_p and getter(None) is None
    assert L.pgv_priorities_enable(None) != 0 and b"pgv_priorities_enable" in L.pgv_last_error()
    assert L.pgv_priorities_set(None, None, None, 0, None) != 0 and b"pgv_priorities_set" in L.pgv_last_error()
    s = pglib.priority_sample(seed=-1, stratified=True)
    assert (s.struct_size, s.seed, s.stratified, s.pushes) == (ctypes.sizeof(pglib.PrioritySample), 0xFFFFFFFF, 1, None)
    assert L.pgv_priorities_sample(None, 0, ctypes.byref(s)) != 0 and b"pgv_priorities_sample" in L.pgv_last_error()


def test_struct_as_a_c_compiler_lays_it_out(tmp_path):
    fields = [f for f, _ in pglib.PrioritySample._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "procgen2_vec.h"', "int main(void) {",
             'printf("%zu", sizeof(pgv_priority_sample));']
    lines += ['printf(" %%zu", offsetof(pgv_priority_sample, %s));' % f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(pglib.PrioritySample)] + [getattr(pglib.PrioritySample, f).offset for f in fields]
    assert ctypes.sizeof(pglib.PrioritySample) == 56 and pglib.PrioritySample.pushes.offset == 16
