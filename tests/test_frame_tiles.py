"""The batched human-size frames (pgv_render_frames) without a GPU: the raster code the two frame painters share
(procgen2_amd/csrc/pg_raster.h) compiled for the CPU — whole frame == tile by tile == the oracle's spec_blit — and the
new symbols in the built libraries."""
import os
import subprocess

import pytest

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = ("64x64", "65x63", "131x77", "200x120", "512x512", "1x1")


def test_tiles_equal_the_whole_frame_and_the_oracle_spec(tmp_path):
    exe = str(tmp_path / "test_frame_tiles")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-mfma", "-ffp-contract=off", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "cpp", "test_frame_tiles.cpp"),
                    os.path.join(ROOT, "oracle", "pgo_raster.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK launch split", "OK row plans", "OK sample index", "ALL OK") + tuple("OK frame %s " % s for s in SIZES):
        assert section in out.stdout, section


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libCoinRun.so"])
def test_frames_symbols_exported(engine_lib, libname):
    path = os.path.join(pglib.LIB_DIR, libname)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pgv_render_frames", "pgv_render_frames_host"} <= names


def test_frames_calls_bound(engine_lib):
    for name in ("pgv_render_frames", "pgv_render_frames_host"):
        fn = getattr(engine_lib, name)
        assert fn.restype is pglib.c_int32 and len(fn.argtypes) == 6
        assert name in pglib.EXPORTED_VEC_SYMBOLS
