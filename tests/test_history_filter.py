"""Filtered history gathers (include/procgen2_vec.h pgv_history_gather_filter) without a GPU: the bindings, the engine's host
half — pgv_gather_filter_params — and procgen2_amd/csrc/pg_history_filter.h compiled for the CPU (tests/cpp/test_history_filter.cpp)
against the numpy draws of tests/history_filter_util.py."""
import ctypes
import os
import subprocess

import numpy as np

from history_aug_util import aug_params_many, config
from history_filter_util import turns_many
from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_params_match_the_model(engine_lib):
    """The struct as the header lays it out; the params row against numpy, aug NULL included; the host's refusals."""
    L, S = engine_lib, pglib.GatherFilter
    assert ctypes.sizeof(S) == 56 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 16, 24, 28, 32, 36, 40, 44, 48]
    row = (ctypes.c_int32 * 8)()
    for flip in (False, True):
        for rot90 in (False, True):
            f = pglib.gather_filter(3, None, flip=flip, rot90=rot90)
            for seed in (0, 1, 0xFFFFFFFF):
                cfg = config((56, 56, 4, 4, 24), color="random", seed=seed)
                a = pglib.gather_aug(56, 56, 4, "replicate", 4, 24, "random", seed)
                want = aug_params_many(cfg, np.arange(256))
                want[:, 7] = turns_many(seed, np.arange(256), flip, rot90)
                for e in range(256):
                    assert L.pgv_gather_filter_params(ctypes.byref(a), ctypes.byref(f), e, row) == 0 and list(row) == want[e].tolist()
            assert L.pgv_gather_filter_params(None, ctypes.byref(f), 5, row) == 0
            assert list(row) == [0] * 7 + [int(turns_many(0, [5], flip, rot90)[0])]
    tall, f = pglib.gather_aug(56, 48, seed=1), pglib.gather_filter(1, None, rot90=True)
    short = pglib.gather_filter(1, None)
    short.struct_size -= 1
    for a, g, e, out in ((tall, f, 0, row), (None, short, 0, row), (None, None, 0, row), (None, f, -1, row), (None, f, 0, None), (pglib.gather_aug(0, 8), f, 0, row)):
        assert L.pgv_gather_filter_params(None if a is None else ctypes.byref(a), None if g is None else ctypes.byref(g), e, out) != 0
        assert b"pgv_gather_filter_params" in L.pgv_last_error()
    assert L.pgv_history_gather_filter(None, None, None, 0, 4, 1, None, ctypes.byref(f), None) != 0 and b"pgv_history_gather_filter" in L.pgv_last_error()


def test_pg_history_filter_on_the_host(tmp_path):
    """pg_history_filter.h under g++: the turns against np.rot90's rule, every byte of the border image and every word a run
    reads in range, and its turn draws against numpy's."""
    exe = str(tmp_path / "test_history_filter")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_history_filter.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK turns", "OK image", "ALL OK"):
        assert section in out.stdout, section
    lines = [line.split() for line in out.stdout.splitlines() if line.startswith("turns ")]
    assert len(lines) == 12
    for _, seed, turns, *drawn in lines:
        assert [int(t) for t in drawn] == turns_many(int(seed), np.arange(256), int(turns) & 1, int(turns) & 2).tolist(), (seed, turns)
