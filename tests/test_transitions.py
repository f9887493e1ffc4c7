"""Transitions (include/procgen2_vec.h pgv_transitions_enable) without a GPU: the new symbols and their bindings, the structs
as a C compiler lays them out, the host half of procgen2_amd/csrc/pg_transitions.h compiled for the CPU
(tests/cpp/test_transitions.cpp), the model the GPU tests trust (tests/transitions_util.py) against plain-Python scalars, and
the ground the GPU tests' runs cover, counted on the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from episodes_util import SAME_STEP, synthetic_actions
from history_util import CALLS, N, RUN_SEED, T
from procgen2_amd import lib as pglib
from transitions_util import (CUT, GAE_L, GAE_PARAMS, GAE_T, GATHER_PARAMS, RECORDED, TERMINATED, TRUNCATED, VALID, VOID, TransitionModel,
                              TransitionsEpisodes, TransitionsVec, entries, gae_loop, run_counts)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "procgen2_amd", "csrc")

SYMBOLS = ("pgv_transitions_enable", "pgv_transitions_action", "pgv_transitions_reward", "pgv_transitions_flags", "pgv_transitions_gather",
           "pgv_transitions_gae")


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libMaze.so"])
def test_transition_symbols_exported(engine_lib, libname):
    path = os.path.join(pglib.LIB_DIR, libname)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names


def test_transition_calls_bound(engine_lib):
    L = engine_lib
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pglib.EXPORTED_VEC_SYMBOLS
    assert L.pgv_transitions_enable.restype is pglib.c_int32 and L.pgv_transitions_gather.restype is pglib.c_int32
    assert L.pgv_transitions_gae.restype is pglib.c_int32
    assert L.pgv_transitions_gae.argtypes[1] is pglib.c_int64 and L.pgv_transitions_gae.argtypes[2] is pglib.c_int32
    assert L.pgv_transitions_gather.argtypes[3] is pglib.c_int32
    for getter in (L.pgv_transitions_action, L.pgv_transitions_reward, L.pgv_transitions_flags):
        assert getter.restype is pglib.c_void_p and getter(None) is None
    assert (pglib.TR_RECORDED, pglib.TR_TERMINATED, pglib.TR_TRUNCATED, pglib.TR_VOID, pglib.TR_CUT) == (RECORDED, TERMINATED, TRUNCATED, VOID, CUT)
    # NULL handles: nothing is enabled, nothing is touched
    cfg = pglib.TransitionsConfig(ctypes.sizeof(pglib.TransitionsConfig), 0)
    assert L.pgv_transitions_enable(None, ctypes.byref(cfg)) != 0 and b"pgv_transitions_enable" in L.pgv_last_error()
    q = pglib.transition_query(3, 0.99, 4, "float16")
    assert L.pgv_transitions_gather(None, None, None, 0, ctypes.byref(q)) != 0 and b"pgv_transitions_gather" in L.pgv_last_error()
    g = pglib.gae(0.99, 0.95, None, None)
    assert L.pgv_transitions_gae(None, 0, 1, ctypes.byref(g)) != 0 and b"pgv_transitions_gae" in L.pgv_last_error()


def test_structs_as_a_c_compiler_lays_them_out(tmp_path):
    """sizeof and offsetof of the three structs and the flag values, from the header itself under gcc, against the ctypes mirror."""
    src = tmp_path / "layout.c"
    fields = {"pgv_transitions_config": ["struct_size", "reserved"],
              "pgv_transition_query": ["struct_size", "n", "gamma", "stack", "dtype", "obs", "next_obs", "action", "nstep_return", "discount", "steps", "status"],
              "pgv_gae": ["struct_size", "gamma", "lambda", "values", "trunc_values", "advantages", "returns"]}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "procgen2_vec.h"', "int main(void) {"]
    for name, fs in fields.items():
        lines.append('printf("%%s %%zu", "%s", sizeof(%s));' % (name, name))
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (name, f) for f in fs]
        lines.append('printf("\\n");')
    lines += ['printf("flags %d %d %d %d %d\\n", PGV_TR_RECORDED, PGV_TR_TERMINATED, PGV_TR_TRUNCATED, PGV_TR_VOID, PGV_TR_CUT);', "return 0; }"]
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, S in (("pgv_transitions_config", pglib.TransitionsConfig), ("pgv_transition_query", pglib.TransitionQuery), ("pgv_gae", pglib.Gae)):
        want = [ctypes.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
        assert [int(x) for x in out[name].split()] == want, name
    assert out["flags"] == "1 2 4 8 16"
    assert ctypes.sizeof(pglib.TransitionQuery) == 80 and pglib.TransitionQuery.obs.offset == 24 and ctypes.sizeof(pglib.Gae) == 48


def test_walk_gae_and_listing_on_the_host(tmp_path):
    """pg_transitions.h under g++: the n-step walk exhaustively over all flag and began patterns of six rows against a deque per
    env, the GAE step against a straight loop, the listing — and the same program once more under the address and
    undefined-behaviour sanitizers (every third pattern)."""
    for name, flags, args in (("test_transitions", ["-O2"], []),
                              ("test_transitions_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["3"])):
        exe = str(tmp_path / name)
        subprocess.run(["g++", "-std=gnu++17", "-ffp-contract=off", "-Wall", "-I" + CSRC] + flags +
                       [os.path.join(ROOT, "tests", "cpp", "test_transitions.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe] + args, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        for section in ("OK walk", "OK gae", "OK listing", "ALL OK"):
            assert section in out.stdout, (name, section)


def by_hand():
    """A ring of T = 6 and three envs, filled by hand through the model's own calls: pushes 0 .. 6 (head 7, pushes 1 .. 6 held)."""
    from history_util import HistoryRing
    ring = HistoryRing(3, 6, True)
    tr = TransitionModel(ring)
    frame = np.zeros((3, 64, 64, 3), np.uint8)
    ring.reset(frame)  # push 0
    rows = [  # (rewards, terminated, truncated, void, flagged before the push) of rows 0 .. 5
        ([1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]),
        ([2, 2, 2], [0, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]),      # env 1 terminates (next-step: began comes with the void step)
        ([4, 0, 4], [0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 0]),      # env 1: the reset's own step
        ([8, 8, 8], [0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 1]),      # env 2 truncated, same-step: began on the next frame
        ([.5, .5, .5], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]),   # env 0: somebody reset it from outside: CUT
        ([16, 16, 16], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]),
    ]
    for k, (r, te, tu, vo, fl) in enumerate(rows):
        ring.flag(np.array(fl))
        ring.push(frame)
        tr.record(np.full(3, 10 + k, np.int32), np.array(r, np.float32), te, tu, vo)
    return ring, tr


def test_model_by_hand():
    ring, tr = by_hand()
    assert ring.head == 7 and ring.T == 6
    w = lambda p, i, n, g=1.0: tr.walk_one(p, i, n, g)  # noqa: E731
    assert w(0, 0, 3)["steps"] == 0                                    # push 0 is no longer held
    assert w(6, 0, 3)["steps"] == 0 and w(7, 0, 3)["steps"] == 0       # the newest push has no successor yet
    got = w(1, 0, 6)                                                   # rows 1 .. 4, cut behind row 4
    assert (got["steps"], float(got["nstep_return"]), float(got["discount"]), got["status"], got["action"]) == (4, 14.5, 1.0, VALID | CUT, 11)
    got = w(1, 1, 3)                                                   # terminated at once
    assert (got["steps"], float(got["nstep_return"]), float(got["discount"]), got["status"]) == (1, 2.0, 0.0, VALID | TERMINATED)
    assert w(2, 1, 3)["status"] == 0                                   # a void row is no entry
    got = w(3, 1, 3)                                                   # ... and the rows behind it are: runs out of the ring
    assert (got["steps"], float(got["nstep_return"]), got["status"]) == (3, 24.5, VALID)
    got = w(2, 2, 5, 0.5)
    assert (got["steps"], float(got["nstep_return"]), float(got["discount"]), got["status"]) == (2, 8.0, 0.25, VALID | TRUNCATED)
    assert w(1, 3, 3)["status"] == 0 and w(1, -1, 3)["status"] == 0
    # the vectorised walk is the scalar one, over everything
    p, i = entries(ring.head, ring.T, 3)
    for n, gamma in GATHER_PARAMS:
        vec = tr.walk(p, i, n, gamma)
        for b in range(p.size):
            one = tr.walk_one(int(p[b]), int(i[b]), n, gamma)
            assert all(np.asarray(vec[k][b]).tobytes() == np.asarray(one[k], vec[k].dtype).tobytes() for k in one), (p[b], i[b], n, gamma)
    # an unrecorded row is taken for nothing, and a stale row never for a new one
    ring.push(np.zeros((3, 64, 64, 3), np.uint8))
    tr.unrecorded()  # row 6, in the slot row 0 had
    assert not tr.flags[0].any() and w(6, 0, 3)["steps"] == 0 and w(5, 0, 3)["steps"] == 1
    # GAE: gamma = lambda = 1 and V = 0 sum the rewards to the episode's end
    ring, tr = by_hand()
    V = np.zeros((6, 3), np.float32)
    adv, ret = tr.gae(1, 5, V, 1.0, 1.0)
    assert adv[:, 0].tolist() == [14.5, 12.5, 8.5, 0.5, 16.0]          # cut behind row 4
    assert adv[:, 1].tolist() == [2.0, 0.0, 24.5, 16.5, 16.0]          # terminated, void, then one episode
    assert adv[:, 2].tolist() == [14.0, 12.0, 8.0, 16.5, 16.0]         # truncated behind row 3, nothing to bootstrap from
    tv = np.full((5, 3), 100.0, np.float32)
    adv, _ = tr.gae(1, 5, V, 1.0, 1.0, tv)
    assert adv[:, 2].tolist() == [114.0, 112.0, 108.0, 16.5, 16.0] and adv[:, 0].tolist() == [14.5, 12.5, 8.5, 0.5, 16.0]


@pytest.mark.parametrize("game,mode,limit", [("maze", SAME_STEP, 7), ("bossfight", "next_step", 0)])
def test_gae_model_against_the_scalar_loop(game, mode, limit):
    """The GAE engine's run on the oracle: T = 17, a stretch of 16 rows, values from a seeded draw; the vectorised model is the
    scalar loop bit for bit, with and without trunc_values."""
    m = TransitionsEpisodes(game, N, mode, GAE_T, True, max_episode_steps=limit)
    m.first_reset()
    for t in range(CALLS):
        m.step(synthetic_actions(RUN_SEED, t, N))
    rng = np.random.default_rng(11)
    V = rng.standard_normal((GAE_L + 1, N)).astype(np.float32)
    tv = rng.standard_normal((GAE_L, N)).astype(np.float32)
    first = m.ring.head - 1 - GAE_L
    ended = 0
    for gamma, lam in GAE_PARAMS:
        for trunc in (None, tv):
            adv, ret = m.tr.gae(first, GAE_L, V, gamma, lam, trunc)
            for i in (0, 1, 63, 64, 65, N - 1):
                a, r = gae_loop(m.tr, first, GAE_L, V, gamma, lam, trunc, i)
                assert a.tobytes() == adv[:, i].tobytes() and r.tobytes() == ret[:, i].tobytes(), (gamma, lam, i)
    slots = [(first + t) % GAE_T for t in range(GAE_L)]
    ended = int(((m.tr.flags[slots] & (TERMINATED | TRUNCATED | VOID)) != 0).sum())
    assert ended >= 30, ended
    m.close()


# What the GPU runs reach, on the oracle alone: N = 131, 40 calls, synthetic actions with run seed 7, seed_base 1.

def test_maze_run_terminates_and_truncates():
    c = run_counts("maze", SAME_STEP, 7)
    assert c["terminated"] >= 50 and c["truncated"] >= 600, c
    assert c["void"] == 0 and c["cut_short"] >= 100, c  # same-step: no reset step is ever seen


def test_bossfight_run_has_void_rows_and_negative_rewards():
    c = run_counts("bossfight", "next_step", 0)
    assert c["terminated"] >= 30 and c["void"] >= 30, c
    assert c["rewards"].get(-10.0, 0) >= 30 and c["truncated"] == 0, c


def test_chaser_run_has_rewards_that_round():
    c = run_counts("chaser", SAME_STEP, 7)
    assert c["rewards"].get(float(np.float32(0.04)), 0) >= 300, c
    assert c["rounded"] >= 100, c  # n-step returns at gamma 0.99 that differ from the plain sum


def test_plain_steps_record_the_done_row():
    """pgv_step's rows on the oracle: TERMINATED from the done row, VOID on the step behind it, never TRUNCATED; CUT where a
    masked reset came in between."""
    m = TransitionsVec("bossfight", N, T, True)
    m.first_reset()
    seen = dict(t=0, v=0, cut=0)
    for t in range(CALLS):
        before = m.o.done.copy()
        m.step(synthetic_actions(RUN_SEED, t, N))
        fl = m.tr.flags[(m.ring.head - 2) % T]
        assert np.array_equal((fl & VOID) != 0, before != 0) and np.array_equal((fl & TERMINATED) != 0, m.o.done != 0) and not (fl & TRUNCATED).any()
        seen["t"] += int(((fl & TERMINATED) != 0).sum())
        seen["v"] += int(((fl & VOID) != 0).sum())
        if t in (9, 22):
            m.reset(((np.arange(N) + t) % 4 == 0).astype(np.uint8))
        if t in (10, 23):
            w = m.tr.walk(*entries(m.ring.head, T, N), 3, 0.99)
            seen["cut"] += int(((w["status"] & CUT) != 0).sum())
    assert seen["t"] >= 20 and seen["v"] >= 20 and seen["cut"] >= 30, seen  # (the masked resets take some envs off their way to an end)
    m.close()
