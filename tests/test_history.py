"""Frame history (include/procgen2_vec.h pgv_history_enable) without a GPU: the new symbols in the built libraries and their
bindings, the host half of procgen2_amd/csrc/pg_history.h compiled for the CPU (tests/cpp/test_history.cpp), the model the
GPU tests trust (tests/history_util.py) against the PolicyStack of the policy observations — the law that ties the two
features — and the ground the GPU tests' episode runs cover, counted on the oracle."""
import os
import subprocess

import numpy as np
import pytest

from episodes_util import synthetic_actions
from history_util import CALLS, EPISODE_RUNS, N, RUN_SEED, T, HistoryEpisodes, HistoryRing, HistoryVec, cut_and_wrapped
from policy_obs_util import transform
from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("pgv_history_enable", "pgv_history_frames", "pgv_history_began", "pgv_history_pending", "pgv_history_head", "pgv_history_capacity",
           "pgv_history_push", "pgv_history_gather")


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libMaze.so"])
def test_history_symbols_exported(engine_lib, libname):
    path = os.path.join(pglib.LIB_DIR, libname)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names


def test_history_calls_bound(engine_lib):
    L = engine_lib
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pglib.EXPORTED_VEC_SYMBOLS
    assert L.pgv_history_enable.restype is pglib.c_int32 and L.pgv_history_push.restype is pglib.c_int32
    assert L.pgv_history_gather.restype is pglib.c_int32 and L.pgv_history_capacity.restype is pglib.c_int32
    assert L.pgv_history_head.restype is pglib.c_int64
    assert L.pgv_history_frames.restype is pglib.c_void_p and L.pgv_history_began.restype is pglib.c_void_p
    assert L.pgv_history_pending.restype is pglib.c_void_p
    S = pglib.HistoryConfig
    # the struct as the header lays it out (LP64): three words, four bytes of padding, a pointer
    assert pglib.ctypes.sizeof(S) == 24
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 16]
    # NULL handles: nothing is enabled, nothing is touched
    assert L.pgv_history_head(None) == -1 and L.pgv_history_capacity(None) == 0
    assert L.pgv_history_frames(None) is None and L.pgv_history_began(None) is None and L.pgv_history_pending(None) is None
    assert L.pgv_history_enable(None, None) != 0 and b"pgv_history_enable" in L.pgv_last_error()
    assert L.pgv_history_push(None) != 0 and b"pgv_history_push" in L.pgv_last_error()
    assert L.pgv_history_gather(None, None, None, 0, 4, 1, None) != 0 and b"pgv_history_gather" in L.pgv_last_error()


def test_walk_offsets_and_listing_on_the_host(tmp_path):
    """pg_history.h under g++: the walk, exhaustively against a deque per env; the slot and offset arithmetic, a case above
    2^32 bytes included; the listing."""
    exe = str(tmp_path / "test_history")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_history.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK walk", "OK offsets", "OK listing", "ALL OK"):
        assert section in out.stdout, section


def test_ring_model_by_hand():
    """The model on frames made up by hand: slots, held, began bytes, a stack cut by one, the walk off the ring, zero rows."""
    rng = np.random.default_rng(3)
    n, T = 3, 4
    ring = HistoryRing(n, T, False)
    frames = rng.integers(0, 256, (7, n, 64, 64, 3), dtype=np.uint8)
    for p in range(7):
        if p == 4:
            ring.flag(np.array([0, 1, 0]))
        ring.push(frames[p])
    assert ring.head == 7 and [ring.held(p) for p in (2, 3, 6, 7)] == [False, True, True, False]
    assert ring.began[0].tolist() == [0, 1, 0] and ring.began[3].tolist() == [0, 0, 0] and not ring.pending.any()  # slot 0 holds push 4
    assert ring.walk(6, 1, 4) == [6, 5, 4, 4] and ring.walk(6, 0, 4) == [6, 5, 4, 3] and ring.walk(5, 2, 8) == [5, 4, 3] + [3] * 5
    got = ring.gather([6, 6, 2, 7, -1, 6, 6], [1, 0, 0, 0, 0, -1, n], 4, "uint8")
    new = lambda p, i: transform(frames[p, i:i + 1], False, "uint8")[0]  # noqa: E731
    assert np.array_equal(got[0], np.concatenate([new(4, 1), new(4, 1), new(5, 1), new(6, 1)]))
    assert np.array_equal(got[1], np.concatenate([new(3, 0), new(4, 0), new(5, 0), new(6, 0)]))
    assert not got[2:].any()
    # a reset rewrites the newest slot under its mask and opens none
    ring.flag(np.array([0, 0, 1]))
    ring.reset(frames[0], np.array([1, 0, 0]))
    assert ring.head == 7 and ring.began[6 % T].tolist() == [1, 0, 0] and ring.pending.tolist() == [0, 0, 1]
    assert np.array_equal(ring.gather([6], [0], 2, "uint8")[0], np.concatenate([new(0, 0), new(0, 0)]))
    assert np.array_equal(ring.gather([6], [1], 2, "uint8")[0], np.concatenate([new(5, 1), new(6, 1)]))


@pytest.mark.parametrize("gray_rule,dtype", [(True, "float16"), (False, "uint8")])
def test_the_law_on_the_oracle(gray_rule, dtype):
    """131 maze envs, 40 steps, masked resets — the first of them before any step, at head == 0: after every call
    gather(head - 1, every env, K) of the ring model equals the PolicyStack fed by the same events."""
    K = 4
    m = HistoryVec("maze", N, T, gray_rule, policy=(K, dtype))
    first = (np.arange(N) % 3 != 0).astype(np.uint8)
    m.reset(first)  # head == 0: opens slot 0; the envs it leaves out keep zero rows and their flags
    assert m.ring.head == 1 and np.array_equal(m.ring.pending, 1 - first) and np.array_equal(m.ring.newest(K, dtype), m.stack.out)
    assert not m.ring.frames[0][first == 0].any()
    cut = 0
    for t in range(CALLS):
        m.step(synthetic_actions(RUN_SEED, t, N))
        assert np.array_equal(m.ring.newest(K, dtype), m.stack.out), t
        if t in (9, 22, 23):
            mask = ((np.arange(N) + t) % 4 == 0).astype(np.uint8)
            m.reset(mask)
            assert np.array_equal(m.ring.newest(K, dtype), m.stack.out), ("reset", t)
        assert np.array_equal(m.ring.pending, m.stack.restart), t
        cut += cut_and_wrapped(m.ring, K)[0]
    assert m.ring.head == CALLS + 1 and cut >= 10, cut
    m.close()


# What the GPU tests' episode runs reach, on the oracle: K-stacks, over every held push after every call, that a began byte
# cut, and that crossed the slot wrap.

@pytest.mark.parametrize("game,mode,limit", EPISODE_RUNS)
def test_episode_runs_cut_stacks_and_cross_the_wrap(game, mode, limit):
    m = HistoryEpisodes(game, N, mode, T, False, max_episode_steps=limit)
    m.first_reset()
    cut = wrapped = 0
    for t in range(CALLS):
        m.step(synthetic_actions(RUN_SEED, t, N))
        c, w = cut_and_wrapped(m.ring, 4)
        cut, wrapped = cut + c, wrapped + w
    m.close()
    assert cut >= 1 and wrapped >= 1, (cut, wrapped)
    if limit:  # every env is truncated every third step: began bytes all over the ring
        assert cut >= N * CALLS, cut
