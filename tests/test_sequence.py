"""Steps without frames (include/procgen2_vec.h pgv_step_sequence) without a GPU: the new symbols in the built libraries and
their bindings, the summary's fold rule of procgen2_amd/csrc/pg_sequence.h compiled for the CPU (tests/cpp/test_sequence.cpp),
the model the GPU tests trust (tests/sequence_util.py) against T drawn oracle steps, and the ground the GPU tests' protocol
covers, counted on the oracle."""
import os
import subprocess

import numpy as np
import pytest

from oracle_util import OracleVec
from procgen2_amd import lib as pglib
from sequence_util import GAMES, PROTOCOL_N, PROTOCOL_STEPS, SequenceModel, fold, protocol_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("pgv_step_sequence", "pgv_step_sequence_host", "pgv_render_obs", "pgv_render_obs_host")


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libMaze.so"])
def test_sequence_symbols_exported(engine_lib, libname):
    path = os.path.join(pglib.LIB_DIR, libname)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names


def test_sequence_calls_bound(engine_lib):
    for name in SYMBOLS:
        assert getattr(engine_lib, name).restype is pglib.c_int32
        assert name in pglib.EXPORTED_VEC_SYMBOLS
    S = pglib.Sequence
    # the struct as the header lays it out (LP64): two words, a pointer, a 64-bit stride, two words, five pointers
    assert pglib.ctypes.sizeof(S) == 72
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 16, 24, 28, 32, 40, 48, 56, 64]
    assert pglib.FRAMES == {"last": 0, "none": 1}
    q = pglib.sequence(5, frames="none", run_seed=-1)
    assert (q.struct_size, q.steps, q.frames, q.run_seed, q.action_stride) == (72, 5, 1, 0xFFFFFFFF, 0) and not q.actions and not q.seq_done


def test_fold_rule_on_the_host(tmp_path):
    exe = str(tmp_path / "test_sequence")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_sequence.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK no done", "OK done places", "OK order", "OK T = 1", "OK listing", "ALL OK"):
        assert section in out.stdout, section


def test_numpy_fold_is_the_rule():
    """The model's fold on the rows the C++ test uses: the first done cuts, the sum is made in step order in float32."""
    r = np.array([[1, 10, 16777216, 1], [2, 0, 1, 1], [0, 1, 1, 16777216], [4, 1, 0, 0]], np.float32)
    d = np.array([[0, 1, 0, 0], [7, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 1]], np.uint8)
    ret, length, done = fold(r, d)
    assert list(length) == [2, 1, 4, 4] and list(done) == [1, 1, 0, 1]
    assert list(ret) == [3.0, 10.0, 16777216.0, 16777218.0] and ret.dtype == np.float32 and length.dtype == np.int32
    ret, length, done = fold(r[:1], d[:1])
    assert list(length) == [1, 1, 1, 1] and list(done) == [0, 1, 0, 0] and list(ret) == [1.0, 10.0, 16777216.0, 1.0]


@pytest.mark.parametrize("game", ["maze", "bossfight"])
def test_model_equals_drawn_oracle_steps(game):
    """Sequences of the model — drawing off on every sub-step but a drawn last one — against a second oracle that draws every
    step: the rows, the final observation of every call that drew one, the state dumps at the end; resets inside
    sequences, on their last sub-step and on the second-to-last (the drawn frame is then a reset frame) all occur."""
    n = 96
    m, o = SequenceModel(game, n), OracleVec(game, n)
    assert np.array_equal(m.reset(), o.reset())
    inside = last = second = 0
    for k, (t, actions) in enumerate(protocol_calls(n)):
        T = len(actions)
        draw = k % 3 != 2
        m.sequence(actions, draw_last=draw)
        for s in range(T):
            obs, reward, done = o.step(actions[s])
            assert np.array_equal(m.rewards[s].view(np.uint32), reward.view(np.uint32)) and np.array_equal(m.dones[s], done), (t, s)
        assert np.array_equal(m.engine_reward.view(np.uint32), reward.view(np.uint32)) and np.array_equal(m.engine_done, done)
        if draw:
            assert np.array_equal(m.obs, obs), "the drawn frame of the call at step %d" % t
        inside += int(m.dones[:T - 1].any(axis=0).sum())
        last += int(m.dones[T - 1].sum())
        second += int(m.dones[T - 2].sum()) if T >= 2 else 0
    assert inside >= 3 and last >= 1 and second >= 1, (inside, last, second)
    for i in range(n):
        assert np.array_equal(m.o.state(i).view(np.uint32), o.state(i).view(np.uint32)), "state of env %d" % i
    m.close(), o.close()


# The ground the GPU tests' protocol covers (tests/sequence_util.py), per game: dones inside a sequence (the reset is served
# inside it), on its last sub-step (the reset crosses the call), on the second-to-last (the rendered frame is a reset frame).
PROTOCOL_COVERAGE = {"coinrun": (39, 1, 5), "maze": (63, 18, 19), "bossfight": (458, 82, 79), "climber": (73, 20, 9),
                     "caveflyer": (50, 12, 10), "chaser": (148, 56, 23), "jumper": (87, 17, 19)}


@pytest.mark.parametrize("game", GAMES)
def test_protocol_covers_resets_at_every_place(game):
    m = SequenceModel(game, PROTOCOL_N, render=False)
    m.reset()
    inside = last = second = steps = 0
    for _, actions in protocol_calls():
        T = len(actions)
        _, dones = m.sequence(actions)
        inside += int((dones[:T - 1] != 0).sum())
        last += int((dones[T - 1] != 0).sum())
        second += int((dones[T - 2] != 0).sum()) if T >= 2 else 0
        steps += T
    m.close()
    assert steps == PROTOCOL_STEPS == 160
    assert (inside, last, second) == PROTOCOL_COVERAGE[game]
    assert inside >= 30 and last >= 1 and second >= 5
