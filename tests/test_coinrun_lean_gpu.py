"""coinrun's early-ended steps and handed-back frames (coinrun.hip), held to the oracle byte for byte: obs, reward bit patterns,
dones, state dumps.  A step that ends after fewer than four sub-steps owes its entities a redo, which the env's render
workgroup — or redo_kernel, in a step without a frame — does in a form of its own that is light on registers (entity_redo:
the ten spark lives held, x and y copied or stored where a spark respawns, the collision walk as loops).

  * 100 envs (a multiple of neither 8 nor 64: a partial pre-pass group, a partial wave of redo_kernel) under pgv_set_debug
    bit 23 (every third frame by the complete path), with masked resets on two consecutive steps;
  * real early ends, no debug bits: DEATH_N envs over DEATH_STEPS steps, in which the oracle alone counts at least 16 deaths
    (done with reward 0, long before the time limit) and at least 12 of them on a sub-step before the last, the redo
    (coinrun_lean_util.early_end tells from the oracle's state dumps);
  * the same seeds without frames: pgv_step_sequence(frames none) up to every step in which an env dies, then
    pgv_render_obs — redo_kernel runs the same entity_redo there.
"""
import numpy as np
import pytest

from engine_util import EngineVec
from episodes_util import synthetic_actions
from oracle_util import OracleVec, assert_same_dump
from coinrun_lean_util import DEATH_N, DEATH_RUN, DEATH_SEED, DEATH_STEPS, death_steps, early_deaths
from sequence_util import SequenceModel
from test_sequence_gpu import NONE, SeqEngine, check_rows

pytestmark = pytest.mark.gpu

BIT_HANDED_BACK = 1 << 23


def same_step(s, got, want):
    (oe, re_, de), (oo, ro, do) = got, want
    assert np.array_equal(de, do), "done, step %d" % s
    assert np.array_equal(re_.view(np.uint32), ro.view(np.uint32)), "reward bits, step %d" % s
    if not np.array_equal(oe, oo):
        bad = np.nonzero((oe != oo).any(axis=1))[0]
        raise AssertionError("obs differ at step %d in %d envs (first env %d, %d bytes)" %
                             (s, bad.size, bad[0], int((oe[bad[0]] != oo[bad[0]]).sum())))


def test_handed_back_frames_with_masked_resets(debug=BIT_HANDED_BACK):
    n, steps = 100, 80
    eng, ora = EngineVec("coinrun", n, seed_base=1), OracleVec("coinrun", n, seed_base=1)
    eng.set_debug(debug)
    assert np.array_equal(eng.reset(), ora.reset_obs()), "reset frame"
    for s in range(steps):
        a = synthetic_actions(0, s, n)
        same_step(s, eng.step(a), ora.step(a))
        if s in (30, 31):
            mask = ((np.arange(n) + s) % 3 == 0).astype(np.uint8)
            assert np.array_equal(eng.reset(mask=mask), ora.reset(mask=mask)), "masked reset at step %d" % s
        if s % 20 == 0:
            for e in range(0, n, 9):
                assert_same_dump(eng.state(e), ora.state(e), "state env %d, step %d" % (e, s))
    eng.close()
    ora.close()


def test_real_early_ends():
    died = death_steps()
    deaths = sum(len(d) for d in died)
    assert deaths >= 16, "the protocol must hold at least 16 deaths on the oracle alone (%d)" % deaths
    redone = sum(len(e) for e in early_deaths(died))  # … and three in four of 16 before the step's last sub-step: the redo
    assert redone >= 12, "deaths on a sub-step before the last, on the oracle alone (%d)" % redone
    n = DEATH_N
    eng, ora = EngineVec("coinrun", n, seed_base=DEATH_SEED), OracleVec("coinrun", n, seed_base=DEATH_SEED)
    assert np.array_equal(eng.reset(), ora.reset_obs()), "reset frame"
    seen = 0
    for s in range(DEATH_STEPS):
        a = synthetic_actions(DEATH_RUN, s, n)
        got, want = eng.step(a), ora.step(a, threads=8)
        same_step(s, got, want)
        ended = np.nonzero(want[2])[0]
        assert set(died[s]) <= set(ended)
        seen += len(died[s])
        for e in ended:  # the entity table the early-ended step's redo leaves
            assert_same_dump(eng.state(e), ora.state(e), "state env %d, step %d" % (e, s))
    assert seen == deaths
    eng.close()
    ora.close()


def test_early_ends_in_steps_without_frames():
    died = early_deaths(death_steps())  # the deaths on a sub-step before the last: redo_kernel's case
    ends = [s for s, d in enumerate(died) if len(d)]
    assert len(ends) >= 8, ends
    n = DEATH_N
    eng, model = SeqEngine("coinrun", n, seed_base=DEATH_SEED), SequenceModel("coinrun", n, seed_base=DEATH_SEED)
    assert np.array_equal(eng.reset(), model.first_reset())  # (one reset, as death_steps' oracle had: the same episodes)
    t = 0
    for last in ends:  # a sequence that ends with the step some env dies in: nothing drawn, then the frame asked for
        actions = np.stack([synthetic_actions(DEATH_RUN, k, n) for k in range(t, last + 1)])
        got = eng.sequence(actions, frames=NONE)
        model.sequence(actions, draw_last=True)
        check_rows(eng, model, got, t)
        assert (model.dones[-1][died[last]] != 0).all()
        assert np.array_equal(eng.render_obs(), model.obs), "pgv_render_obs after the sequence ending at step %d" % last
        for e in died[last]:
            assert_same_dump(eng.state(e), model.o.state(e), "state env %d, step %d" % (e, last))
        t = last + 1
    eng.close()
    model.close()
