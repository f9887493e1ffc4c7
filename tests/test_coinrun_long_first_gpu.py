"""coinrun's handed-back frames drawn FIRST in the render launch (coinrun.hip render_kernel, Setup::hand_back): the pre-pass
lists the frames it leaves to the complete path, and the render grid has F early blocks in front of its n env blocks that
take them from the list — same function, same arguments, another block.  A frame the list has no room for is drawn in
place, as every such frame is under pgv_set_debug bit 27 (kDebugFatInPlace: F = 0, the grid of before).

  * 200 envs under bit 23 (every third frame handed back: 67 of them, F = clamp(200 / 256, 64, 1024) = 64 — 64 early, 3 in
    place), 60 steps with masked resets on two consecutive steps, against the oracle;
  * the same protocol under bits 23 and 23 | 27 on the engine: equal bytes, equal state;
  * the two list counters, which the pre-pass launches take in turn: 75 envs and 3 envs (n < F) under bit 23 — a step, then
    pgv_render_obs twice (two pre-pass / render pairs with no step between), a masked reset, a step, pgv_render_obs.
"""
import numpy as np
import pytest

from episodes_util import synthetic_actions
from oracle_util import OracleVec, assert_same_dump
from test_coinrun_lean_gpu import same_step
from test_sequence_gpu import SeqEngine

pytestmark = pytest.mark.gpu

BIT_HANDED_BACK = 1 << 23
BIT_IN_PLACE = 1 << 27
N, STEPS, RESETS = 200, 60, (30, 31)
assert len(range(0, N, 3)) == 67 and min(max(N // 256, 64), 1024) == 64  # three frames more than early blocks


def reset_mask(n, s):
    return ((np.arange(n) + s) % 3 == 0).astype(np.uint8)


def engine_run(debug):
    """The protocol on the engine alone: per step (obs, reward, done), the masked resets' frames, state dumps every 20 steps."""
    eng = SeqEngine("coinrun", N, seed_base=1)
    eng.set_debug(debug)
    first = eng.reset().copy()
    steps, resets, dumps = [], [], []
    for s in range(STEPS):
        steps.append(tuple(x.copy() for x in eng.step(synthetic_actions(0, s, N))))
        if s in RESETS:
            resets.append(eng.reset(mask=reset_mask(N, s)).copy())
        if s % 20 == 0:
            dumps.append([np.array(eng.state(e)) for e in range(0, N, 9)])
    eng.close()
    return first, steps, resets, dumps


@pytest.fixture(scope="module")
def early_run():
    return engine_run(BIT_HANDED_BACK)


def test_early_blocks_and_overflow_against_the_oracle(early_run):
    first, steps, resets, _ = early_run
    ora = OracleVec("coinrun", N, seed_base=1)
    assert np.array_equal(first, ora.reset_obs()), "reset frame"
    k = 0
    for s in range(STEPS):
        same_step(s, steps[s], ora.step(synthetic_actions(0, s, N)))
        if s in RESETS:
            assert np.array_equal(resets[k], ora.reset(mask=reset_mask(N, s))), "masked reset at step %d" % s
            k += 1
    ora.close()


def test_in_place_equals_early(early_run):
    first, steps, resets, dumps = early_run
    first_p, steps_p, resets_p, dumps_p = engine_run(BIT_HANDED_BACK | BIT_IN_PLACE)
    assert np.array_equal(first, first_p), "reset frame"
    for s in range(STEPS):
        same_step(s, steps[s], steps_p[s])
    for k, (a, b) in enumerate(zip(resets, resets_p)):
        assert np.array_equal(a, b), "masked reset %d" % k
    assert len(dumps) == len(dumps_p) == 3
    for k, (da, db) in enumerate(zip(dumps, dumps_p)):
        for j, (a, b) in enumerate(zip(da, db)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "state env %d, step %d" % (9 * j, 20 * k)


@pytest.mark.parametrize("n", [75, 3])
def test_the_list_counters(n):
    eng, ora = SeqEngine("coinrun", n, seed_base=1), OracleVec("coinrun", n, seed_base=1)
    eng.set_debug(BIT_HANDED_BACK)
    assert np.array_equal(eng.reset(), ora.reset_obs()), "reset frame"
    for s in range(3):
        a = synthetic_actions(0, s, n)
        want = ora.step(a)
        same_step(s, eng.step(a), want)
    one, two = eng.render_obs().copy(), eng.render_obs().copy()
    assert np.array_equal(one, two), "pgv_render_obs twice"
    assert np.array_equal(one, want[0]), "pgv_render_obs against the step's frame"
    mask = reset_mask(n, 0)
    assert np.array_equal(eng.reset(mask=mask), ora.reset(mask=mask)), "masked reset"
    a = synthetic_actions(0, 3, n)
    want = ora.step(a)
    same_step(3, eng.step(a), want)
    assert np.array_equal(eng.render_obs(), want[0]), "pgv_render_obs after a masked reset and a step"
    for e in range(0, n, 9):
        assert_same_dump(eng.state(e), ora.state(e), "state env %d" % e)
    eng.close()
    ora.close()
