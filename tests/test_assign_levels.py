"""Assigned levels (include/procgen2_vec.h pgv_assign_levels), the CPU half: the reference model of the semantics
(tests/assign_util.py AssignModel, built on single oracle envs) is itself held to the oracle's vector wherever the two
describe the same thing — so that the yardstick of the GPU tests, and not the engine, defines the feature.
"""
import numpy as np
import pytest

from assign_util import GAME_STEPS, AssignModel, actions_of, run_schedule
from oracle_util import OracleVec, assert_same_dump
from test_levels import _fresh_make_obs


def _lockstep(model, ora, steps, n, each_step=None):
    assert np.array_equal(model.reset_obs(), ora.reset_obs()), "first reset"
    ends = 0
    for s in range(steps):
        a = actions_of(s, n)
        om, rm, dm = model.step(a)
        oo, ro, do = ora.step(a)
        assert np.array_equal(dm, do), "done, step %d" % s
        assert np.array_equal(rm.view(np.uint32), ro.view(np.uint32)), "reward bits, step %d" % s
        assert np.array_equal(om, oo), "obs, step %d" % s
        ends += int(do.sum())
        if each_step:
            each_step(s, do)
    for e in range(n):
        assert_same_dump(model.state(e), ora.state(e), "state env %d" % e)
        assert_same_dump(model.tiles(e), ora.tiles(e), "tiles env %d" % e)
    return ends


@pytest.mark.parametrize("game,steps", GAME_STEPS)
@pytest.mark.parametrize("num_levels,start_level", [(7, 50), (0, 0)])
def test_model_without_assignments_is_the_oracle_vector(game, steps, num_levels, start_level):
    n = 8
    model = AssignModel(game, n, seed_base=3, num_levels=num_levels, start_level=start_level)
    ora = OracleVec(game, n, seed_base=3, num_levels=num_levels, start_level=start_level)
    assert (model.level_known == (1 if num_levels else 0)).all()
    ends = _lockstep(model, ora, steps, n)
    assert ends > 0 or game in ("climber", "jumper", "coinrun", "caveflyer"), ends
    assert (model.level_known == (1 if num_levels else 0)).all()
    if num_levels:
        assert ((model.level_numbers >= start_level) & (model.level_numbers < start_level + num_levels)).all()
    else:
        assert (model.level_numbers == 0).all()
    # a masked reseeding reset, as test_levels.py makes it
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    seeds = (np.arange(n, dtype=np.int32) % 4) - 1
    assert np.array_equal(model.reset(mask=mask, seeds=seeds), ora.reset(mask=mask, seeds=seeds)), "masked reset"
    for s in range(steps, steps + 20):
        a = actions_of(s, n)
        for got, want in zip(model.step(a), ora.step(a)):
            assert np.array_equal(got, want), s
    model.close()
    ora.close()


@pytest.mark.parametrize("game,steps", GAME_STEPS)
@pytest.mark.parametrize("num_levels", [0, 7])
def test_model_with_every_episode_assigned_one_level_is_a_one_level_set(game, steps, num_levels):
    """Every level the model builds is assigned the same number L, in a free-mode engine and in one with a level set of
    its own: both are then OracleVec(num_levels=1, start_level=L)."""
    n, L = 6, 31337
    model = AssignModel(game, n, seed_base=3, num_levels=num_levels, start_level=50)
    ora = OracleVec(game, n, seed_base=9, num_levels=1, start_level=L)
    model.assign(range(n), [L] * n)
    model.reset()
    ora.reset()
    assert model.assigned_by_reset == n
    drawn_before = list(model.drawn)

    def each_step(s, done):
        model.assign(np.nonzero(done)[0], [L] * int(done.sum()))

    ends = _lockstep(model, ora, steps, n, each_step)
    assert model.assigned_by_auto == ends - int(np.count_nonzero(model.pending_reset))
    assert (model.level_known == 1).all() and (model.level_numbers == L).all()
    assert model.drawn == drawn_before, "an assigned level takes no place in the env's own sequence"
    model.close()
    ora.close()


def test_model_assignment_rules():
    """One pending assignment per env: overwritten by a later one, consumed by the level it builds, dropped by a reset with
    seeds; after the assigned episode a free-mode env goes on as the env made with that number goes on."""
    game, n = "maze", 4
    model = AssignModel(game, n, seed_base=5)
    model.assign([0, 0, 2, 7, -1], [10, 11, 12, 13, 14])  # env 0: the later one wins; 7 and -1: outside the batch
    model.assign([3], [99])
    obs = model.reset(mask=np.array([1, 1, 1, 0], np.uint8)).copy()
    assert np.array_equal(obs[0], _fresh_make_obs(game, 11)) and np.array_equal(obs[2], _fresh_make_obs(game, 12))
    assert list(model.level_known) == [1, 0, 1, 0] and list(model.level_numbers) == [11, 0, 12, 0]
    assert model.assigned == [None, None, None, 99]
    model.reset(mask=np.array([0, 0, 0, 1], np.uint8), seeds=np.array([0, 0, 0, 4], np.int32))  # drops env 3's
    assert model.assigned[3] is None and model.level_known[3] == 0
    # env 0 goes on as a single env made with seed 11 goes on
    L = model.L
    ref = L.pgo_make(game.encode(), 11, 1)
    L.pgo_present(ref)
    L.pgo_reset(ref, 0, 0)
    model.reset(mask=np.array([1, 0, 0, 0], np.uint8))
    assert np.array_equal(model.obs[0], np.ctypeslib.as_array(L.pgo_obs(ref), shape=(model.obs.shape[1],)))
    assert model.level_known[0] == 0 and model.level_numbers[0] == 0
    L.pgo_close(ref)
    model.close()


@pytest.mark.parametrize("game,steps", GAME_STEPS)
@pytest.mark.parametrize("num_levels", [7, 0])
def test_schedule_of_the_gpu_tests_exercises_what_it_claims(game, steps, num_levels):
    """The lock-step script the GPU tests run (assign_util.run_schedule), on the model alone: with these seeds and actions
    at least one assigned level is installed by the explicit reset in every game, and at least 8 by auto-resets in the
    three games whose episodes end within these step counts."""
    n = 96
    model = AssignModel(game, n, seed_base=3, num_levels=num_levels, start_level=50)
    run_schedule(model, model.assign, steps, n)
    print("\n%s num_levels=%d: %d assigned levels installed by explicit resets, %d by auto-resets"
          % (game, num_levels, model.assigned_by_reset, model.assigned_by_auto))
    assert model.assigned_by_reset >= 1
    if game in ("maze", "bossfight", "chaser"):
        assert model.assigned_by_auto >= 8
    model.close()
