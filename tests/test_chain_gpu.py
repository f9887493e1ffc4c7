"""Carried container state deep in a level chain, against the oracle (need an MI355X).

The protocol "churn, then play" of tests/chain_util.py: rounds of masked resets, seeded and not, take every env of a batch
of 65 some twenty levels down its chain with no play between them, so that its sets' bucket counts are those of the largest
level it has seen and not those a fresh env would have; then a stretch of play in which sprites overlap and the order they
are listed in shows in the frames.  tests/test_chain.py asserts on the oracle alone that every case kept here tells the good
oracle from one that starts every level with fresh containers, by at least 20 env-steps in 5 envs — so an engine that
dropped, mis-saved or mis-restored a bucket count fails here.

  every path        each debug word of variant_paths_util.paths(game) side by side on one oracle run, every output bit for
                    bit after every call, state and tile rows of all envs after the churn and at the end; 65 envs, and one
                    env that is a witness env of the 65 over again (chaser, caveflyer);
  same-step         the play phase under step_episodes (same_step, a time limit, a ring of 4) on the default and the
                    no-prefetch path against the episodes model, where the terminal frames differ too (chaser, caveflyer);
  dropped           after the churn every env is assigned a level, a seeded reset drops it in half of them (chain_restore), the
                    other half consume theirs; built ahead and assigned right before the reset; against AssignModel (caveflyer);
  records           after the churn: save_envs of all envs loaded at shuffled slots of a fresh engine, a whole-batch
                    snapshot loaded into a second fresh engine; both play on beside the oracle.
"""
import numpy as np
import pytest

import chain_util as cu
import variant_paths_util as vp
from engine_util import EngineVec
from episodes_util import SAME_STEP, EpisodeModel
from oracle_util import OracleVec
from test_variant_paths_gpu import _same_frames

pytestmark = pytest.mark.gpu


def _engines(game, n, mode, paths, env_offset=0):
    engines = []
    for debug in paths:
        eng = EngineVec(game, n, seed_base=cu.SEED_BASE, mode=mode, env_offset=env_offset)
        if debug:
            eng.set_debug(debug)
        engines.append((vp.PATH_NAMES[debug], eng))
    return engines


def _same_step(name, got, t, obs, reward, done):
    oe, re_, de = got
    what = "%s, step %d" % (name, t)
    if not np.array_equal(de, done):
        raise AssertionError("%s: done differs, first env %d" % (what, np.nonzero(de != done)[0][0]))
    if not np.array_equal(re_.view(np.uint32), reward.view(np.uint32)):
        raise AssertionError("%s: reward bits differ, first env %d" % (what, np.nonzero(re_.view(np.uint32) != reward.view(np.uint32))[0][0]))
    _same_frames(oe, obs, what)


def _run_beside_the_oracle(game, mode, n, paths, env_offset=0):
    R, P, cast = cu.CASES[(game, mode)]
    engines = _engines(game, n, mode, paths, env_offset)
    ora = OracleVec(game, n, seed_base=cu.SEED_BASE, mode=mode, env_offset=env_offset)
    try:
        for name, eng in engines:
            _same_frames(eng.reset(), ora.reset_obs(), "%s, first reset" % name)

        def each_reset(r, mask, seeds, obs):
            for name, eng in engines:
                _same_frames(eng.reset(mask=mask, seeds=seeds), obs, "%s, churn round %d" % (name, r))

        def each_step(t, a, obs, reward, done):
            for name, eng in engines:
                _same_step(name, eng.step(a), t, obs, reward, done)

        def after_churn():
            for name, eng in engines:
                cu.assert_same_rows(name, eng, ora, n, "after the churn")

        churned, end = cu.run(ora, R, P, each_reset, each_step, after_churn, n=n, actions_of=cu.cast_actions(game, mode) if cast else None,
                              env_offset=env_offset)
        for name, eng in engines:
            cu.assert_same_rows(name, eng, ora, n, "after the last step")
        return churned
    finally:
        ora.close()
        for _, eng in engines:
            eng.close()


@pytest.mark.parametrize("game,mode", cu.cases())
def test_every_path_deep_in_the_chain(game, mode):
    churned = _run_beside_the_oracle(game, mode, cu.N, vp.paths(game))
    assert churned.median() >= cu.MIN_DEPTH and churned.reseeding >= 5


@pytest.mark.parametrize("game,mode", sorted(cu.SMALL_CASES))
def test_one_env_deep_in_the_chain(game, mode):
    """A one-env engine, the default path and the complete render path: a witness env of the 65 over again, at its
    env_offset (chain_util.SMALL_CASES; tests/test_chain.py test_the_one_env_case_is_a_witness)."""
    churned = _run_beside_the_oracle(game, mode, cu.SMALL_N, vp.SMALL_PATHS, cu.SMALL_CASES[(game, mode)])
    assert churned.median() >= cu.MIN_DEPTH


# ------------------------------------------------------------------------------------------------------ same-step installs

def _episode_engine(game, n, mode, debug):
    """tests/test_episodes_gpu.py's Engine (ProcgenVecEnv with same-step episodes, driven with host arrays) with the chain's
    seed base, seeded resets and a debug word."""
    from procgen2_amd import lib as pglib
    from test_episodes_gpu import Engine

    class ChainEngine(Engine):
        def reset(self, mask=None, seeds=None):
            self.v.reset(mask=mask, seeds=seeds)
            return self.rows()[0]

    eng = ChainEngine(game, n, SAME_STEP, cu.EPISODE_LIMIT, cu.EPISODE_RING, distribution_mode=mode, seed_base=cu.SEED_BASE)
    if debug:
        pglib.check(eng.v.L, eng.v.L.pgv_set_debug(eng.v._h, debug), "pgv_set_debug")
    return eng


@pytest.mark.parametrize("debug", (0, vp.NO_PREFETCH), ids=("default", "no-prefetch"))
@pytest.mark.parametrize("game,mode", sorted(cu.SAME_STEP_CASES))
def test_same_step_installs_deep_in_the_chain(game, mode, debug):
    """tests/test_chain.py test_same_step_play_tells_the_oracles_apart: in these runs the fresh-containers oracle differs in
    the frames the steps leave and in a terminal frame of the ring."""
    from test_episodes_gpu import check_step
    R, _, _ = cu.CASES[(game, mode)]
    n = cu.N
    eng = _episode_engine(game, n, mode, debug)
    model = EpisodeModel(game, n, SAME_STEP, cu.EPISODE_LIMIT, cu.EPISODE_RING, seed_base=cu.SEED_BASE, distribution_mode=mode)
    try:
        assert np.array_equal(eng.reset(), model.first_reset())
        fewest = cu.run_same_step(model, R, cu.SAME_STEP_CASES[(game, mode)], eng, check_step)
        assert fewest >= 3, fewest
    finally:
        eng.close(), model.close()


# ------------------------------------------------------------------------------------------------- records and snapshots

@pytest.mark.parametrize("game,mode", cu.RECORD_CASES)
def test_records_and_snapshots_keep_the_carried_counts(game, mode):
    from test_env_records_gpu import _engine
    R, P, cast = cu.CASES[(game, mode)]
    n = cu.N
    make = lambda: _engine(game, n, seed_base=cu.SEED_BASE, mode=mode)  # noqa: E731
    churned_eng, by_records, by_snapshot = make(), make(), make()
    ora = OracleVec(game, n, seed_base=cu.SEED_BASE, mode=mode)
    slot_of = (np.arange(n) * 37 + 11) % n  # oracle env i lies in slot slot_of[i] of the engine loaded from records
    env_in = np.argsort(slot_of)             # slot p holds oracle env env_in[p]
    try:
        _same_frames(churned_eng.reset(), ora.reset_obs(), "first reset")
        for e in (by_records, by_snapshot):
            e.reset()

        def each_reset(r, mask, seeds, obs):
            _same_frames(churned_eng.reset(mask=mask, seeds=seeds), obs, "churn round %d" % r)

        def after_churn():
            by_records.load_envs(churned_eng.save_envs(), slot_of)
            by_snapshot.load_state(churned_eng.save_state())
            _same_frames(by_records._fetch()[0], ora.obs[env_in], "frames of the loaded records")
            _same_frames(by_snapshot._fetch()[0], ora.obs, "frames of the loaded snapshot")
            cu.assert_same_rows("snapshot", by_snapshot, ora, n, "after the load")
            cu.assert_same_rows("records at shuffled slots", by_records, ora, n, "after the load", env_in)

        def each_step(t, a, obs, reward, done):
            _same_step("churned engine", churned_eng.step(a), t, obs, reward, done)
            if t < cu.churn_steps(R):  # the fresh engines are loaded after the churn
                return
            _same_step("snapshot", by_snapshot.step(a), t, obs, reward, done)
            _same_step("records at shuffled slots", by_records.step(a[env_in]), t, obs[env_in], reward[env_in], done[env_in])

        cu.run(ora, R, P, each_reset, each_step, after_churn, n=n, actions_of=cu.cast_actions(game, mode) if cast else None)
        cu.assert_same_rows("snapshot", by_snapshot, ora, n, "after the last step")
        cu.assert_same_rows("records at shuffled slots", by_records, ora, n, "after the last step", env_in)
    finally:
        ora.close()
        for e in (churned_eng, by_records, by_snapshot):
            e.close()


# ---------------------------------------------------------------------------------------------------- dropped assignments

@pytest.mark.parametrize("wait", cu.DROP_WAITS, ids=("built-ahead", "assigned-right-before"))
@pytest.mark.parametrize("game,mode", sorted(cu.DROP_CASES))
def test_dropped_assignments_go_back_to_the_carried_counts(game, mode, wait):
    """chain_util.run_dropped on the engine beside AssignModel, free mode: after the churn every env is assigned a level; a
    reset with seeds drops it in the even envs, which must go on with the counts they carried (chain_keep / chain_restore,
    pg_prefetch.h), a reset without seeds consumes it in the odd ones; outputs and level words after every call, state and
    tile rows of all envs at the end.  tests/test_chain.py: a model that gives the dropped envs fresh containers differs in
    at least 5 envs in this run."""
    from assign_util import AssignModel
    from oracle_util import assert_same_dump
    from test_assign_levels_gpu import Engine, Pair
    R, _, _ = cu.CASES[(game, mode)]
    n = cu.N
    eng = Engine(game, n, seed_base=cu.SEED_BASE, distribution_mode=mode)
    model = AssignModel(game, n, seed_base=cu.SEED_BASE, mode=mode)
    pair = Pair(eng, model)
    try:
        cu.run_dropped(pair, pair.assign, R, wait, cu.DROP_CASES[(game, mode)], check=pair.check)
        assert model.assigned_by_reset >= 25, model.assigned_by_reset
        for e in range(n):
            assert_same_dump(eng.state(e), model.state(e), "state of env %d after the last step" % e)
            assert_same_dump(eng.tiles(e), model.tiles(e), "tiles of env %d after the last step" % e)
    finally:
        eng.close(), model.close()
