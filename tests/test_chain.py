"""The CPU half of tests/test_chain_gpu.py: the protocol "churn, then play" (tests/chain_util.py) on the oracle alone, beside
the WRONG oracle that starts every level with fresh containers (OracleVec.set_fresh_containers).  For every case the GPU
half keeps: the two oracles differ in at least 20 env-steps spread over at least 5 envs, the churn leaves the median env at
least 20 levels deep, and reseeding resets were among it; the same for the one-env, the same-step and the
dropped-assignment cases, each by its own run — so the GPU tests are known not to be vacuous before a GPU is touched.  The counts are printed (pytest -s shows them); tools/chain_census.py prints them for every (game, mode) pair,
profiles/chain/census.md keeps that table.
"""
import numpy as np
import pytest

import chain_util as cu
import variant_paths_util as vp
from oracle_util import OracleVec


def test_the_switch_leaves_the_levels_as_they_are():
    """Two oracles, one with the switch on: the first levels (made before it was set) are the same, and through the churn
    the tile maps — so the rng streams too — stay the same: the switch touches the containers alone."""
    game, n = "chaser", 8
    a, b = OracleVec(game, n, seed_base=cu.SEED_BASE), OracleVec(game, n, seed_base=cu.SEED_BASE)
    b.set_fresh_containers(True)
    assert np.array_equal(a.reset_obs(), b.reset_obs())
    for r in range(12):
        mask, seeds, _ = cu.churn_round(r, n)
        a.reset(mask=mask, seeds=seeds), b.reset(mask=mask, seeds=seeds)
        for e in range(n):
            assert np.array_equal(a.tiles(e), b.tiles(e)), (r, e)
    a.close(), b.close()


def test_the_churn_is_the_one_the_protocol_names():
    n = cu.N
    for r in range(8):
        mask, seeds, then_step = cu.churn_round(r)
        if r % 4 == 3:
            assert then_step and seeds.dtype == np.int32 and list(np.nonzero(mask)[0][:3]) == [2, 7, 12]
            assert seeds[2] == 14 - 40 - r < 0 < seeds[np.nonzero(mask)[0][-1]]
        else:
            assert seeds is None and not then_step and np.array_equal(np.nonzero(mask)[0], np.nonzero((np.arange(n) + r) % 3)[0])
    assert cu.N == 65 and cu.SMALL_N == 1 and cu.churn_steps(44) == 11
    assert set(cu.RECORD_CASES) <= set(cu.CASES) and set(cu.SMALL_CASES) <= set(cu.CASES) and set(cu.SAME_STEP_CASES) <= set(cu.CASES)
    assert all((g, m) in vp.PAIRS for g, m in cu.CASES)


@pytest.mark.parametrize("game,mode", cu.cases())
def test_fresh_containers_part_from_the_good_oracle_within_the_run(game, mode):
    R, P, cast = cu.CASES[(game, mode)]
    w, churned, end, ends = cu.compare_oracles(game, mode, R, P, cast=cast)
    print("chain: %s mode %d, R = %d, P = %d%s: median depth %g after the churn (%g at the end), %d reseeding resets, %d auto-resets; "
          "the fresh-containers oracle differs in %d env-steps over %d envs (frames %d, state rows %d, rewards %d, dones %d), first at %s; "
          "20 in 5 envs met at %s" % (game, mode, R, P, ", the cast plays" if cast else "", churned.median(), end.median(), churned.reseeding,
                                      ends, w.env_steps, w.envs, w.count["frames"], w.count["state"], w.count["reward"], w.count["done"],
                                      w.first, w.met_at))
    assert w.env_steps >= cu.MIN_WITNESS and w.envs >= cu.MIN_ENVS, (w.env_steps, w.envs)
    assert churned.median() >= cu.MIN_DEPTH, churned.median()
    assert churned.reseeding == R // 4 >= 5


@pytest.mark.parametrize("game,mode", sorted(cu.SMALL_CASES))
def test_the_one_env_case_is_a_witness(game, mode):
    """The one-env batch at its env_offset is a witness env of the 65 over again: it differs from the fresh-containers oracle
    at least once, and chaser's is one of the reseeded envs."""
    R, P, cast = cu.CASES[(game, mode)]
    offset = cu.SMALL_CASES[(game, mode)]
    assert not cast
    w, churned, end, ends = cu.compare_oracles(game, mode, R, P, n=1, env_offset=offset)
    print("chain: %s mode %d, one env at offset %d: %d levels deep, differs in %d steps, first at %s" % (game, mode, offset, churned.depth[0], w.env_steps, w.first))
    assert w.env_steps >= 1 and churned.depth[0] >= cu.MIN_DEPTH
    assert game != "chaser" or (offset % 5 == 2 and churned.depth[0] == 33)


@pytest.mark.parametrize("game,mode", sorted(cu.SAME_STEP_CASES))
def test_same_step_play_tells_the_oracles_apart(game, mode):
    """The same-step protocol on the model over the good and over the fresh-containers oracle: the frames the steps leave
    differ by the coverage condition, a terminal frame of the ring differs too, and every env ends three times."""
    R, _, _ = cu.CASES[(game, mode)]
    w, terminal, fewest = cu.compare_same_step(game, mode, R, cu.SAME_STEP_CASES[(game, mode)])
    print("chain: %s mode %d, same-step: %d env-steps over %d envs differ (met at %s), terminal frames at steps %s, every env ends %d times"
          % (game, mode, w.env_steps, w.envs, w.met_at, terminal, fewest))
    assert w.env_steps >= cu.MIN_WITNESS and w.envs >= cu.MIN_ENVS, (w.env_steps, w.envs)
    assert len(terminal) >= 1 and fewest >= 3, (terminal, fewest)


@pytest.mark.parametrize("wait", cu.DROP_WAITS)
@pytest.mark.parametrize("game,mode", sorted(cu.DROP_CASES))
def test_dropped_assignments_need_the_carried_counts(game, mode, wait):
    """The dropped-assignment protocol on AssignModel and on a model whose envs with a dropped assignment got fresh
    containers at the seeded reset: their frames differ in at least 5 envs over the play, all of them envs whose assignment
    was dropped; the other half consumed theirs."""
    R, _, _ = cu.CASES[(game, mode)]
    w, dropped, consumed = cu.compare_dropped(game, mode, R, wait, cu.DROP_CASES[(game, mode)])
    print("chain: %s mode %d, dropped assignments, wait %d: %d dropped, %d consumed by the reset without seeds; the wrong model differs in %d "
          "env-steps over %d envs (%s), 20 in 5 envs met at %s" % (game, mode, wait, len(dropped), consumed, w.env_steps, w.envs,
                                                                  [int(e) for e in np.nonzero(w.any)[0]], w.met_at))
    assert w.envs >= cu.MIN_DROP_ENVS, (w.envs, w.env_steps)
    assert set(np.nonzero(w.any)[0]) <= set(dropped) and len(dropped) >= 30 and consumed >= 25, (len(dropped), consumed)
