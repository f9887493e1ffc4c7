"""The plans of tests/test_feature_scale_gpu.py hold on the oracle alone: the conditions that keep the full-batch tests of
the feature layers from passing vacuously (tests/feature_scale_util.py states them), established without a GPU — as
test_the_snapshot_plan_holds_on_the_oracle does for the snapshots.  Every run here is a whole batch without drawing."""
import numpy as np
import pytest

import feature_scale_util as fs
from episodes_util import synthetic_actions


def test_the_numpy_action_hash_is_the_oracles():
    for run_seed, step, n, offset in ((7, 0, 300, 0), (7, 26, 257, 69744), (0, 3, 64, 65504), (0xFFFFFFFF, 1000, 65, 0)):
        assert np.array_equal(fs.actions_of(run_seed, step, n, offset), synthetic_actions(run_seed, step, n, offset))


def test_the_slices_and_the_boundaries():
    """The rows named as holding bytes 2^31 and 2^32 do, and drawn slices lie around them."""
    # a second trip of the base loop (18 workgroups past 256), all four waves, a last workgroup of 113 envs: a ragged wave of 49
    assert fs.EP_BLOCKS == 274 and fs.EP_N % 256 == 113
    assert fs.straddlers(196608, 22000) == [10922, 21845] and fs.straddlers(98304, 44000) == [21845, 43690]
    assert fs.policy_slices("float32", 4, 22000)[2:] == [(10890, 64), (21813, 64)]
    assert fs.policy_slices("uint8", 8, 44000)[2:] == [(21813, 64), (43658, 64)]
    gray, n, T, slices = fs.HI_RGB
    assert fs.frame_straddlers(gray, n, T) == [(7, 20762), (15, 19525)]
    assert all(fs.slice_of(slices, env) is not None for _, env in fs.frame_straddlers(gray, n, T))
    gray, n, T, slices = fs.HI_GRAY
    assert fs.frame_straddlers(gray, n, T) == [] and 8 * n * 4096 == 1 << 31 and 16 * n * 4096 == 1 << 32
    for dtype, K, n in (("float32", 4, 22000), ("uint8", 8, 44000)):
        assert n * K * 3 * 4096 * (4 if dtype == "float32" else 1) > 1 << 32
    assert 22000 * 16 * 3 * 4096 > 1 << 32 and 65536 * 17 * 4096 > 1 << 32
    assert fs.straddlers(fs.GATHER_K * 3 * 4096 * 4, 22000) == [10922, 21845]  # the gather's output rows
    assert fs.GATHER_NAMED[1] <= 10922 < fs.GATHER_NAMED[1] + 64 and fs.GATHER_NAMED[2] <= 21845 < fs.GATHER_NAMED[2] + 64


@pytest.mark.parametrize("game,mode,limit,capacity", fs.EP_CASES)
def test_the_episode_plan_holds_on_the_oracle(game, mode, limit, capacity):
    """Every case reaches what feature_scale_util.EP_MEETS says it does — between them, all of: ends in more than 256
    workgroups in one call, a ring cut inside a workgroup past 64, more than n / 2 ends in a call, a call with fewer than 64."""
    m = fs.episode_model(game, mode, limit, capacity)
    ground = fs.EpisodeGround(fs.EP_N, capacity)
    spots = 0
    for t in range(fs.EP_CALLS):
        m.step(fs.actions_of(fs.RUN_SEED, t, fs.EP_N))
        ground.add(m.ended_env)
        spots += len(fs.ring_spots(m.ended_env, int(m.counts[1])))
    m.close()
    assert ground.met == fs.EP_MEETS[game, mode], ground.met
    assert spots >= 8
    assert set.union(*fs.EP_MEETS.values()) == {"many", "cut", "half", "few", "empty"}


@pytest.mark.parametrize("game,n", [("maze", 22000), ("maze", 44000), ("maze", 65536)])
def test_the_policy_and_history_plans_hold_on_the_oracle(game, n):
    """Inside every drawn slice of the policy runs (22 000 and 44 000 envs) and of the history runs (22 000 and 65 536) at
    least one env's episode ends and begins anew during the run and at least one's does not; the masked reset names a
    third of each."""
    runs = []
    if n in (22000, 44000):
        dtype, K = ("float32", 4) if n == 22000 else ("uint8", 8)
        runs.append((fs.policy_calls(n), fs.policy_slices(dtype, K, n)))
    if n in (22000, 65536):
        runs.append((fs.history_calls(), (fs.HI_RGB if n == 22000 else fs.HI_GRAY)[3]))
    for calls, slices in runs:
        fresh_on_steps = 0
        for (kind, _), m, fresh, _ in fs.run_logic(game, n, calls):
            fresh_on_steps += int(fresh.sum()) if kind == "step" else 0
            restarted = m.restarted.copy()
        assert fs.slices_restart_and_not(restarted, slices), [int(restarted[a:a + k].sum()) for a, k in slices]
        assert fresh_on_steps >= n // 50  # (restart flags are busy: maze ends episodes from the first step)


def test_the_gathers_entries():
    """At least 1 % and at most 50 % of the gather's pushes are not held; the named entries name envs of drawn slices and
    both kinds of push; both envs outside the batch are there."""
    gray, n, T, slices = fs.HI_RGB
    head = 1 + fs.HI_STEPS
    pushes, envs, named = fs.gather_entries(n, T, head, slices)
    assert pushes.size == envs.size == n and named.size == 256
    not_held = ~((pushes >= head - T) & (pushes < head) & (pushes >= 0))
    assert 0.01 * n <= not_held.sum() <= 0.5 * n, int(not_held.sum())
    assert all(fs.slice_of(slices, int(e)) is not None for e in envs[named])
    assert not_held[named].any() and not not_held[named].all()
    assert [int(envs[b]) for b, _ in fs.GATHER_OUTSIDE] == [-1, n]
    h = fs.held(pushes, envs, n, T, head)
    assert not h[[b for b, _ in fs.GATHER_OUTSIDE]].any() and np.array_equal(h[named], ~not_held[named])
    assert pushes.min() == head - T - 2 and pushes.max() == head


@pytest.mark.parametrize("game", list(fs.SEQ_GAMES))
def test_the_sequence_plan_holds_on_the_oracle(game):
    """In each game some env has its first done in the first third of a call and some in the last third, and maze and chaser
    have at least 256 dones inside a call (coinrun: 100) — chaser at T = 40, because it ends nothing before step 42."""
    T, ground = fs.SEQ_GAMES[game], fs.SequenceGround()
    m = fs.sequence_model(game)
    for call in range(2):
        m.sequence(fs.sequence_actions(call, T, fs.SEQ_N))
        ground.add(m, T)
    m.close()
    assert ground.holds(game), (ground.early, ground.late, ground.inside)


def test_the_index_lists_of_the_symbolic_calls():
    idx, sample = fs.symbolic_indices(), fs.symbolic_sample()
    assert idx.size == fs.SY_B == 100003 and sample.size == fs.SY_SAMPLE and set(fs.SY_EDGES) <= set(sample.tolist())
    inside = (idx >= 0) & (idx < fs.SY_N)
    assert (~inside).sum() == 4 and sorted(idx[~inside].tolist()) == [-2 ** 31, -1, fs.SY_N, 2 ** 31 - 1]
    assert set(fs.SY_EDGES) <= set(idx.tolist()) and np.unique(idx[inside]).size < inside.sum()  # (repeats)


def test_the_levels_plan_holds_on_the_oracle():
    """The levels of 65 536 oracle mazes after 5 steps, every 97th row spoiled: every refusal status occurs at least 10 times
    and at least 90 % of the rows are installed (an env whose mouse stands on the cheese — done, its reset pending — is refused)."""
    from custom_levels_util import HARD, SIDE, levels_of_dumps, oracle_dumps, status_of
    from oracle_util import OracleVec
    n, side = fs.LV_N, SIDE[HARD]
    o = OracleVec("maze", n, seed_base=fs.LV_SEEDS[0], render=False, threads=fs.host_threads())
    for t in range(fs.LV_A_STEPS):
        o.step(fs.actions_of(fs.RUN_SEED, t, n))
    levels, indices = fs.spoil_levels(levels_of_dumps(*oracle_dumps(o), side), n, side)
    o.close()
    status = status_of(levels, indices, n, side)
    assert fs.levels_plan_holds(status), np.bincount(status, minlength=6)
