"""The CPU half of tests/test_variant_paths_gpu.py and of the per-variant sequence and episode tests: their protocols run on
the oracle alone, and every floor the GPU tests lean on is asserted here — auto-resets served, maze envs ending at the step
cap together, resets inside a sequence, chaser's late-pass rows, every env ending twice under the episode limit — so the GPU
tests are known not to be vacuous before a GPU is touched.  The counts are printed (pytest -s shows them).  The `mode` forms
of SequenceModel and EpisodeModel are held to plain drawn oracle steps in two pairs, as tests/test_sequence.py and
tests/test_episodes.py hold the default forms.
"""
import numpy as np
import pytest

import variant_paths_util as vp
from episodes_util import SAME_STEP, EpisodeModel, synthetic_actions
from oracle_util import OracleVec
from sequence_util import CHASER_LATE_ROWS, SequenceModel, chaser_late_rows, count_protocol, protocol_calls
from test_modes import EXTREME, MEMORY, NON_DEFAULT

MODEL_PAIRS = [("chaser", EXTREME), ("jumper", MEMORY)]


def test_the_pairs_are_the_engines_table():
    assert len(vp.PAIRS) == 18 and len(NON_DEFAULT) == 11 and set(NON_DEFAULT) < set(vp.PAIRS)
    assert vp.N == 131 and all(vp.N % k for k in range(2, vp.N))  # prime: a multiple of no gang, block or group size
    assert max(vp.DUMP_ENVS) == vp.N - 1
    for game, mode in vp.PAIRS:
        assert set(vp.paths(game)) <= set(vp.PATH_NAMES) and vp.paths(game)[:4] == [0, 1, 1 << 8, 1 << 21]
        assert max(vp.dump_after(game, mode)) == vp.steps_of(game, mode) - 1 and set(vp.dump_after(game, mode)) >= {0, 59, 62, 111}


@pytest.mark.parametrize("game,mode", vp.PAIRS)
def test_lockstep_protocol_serves_resets(game, mode):
    """Protocol A on the oracle: at least 10 auto-resets in every case; in maze at least 30 envs end at the cap in one step."""
    masked = []
    ends, cap_ends = vp.run_on_oracle(game, mode, each_reset=lambda s, ora, mask, seeds, obs: masked.append((s, int(mask.sum()), seeds is not None)))
    print("variant paths: %s mode %d, %d steps: %d auto-resets, at most %d in one step at the cap" % (game, mode, vp.steps_of(game, mode), ends, cap_ends))
    assert [(s, k) for s, _, k in masked] == [(60, False), (vp.second_reset_after(game), False), (110, True)] and all(m > 20 for _, m, _ in masked)
    vp.assert_covers(game, mode, ends, cap_ends)


def test_masked_resets_are_the_ones_the_protocol_names():
    for game in ("coinrun", "maze"):
        second = 63 if game == "maze" else 61
        mask, seeds = vp.masked_reset_after(game, 110)
        assert seeds.dtype == np.int32 and seeds.min() == -5 and list(np.nonzero(mask)[0][:3]) == [2, 7, 12] and seeds[2] == 9
        for s in (60, second):
            mask, none = vp.masked_reset_after(game, s)
            assert none is None and np.array_equal(np.nonzero(mask)[0], np.arange((-s) % 3, vp.N, 3))
        assert all(vp.masked_reset_after(game, s) is None for s in range(520) if s not in (60, second, 110))


@pytest.mark.parametrize("game,mode", NON_DEFAULT)
def test_small_batches_are_what_the_protocol_says(game, mode):
    """test_variants_at_one_and_65_envs on the oracle: a one-env and a 65-env oracle of every variant run the 80 steps and
    the masked reset of env 0."""
    for n in vp.SMALL_NS:
        ora = OracleVec(game, n, seed_base=vp.SEED_BASE, render=False, mode=mode)
        ends = 0
        for s in range(vp.SMALL_STEPS):
            _, _, done = ora.step(vp.actions(s, n))
            ends += int((done != 0).sum())
            if s == vp.SMALL_RESET_AFTER:
                ora.reset(mask=(np.arange(n) == 0).astype(np.uint8))
        print("variant paths: %s mode %d, %d envs, %d steps: %d auto-resets" % (game, mode, n, vp.SMALL_STEPS, ends))
        ora.close()


@pytest.mark.parametrize("game,mode", NON_DEFAULT)
def test_sequence_protocol_resets_inside_sequences(game, mode):
    """Protocol B (sequences) on the oracle: at least 10 resets fall inside a sequence in every non-default pair."""
    inside, third, every = count_protocol(game, mode)
    print("sequences: %s mode %d: %d resets inside a sequence; rows reset in a call's last sub-step: %d in every third call, %d in all"
          % (game, mode, inside, third, every))
    assert inside >= 10, inside
    if game == "chaser":
        assert CHASER_LATE_ROWS[mode] == (third, every)
        count, every_call, floor = chaser_late_rows(mode)
        assert count >= 6 and floor * 2 >= count and floor >= 3, (count, every_call, floor)


def test_chaser_late_rows_default_mode():
    inside, third, every = count_protocol("chaser", 0)
    assert CHASER_LATE_ROWS[0] == (third, every) and chaser_late_rows(0) == (8, False, 5)


@pytest.mark.parametrize("game,mode", NON_DEFAULT)
def test_episode_limit_case_ends_every_env_twice(game, mode):
    """Protocol B (episodes) on the model: truncations, a ring overflow, and every env ends at least twice in the 70 steps."""
    model = EpisodeModel(game, vp.EPISODE_N, SAME_STEP, vp.EPISODE_LIMIT, vp.EPISODE_RING, distribution_mode=mode, render=False)
    model.first_reset(), model.reset()
    got = vp.run_limit_case(model)
    print("episodes: %s mode %d: %d terminated, %d truncated, %d steps overflow the ring, every env ends at least %d times" % ((game, mode) + got))
    vp.assert_limit_case_covers(*got)
    model.close()


@pytest.mark.parametrize("game,mode", MODEL_PAIRS)
def test_sequence_model_in_a_mode_equals_drawn_oracle_steps(game, mode):
    """SequenceModel(mode=) against a second oracle of that mode that draws every step (tests/test_sequence.py
    test_model_equals_drawn_oracle_steps): rows, the drawn frame of every call that drew one, the state dumps at the end."""
    n = 96
    m, o = SequenceModel(game, n, mode=mode), OracleVec(game, n, mode=mode)
    assert np.array_equal(m.reset(), o.reset())
    inside = 0
    for k, (t, actions) in enumerate(protocol_calls(n)):
        draw = k % 3 != 2
        m.sequence(actions, draw_last=draw)
        for s in range(len(actions)):
            obs, reward, done = o.step(actions[s])
            assert np.array_equal(m.rewards[s].view(np.uint32), reward.view(np.uint32)) and np.array_equal(m.dones[s], done), (t, s)
        assert np.array_equal(m.engine_reward.view(np.uint32), reward.view(np.uint32)) and np.array_equal(m.engine_done, done)
        if draw:
            assert np.array_equal(m.obs, obs), "the drawn frame of the call at step %d" % t
        inside += int(m.dones[:-1].any(axis=0).sum())
    assert inside >= 3, inside
    for i in range(n):
        assert m.o.state(i).size == o.state(i).size
        assert np.array_equal(m.o.state(i).view(np.uint32), o.state(i).view(np.uint32)), "state of env %d" % i
    # the mode is the one asked for: another world than the default's
    d = OracleVec(game, 1, render=False)
    assert d.tiles(0).size != o.tiles(0).size
    m.close(), o.close(), d.close()


@pytest.mark.parametrize("game,mode", MODEL_PAIRS)
def test_episode_model_in_a_mode_counts_as_the_callers_loop_does(game, mode):
    """EpisodeModel(distribution_mode=) against a loop written out by hand over a second oracle of that mode
    (tests/test_episodes.py test_model_counts_episodes_as_the_callers_loop_does): same-step with a limit of 9, 60 steps."""
    n, T = 12, 9
    m = EpisodeModel(game, n, SAME_STEP, max_episode_steps=T, final_capacity=3, distribution_mode=mode)
    o = OracleVec(game, n, mode=mode)
    assert np.array_equal(m.first_reset(), o.reset_obs())
    length, ret = np.zeros(n, np.int64), np.zeros(n, np.float32)
    truncated = 0
    for t in range(60):
        a = synthetic_actions(7, t, n)
        m.step(a)
        obs, reward, done = o.step(a)
        length += 1
        ret = (ret + reward).astype(np.float32)
        ended = (done != 0) | (length == T)
        assert np.array_equal(m.ended != 0, ended) and np.array_equal(m.truncated != 0, ended & (done == 0))
        where = np.nonzero(ended)[0]
        assert np.array_equal(m.ended_env, where) and np.array_equal(m.ended_length, length[where])
        assert np.array_equal(m.ended_return.view(np.uint32), ret[where].view(np.uint32))
        assert np.array_equal(m.final_obs, obs[where[:3]]) and list(m.counts) == [where.size, min(where.size, 3)]
        truncated += int((ended & (done == 0)).sum())
        if ended.any():
            o.reset(mask=ended.astype(np.uint8))
            length[ended], ret[ended] = 0, 0
        assert np.array_equal(m.obs, o.obs)
    assert truncated > 0 and m.longest <= T
    for i in range(n):
        assert np.array_equal(m.o.state(i).view(np.uint32), o.state(i).view(np.uint32)), "state of env %d" % i
    m.close(), o.close()
