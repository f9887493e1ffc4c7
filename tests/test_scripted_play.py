"""The CPU half of tests/test_scripted_play_gpu.py: the scripted agents of tests/scripted_play_util.py play all seven games
(bossfight, chaser, climber, caveflyer, coinrun, jumper, maze) on the oracle alone, frames off, and every floor the GPU half
leans on is asserted here — wins, the
boss's phases 0 to 5 and its damaged state, a win and a death in one step, cleared boards and eaten enemies, levels won with
three coins and more, caveflyer's destroyed targets, more than one and two gangs of 8 live bullets, the full ring of 32, more
draws than the render wave has lanes and a ship turned past a full turn; coinrun's 100 wins, its deaths in lava, by saw and
by mob, a quarter of the env-steps past the middle of the level, crates stood on and dropped through, 60 of 65 envs three
levels deep and one eight; jumper's wins, spike deaths (none in memory mode: it has no spikes), 5 000 env-steps without a
jump left, an env 20 cells from its start and one whose compass saw five octants in memory mode; maze's median env ending
twice as many episodes as under random play — so the GPU tests are known not to be vacuous before
a GPU is touched.  The counts are printed (pytest -s).

chaser in extreme mode falls back: no agent here clears a 19 x 19 board with five enemies in a run of a length the suite
can afford (the agent eats at most one cell in five steps, so its 190 or so points and orbs take 950 steps at the least; the
best of 65 envs stands at 79 % after 1 250 steps, at 89 % after 1 500 and dies at 95 %; none clears a board in 2 500).  Its
cleared-board floor is therefore an episode that ate at least 85 % of its board's points and orbs, reached at step 1 429.  Every
other floor, and every floor of chaser's easy and hard modes (2 and 1 cleared boards), stands as it is.
"""
import numpy as np
import pytest

import scripted_play_util as sp
import variant_paths_util as vp
from episodes_util import SAME_STEP, EpisodeModel
from oracle_util import OracleVec
from test_modes import EASY, EXTREME, HARD, MEMORY


def test_the_protocol_is_what_the_file_says():
    assert sp.N >= 65 and sp.N % 64 != 0
    assert len(sp.PAIRS) == 18 and set(sp.PAIRS) == set(sp.STEPS) and {g for g, _ in sp.PAIRS} == set(sp.POLICIES)
    assert sp.ATE_85_INSTEAD == {("chaser", EXTREME)}
    for game, mode in sp.PAIRS:
        c = sp.columns(game, mode)
        assert (c.width - c.fixed) % max(1, c.record) == 0 and "agent_x" in c.f
        assert all(least > 0 for least in sp.floors(game, mode).values())
    for mode in (EASY, HARD, MEMORY):
        # caveflyer's overflow predicate is spelled from the row's own numbers: 10 puff slots, a ring of 32 bullets, one
        # record a thing but for the ship, and the 64 lanes the render wave has for them and the ship
        c = sp.columns("caveflyer", mode)
        assert len(c.slots("puff", "life")) == 10 and len(c.slots("shot", "frame")) == 32 and sp.LANES == 64
        assert sp.cave_draws(c, 0, 0) == 11 and sp.cave_draws(c, 37, 17) == 65
        assert c.unlisted == (1,) and c.fixed == c.f["n_things"] + 1 + 3 * (32 + 10)
        counter = sp.Counter("caveflyer", mode, 3)

        class Rows:  # three made-up envs: 37 live sprites of 40 things, and 16, 17 and 32 bullets
            states = np.zeros((3, c.width), np.float32)
        Rows.states[:, c.f["n_things"]] = 40
        Rows.states[:, c.f["s_count"]] = (16, 17, 32)
        Rows.states[:, c.fixed + c.r["alive"]:c.fixed + 37 * c.record:c.record] = 1
        assert [c.count(row) for row in Rows.states] == [39] * 3 and c.records(Rows.states[0])[:, c.r["alive"]].sum() == 37
        assert counter.caveflyer_overflow(Rows).tolist() == [False, True, True]
        Rows.states[0, c.f["n_things"]] = 1  # (the goal alone: the ship is not among the things yet)
        assert c.count(Rows.states[0]) == 1


@pytest.mark.parametrize("game,mode", sp.PAIRS)
def test_scripted_play_covers(game, mode):
    counts = sp.run_on_oracle(game, mode)
    print("scripted play: %s mode %d, %d envs, %d steps: %r" % (game, mode, sp.N, sp.STEPS[(game, mode)], counts))
    sp.assert_covers(game, mode, counts)


@pytest.mark.parametrize("game,mode", sp.PAIRS)
def test_random_play_does_not_cover(game, mode):
    """The floors ask for something: the variant-path protocol's actions, over its 200 steps at this batch size, miss them."""
    counts = sp.run_on_oracle(game, mode, steps=vp.steps_of(game, mode), actions_of=vp.actions)
    print("random play: %s mode %d, %d envs, %d steps: %r" % (game, mode, sp.N, vp.steps_of(game, mode), counts))
    with pytest.raises(AssertionError):
        sp.assert_covers(game, mode, counts)
    if game in ("coinrun", "jumper", "maze"):
        _random_play_misses(game, mode, counts)
        return
    if game != "caveflyer":
        assert counts["wins"] == 0
        return
    # caveflyer: random play does reach the goal.  What it misses is a second gang of bullets (at most 8 are live), with it
    # every floor that counts them, a full turn, and in memory mode a frame with more draws than the render wave has lanes
    floors = sp.floors(game, mode)
    assert counts["wins"] > 0 and counts["most_shots"] <= 8 and counts["steps_over_8"] == 0 and counts["steps_over_16"] == 0
    assert counts["most_turn"] < sp.FULL_TURN and counts["ring_full_steps"] == 0
    assert counts["overflow_steps"] == 0 and (mode == MEMORY) == ("overflow_steps" in floors)


def _random_play_misses(game, mode, counts):
    """coinrun, jumper and maze: random play does win.  What it misses is named here, count by count."""
    floors = sp.floors(game, mode)
    if game == "coinrun":  # no death in lava, no env past its first auto-reset, next to no frame of a level's last tenth
        missed = ("wins", "deaths", "lava_deaths", "envs_with_3_ends", "most_ends", "deep_starts", "drop_steps")
        assert counts["lava_deaths"] == 0 and counts["envs_with_3_ends"] == 0 and counts["most_ends"] <= 1 and counts["deep_starts"] == 0
        assert 4 * counts["past_half"] < counts["env_steps"] and 20 * counts["past_09"] < counts["env_steps"]
    elif game == "jumper":
        missed = ("wins", "most_ends")
        if mode == MEMORY:  # one episode ends in 400 steps, and no env's needle leaves half the compass
            missed += ("most_octants_in_an_env",)
            assert counts["ends"] <= 1 and counts["deaths"] == 0
    else:
        missed = ("median_ends", "deep_starts")
        assert counts["median_ends"] == sp.RANDOM_MAZE_MEDIAN[mode][1]
        short = sp.run_on_oracle(game, mode, actions_of=vp.actions)
        assert short["median_ends"] == sp.RANDOM_MAZE_MEDIAN[mode][0] and short["deep_starts"] == 0
    for name in missed:
        assert counts[name] < floors[name], (game, mode, name, counts[name], floors[name])


@pytest.mark.parametrize("game", sp.GAMES)
def test_same_step_protocol_ends_in_wins(game):
    """The same-step case of the GPU half on the model alone: at least one winning episode whose terminal frame is kept."""
    model = EpisodeModel(game, sp.N, SAME_STEP, 0, sp.SAME_STEP_RING, render=False)
    model.first_reset()
    counts = sp.run_same_step(game, model)
    model.close()
    print("scripted play, same-step: %s, %d envs, %d steps: %r" % (game, sp.N, sp.STEPS[(game, sp.DEFAULT_MODE[game])], counts))
    sp.assert_same_step_covers(game, counts)


@pytest.mark.parametrize("game", sp.GAMES)
def test_policies_are_functions_of_what_they_are_given(game):
    """The same dumps, step and generator state give the same actions, the dumps are left as they were, and every action is
    one the games know."""
    mode = 1
    ora = OracleVec(game, 9, seed_base=sp.SEED_BASE, render=False, mode=mode)
    c = sp.columns(game, mode)
    for s in range(40):
        d = sp.Dumps(ora, c)
        kept = d.states.copy(), d.tiles.copy()
        a = sp.choose_actions(game, mode, d, s, np.random.default_rng(s))
        b = sp.choose_actions(game, mode, d, s, np.random.default_rng(s))
        assert np.array_equal(a, b) and a.dtype == np.int32 and ((a >= 0) & (a < 15)).all()
        assert np.array_equal(d.states.view(np.uint32), kept[0].view(np.uint32)) and np.array_equal(d.tiles, kept[1])
        for e in (0, 8):  # the dumps the policies read are the oracle's own
            st = ora.state(e)
            assert np.array_equal(d.states[e, :st.size].view(np.uint32), st.view(np.uint32)) and not d.states[e, st.size:].any()
            assert np.array_equal(d.tiles[e, :c.cells], ora.tiles(e))
        ora.step(a)
    ora.close()
