"""Play to win: the HIP engine against the oracle on the games' winning and late-game paths (need an MI355X).

Every other lock-step test is driven by random or one-key action streams, and those lose: bossfight never leaves its second
phase, no chaser board is cleared, climber picks up two or three coins in a run, coinrun stays in the first half of its
levels and no env of it goes past its first auto-reset.  Here the scripted agents of tests/scripted_play_util.py play all seven
games (bossfight, chaser, climber, caveflyer, coinrun, jumper, maze) on the oracle — reading the oracle's dumps, never the
engine's — and their actions go to the engine under its default path AND every alternate path behind pgv_set_debug, side by
side: dones, reward bit patterns and every observation byte after every step, and state_obs / tile_obs rows against the
oracle's dumps wherever an env is in a state random play does not visit (bossfight: the shield down, hp 0, explosions, phase
4 and later; chaser: an enemy just eaten under an orb's timer; climber: a coin just destroyed, and the step after;
caveflyer: a target just destroyed, and the step after, more than 16 live bullets — three and four trips of the bullet loop's
gangs of 8 — the full ring of 32, and more draws than the render wave has lanes, which is where the complete render path and
the frames the pre-pass hands back part from the default; coinrun: the first step of an env's fourth and later level — a
level deep in the generator's chain installed under prefetch, under generation inside the step and under every renderer at
once — a crate dropped through, and the step after, an env grounded on a crate, past 0.9 of the way to the coin, with lava
within 8 columns; jumper: the first step of a fourth and later level, in memory mode an agent more than 15 cells from where
its episode began, no jump left with the timer running; maze: the first step of a sixth and later level).  One case holds
the batched human-size frames of caveflyer's memory mode to the oracle in those last two states of its, one more those of
coinrun late in its levels and of jumper's memory mode far from the start.  One
case a game runs the agents through step_episodes in same-step mode against the model of tests/episodes_util.py: the
returns, lengths and terminal frames of winning episodes.  The floors of tests/test_scripted_play.py are asserted again on
the runs made here.

chaser in extreme mode falls back, as tests/test_scripted_play.py explains: no board is cleared in its 1 450 steps (nor in
2 500), so its cleared-board floor is one episode that ate at least 85 % of its board's points and orbs (the best reaches
87.6 % inside the run).  Every other floor stands as the other modes have it.
"""
import numpy as np
import pytest

import scripted_play_util as sp
import variant_paths_util as vp
from engine_util import EngineVec
from episodes_util import SAME_STEP, EpisodeModel
from oracle_util import OBS_BYTES, assert_same_dump, oracle, oracle_state
from procgen2_amd import lib as pglib
from test_episodes_gpu import Engine as EpisodeEngine
from test_episodes_gpu import check_step
from test_frames_batch_gpu import _oracle_step, assert_frame, frames_host, oracle_frame
from test_modes import HARD, MEMORY
from test_parity_gpu import _host_threads

pytestmark = pytest.mark.gpu


class PathEngine:
    """ProcgenVecEnv under one pgv_set_debug word, driven with host arrays and read back as numpy."""

    def __init__(self, game, mode, debug):
        import torch
        from procgen2_amd.vec_env import ProcgenVecEnv
        self.torch, self.name = torch, vp.PATH_NAMES[debug]
        self.v = ProcgenVecEnv(game, sp.N, seed_base=sp.SEED_BASE, distribution_mode=mode)
        assert self.v.L.pgv_mode(self.v._h) == mode
        if debug:
            pglib.check(self.v.L, self.v.L.pgv_set_debug(self.v._h, debug), "pgv_set_debug")

    def rows(self):
        v = self.v
        return v.obs.reshape(sp.N, OBS_BYTES).cpu().numpy(), v.reward.cpu().numpy(), v.done.cpu().numpy()

    def reset(self):
        self.v.reset()
        return self.rows()[0]

    def step(self, actions):
        self.v.step(self.torch.as_tensor(actions))
        return self.rows()

    def symbolic(self, envs):
        idx = np.asarray(envs, np.int32)
        rows, lengths = self.v.state_obs(idx)
        return rows.cpu().numpy(), lengths.cpu().numpy(), self.v.tile_obs(idx).cpu().numpy()

    def close(self):
        self.v.close()


def _same_frames(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        first = np.nonzero(got[bad[0]] != want[bad[0]])[0]
        raise AssertionError("%s: obs differ in %d envs (first env %d, %d bytes, the first at %d: %d, the oracle's %d)" %
                             (what, bad.size, bad[0], first.size, first[0], got[bad[0], first[0]], want[bad[0], first[0]]))


def _same_rows(eng, a, s, obs, reward, done):
    oe, re_, de = eng.step(a)
    what = "%s, step %d" % (eng.name, s)
    if not np.array_equal(de, done):
        raise AssertionError("%s: done differs, first env %d" % (what, np.nonzero(de != done)[0][0]))
    if not np.array_equal(re_.view(np.uint32), reward.view(np.uint32)):
        e = np.nonzero(re_.view(np.uint32) != reward.view(np.uint32))[0][0]
        raise AssertionError("%s: reward bits differ, first env %d: %r, the oracle's %r" % (what, e, re_[e], reward[e]))
    _same_frames(oe, obs, what)


def _same_symbolic(eng, dumps, envs, s):
    """state_obs / tile_obs rows of `envs` against the oracle's dumps after the step (the ones the event counter read)."""
    rows, lengths, tiles = eng.symbolic(envs)
    cells = eng.v.state_layout.cells
    for k, e in enumerate(envs):
        what = "%s, step %d: %%s of env %d" % (eng.name, s, e)
        assert_same_dump(rows[k, :lengths[k]], dumps.state(e), what % "state row")
        assert not rows[k, lengths[k]:].view(np.uint32).any(), what % "the row behind the state"
        assert_same_dump(tiles[k], dumps.tiles[e, :cells], what % "tile row")


@pytest.mark.parametrize("game,mode", sp.PAIRS)
def test_every_path_matches_the_oracle_under_scripted_play(game, mode):
    engines = [PathEngine(game, mode, debug) for debug in vp.paths(game)]
    compared = [0]

    def at_start(ora):
        for eng in engines:
            _same_frames(eng.reset(), ora.reset_obs(), "%s, first reset" % eng.name)

    def each_step(s, ora, a, obs, reward, done, counter):
        for eng in engines:
            _same_rows(eng, a, s, obs, reward, done)
            if counter.rare:
                _same_symbolic(eng, counter.after, counter.rare, s)
        compared[0] += len(counter.rare)

    try:
        counts = sp.run_on_oracle(game, mode, each_step, at_start, render=True, threads=_host_threads())
        print("scripted play: %s mode %d, %d envs, %d steps, %d paths: %r; state and tile rows of %d envs in rare states" %
              (game, mode, sp.N, sp.STEPS[(game, mode)], len(engines), counts, compared[0]))
        sp.assert_covers(game, mode, counts)
        assert compared[0] >= 20, compared[0]
    finally:
        for eng in engines:
            eng.close()


class _Played(Exception):
    """Ends a run of the protocol before its last step."""


def test_human_size_frames_with_a_full_ring():
    """caveflyer's three renderers share one draw list, and under the cast it is longer than a wavefront with bullets behind
    the sprites.  Memory mode, one default-path engine beside the oracle: at the first step after which at least four envs
    draw more than 64 things, and at the first after which one holds all 32 bullets, the batched human-size frames of up to
    four such envs — 128 x 128, and one 192 x 96 — against pgo_render_frame, byte for byte.  The oracle's frame comes from a
    single env brought to the same state by the same actions (its state dump is held to the protocol's own first)."""
    game, mode = "caveflyer", MEMORY
    L = oracle()
    c = sp.columns(game, mode)
    eng = EngineVec(game, sp.N, seed_base=sp.SEED_BASE, mode=mode)
    history, seen = [], {}

    def single(env):
        h = L.pgo_make_mode(game.encode(), sp.SEED_BASE + env, 1, mode)
        L.pgo_reset(h, 0, 0)
        pending = [False]
        for a in history:
            _oracle_step(L, [h], pending, a[env:env + 1])
        return h

    def frames_of(envs, dumps, what):
        for k, (w, h) in enumerate(((128, 128), (192, 96))):
            chosen = envs[:4] if k == 0 else envs[:1]
            got = frames_host(eng, chosen, w, h)
            for j, env in enumerate(chosen):
                handle = single(env)
                try:
                    assert_same_dump(oracle_state(handle), dumps.state(env), "%s: the single env %d" % (what, env))
                    assert_frame(got[j], oracle_frame(L, handle, w, h), "%s: env %d, %dx%d" % (what, env, w, h))
                finally:
                    L.pgo_close(handle)

    def at_start(ora):
        _same_frames(eng.reset(), ora.reset_obs(), "first reset")

    def each_step(s, ora, a, obs, reward, done, counter):
        history.append(a.copy())
        oe, re_, de = eng.step(a)
        assert np.array_equal(de, done) and np.array_equal(re_.view(np.uint32), reward.view(np.uint32)), s
        _same_frames(oe, obs, "step %d" % s)
        after = counter.after
        shots = after.states[:, c.f["s_count"]].astype(int)
        over, full = np.nonzero(counter.caveflyer_overflow(after))[0], np.nonzero(shots == len(c.slots("shot", "frame")))[0]
        if "overflow" not in seen and over.size >= 4:
            seen["overflow"] = (s, over.size, int(shots[over].max()))
            frames_of(over.tolist(), after, "step %d, more than %d draws" % (s, sp.LANES))
        if "full ring" not in seen and full.size >= 1:
            seen["full ring"] = (s, full.size, int(shots[full].max()))
            frames_of(full.tolist(), after, "step %d, a full ring" % s)
        if len(seen) == 2:
            raise _Played

    try:
        with pytest.raises(_Played):  # both states are met inside the protocol's run: tests/test_scripted_play.py's floors
            sp.run_on_oracle(game, mode, each_step, at_start, render=True, threads=_host_threads())
        print("human-size frames: caveflyer mode %d, (step, envs in the state, most bullets): %r" % (mode, seen))
    finally:
        eng.close()


def _frames_late_in_a_run(game, mode, state_of, what):
    """One default-path engine beside the oracle under the agents of (game, mode), up to the first step after which
    state_of(counter, done) names envs: the batched human-size frames of up to four of them, 128 x 128, and of the first at
    192 x 96, against pgo_render_frame of a single oracle env brought to the same state by the same actions (its state dump
    is held to the protocol's own first).  Returns (step, the envs)."""
    L = oracle()
    eng = EngineVec(game, sp.N, seed_base=sp.SEED_BASE, mode=mode)
    history, seen = [], []

    def single(env):
        h = L.pgo_make_mode(game.encode(), sp.SEED_BASE + env, 1, mode)
        L.pgo_reset(h, 0, 0)
        pending = [False]
        for a in history:
            _oracle_step(L, [h], pending, a[env:env + 1])
        return h

    def at_start(ora):
        _same_frames(eng.reset(), ora.reset_obs(), "first reset")

    def each_step(s, ora, a, obs, reward, done, counter):
        history.append(a.copy())
        oe, re_, de = eng.step(a)
        assert np.array_equal(de, done) and np.array_equal(re_.view(np.uint32), reward.view(np.uint32)), s
        _same_frames(oe, obs, "step %d" % s)
        envs = state_of(counter, done)
        if not envs:
            return
        seen.append((s, envs[:4]))
        for k, (w, h) in enumerate(((128, 128), (192, 96))):
            chosen = envs[:4] if k == 0 else envs[:1]
            got = frames_host(eng, chosen, w, h)
            for j, env in enumerate(chosen):
                handle = single(env)
                try:
                    assert_same_dump(oracle_state(handle), counter.after.state(env), "%s, step %d: the single env %d" % (what, s, env))
                    assert_frame(got[j], oracle_frame(L, handle, w, h), "%s, step %d: env %d, %dx%d" % (what, s, env, w, h))
                finally:
                    L.pgo_close(handle)
        raise _Played

    try:
        with pytest.raises(_Played):  # the state is met inside the protocol's run: tests/test_scripted_play.py's floors
            sp.run_on_oracle(game, mode, each_step, at_start, render=True, threads=_host_threads())
    finally:
        eng.close()
    return seen[0]


def test_human_size_frames_late_in_the_level():
    """The three renderers share one draw list, and its late-level inputs come only with the agents.  coinrun: the first
    step after which four envs that play on are past 0.9 of the way to the coin with a lava tile or a saw in view — the
    pits, the coin and the solid fill to the right of its column.  jumper's memory mode: the first step after which an agent
    is 20 cells from where its episode began, in the 45 x 45 world.  Their batched human-size frames against the oracle's."""
    def late(counter, done):
        at = (counter.coinrun_progress(counter.after) > 0.9) & counter.coinrun_hazard_in_view(counter.after) & (done == 0)
        return np.nonzero(at)[0].tolist() if at.sum() >= 4 else []

    def far(counter, done):
        return np.nonzero((counter.far_from_start >= 20) & (done == 0))[0].tolist()

    seen = [_frames_late_in_a_run("coinrun", HARD, late, "coinrun past 0.9 of the way"),
            _frames_late_in_a_run("jumper", MEMORY, far, "jumper 20 cells from its start")]
    print("human-size frames late in the level: coinrun mode %d and jumper mode %d, (step, envs): %r" % (HARD, MEMORY, seen))


@pytest.mark.parametrize("game", sp.GAMES)
def test_same_step_episodes_of_scripted_play(game):
    """step_episodes in same-step mode under the agents, against the model: every step's rows, and with them the float32
    returns (chaser's: a long sum of 0.04s and one 10.04; caveflyer's: 3.0s and a 10.0), the lengths and the terminal frames
    of the episodes that were won."""
    eng = EpisodeEngine(game, sp.N, SAME_STEP, 0, sp.SAME_STEP_RING)
    model = EpisodeModel(game, sp.N, SAME_STEP, 0, sp.SAME_STEP_RING, threads=_host_threads())
    try:
        assert np.array_equal(eng.reset(), model.first_reset())
        counts = sp.run_same_step(game, model, eng, check_step)
        print("scripted play, same-step: %s, %d envs: %r" % (game, sp.N, counts))
        sp.assert_same_step_covers(game, counts)
    finally:
        eng.close(), model.close()
