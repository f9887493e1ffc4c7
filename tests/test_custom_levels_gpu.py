"""Caller-made levels on the device (include/procgen2_vec.h pgv_get_levels / pgv_set_levels), maze in its three modes:
the oracle's levels transplanted into engines made with other seeds and held to the oracle frame by frame, also behind the
draw-list replay and without the render pre-pass; the round trips; random maps the generator never makes against the numpy
step of custom_levels_util (which test_custom_levels.py holds to the oracle), against a queue BFS and across the three
renderers; every refusal; what an install leaves alone; and the neighbours — policy observations, frame history, same-step
episodes, records, snapshots, frameless sequences.  Batches of 131, 65 and 1 envs."""
import ctypes

import numpy as np
import pytest
import torch

from custom_levels_util import (AX, AY, KNOWN_CUSTOM, MODES, MODE_NAMES, SIDE, STATUS, TIMEOUT, Levels, MazeModel, levels_of_dumps,
                                oracle_dumps, oracle_levels, random_levels)
from history_util import Frames
from path_util import MAZE_STEP_ACTIONS, bfs, probe_of

from procgen2_amd import lib as pglib

pytestmark = pytest.mark.gpu

MODE_IDS = [MODE_NAMES[m] for m in MODES]
REPLAY, NO_PREPASS = 1, 1 << 21  # pgv_set_debug: the draw-list replay, no render pre-pass


def make(mode, n, seed_base=1, debug=0, reset=True, game="maze", **kw):
    from procgen2_amd.vec_env import ProcgenVecEnv
    env = ProcgenVecEnv(game, n, seed_base=seed_base, distribution_mode=mode if game == "maze" else None, **kw)
    if debug:
        pglib.check(env.L, env.L.pgv_set_debug(env._h, debug), "pgv_set_debug")
    if reset:
        env.reset()
    return env


def on_device(env, levels):
    return Levels(*(torch.from_numpy(np.ascontiguousarray(x)).to(env.device) for x in levels))


def install(env, levels, indices=None, ids=None, **kw):
    """set_levels with numpy rows put on the device first → the status as numpy."""
    lv = on_device(env, levels)
    if ids is not None:
        ids = torch.from_numpy(np.asarray(ids, np.int64)).to(env.device)
    if indices is not None:
        indices = torch.from_numpy(np.asarray(indices, np.int32)).to(env.device)
    return env.set_levels(lv, ids=ids, indices=indices, **kw).cpu().numpy()


def rows_of(env):
    """Everything an env shows: state rows and tile rows, obs, reward, done and the level words, as numpy."""
    state, lengths = env.state_obs()
    assert (lengths == 10).all()
    return {"state": state.cpu().numpy().view(np.uint32), "tiles": env.tile_obs().cpu().numpy(),
            "obs": env.obs.cpu().numpy().reshape(env.num_envs, -1), "reward": env.reward.cpu().numpy().view(np.uint32),
            "done": env.done.cpu().numpy(), "number": env.level_numbers.view(torch.int32).cpu().numpy(),
            "known": env.level_known.cpu().numpy()}


def assert_same(a, b, what, rows=None, keys=None):
    for key in keys or a:
        x, y = (a[key], b[key]) if rows is None else (a[key][rows], b[key][rows])
        if not np.array_equal(x, y):
            bad = np.nonzero((x != y).reshape(x.shape[0], -1).any(axis=1))[0]
            raise AssertionError("%s: %s differs in rows %s" % (what, key, bad[:8]))


def guided_actions(rng, fields, agent_cells, side, share=0.75):
    """Random actions that end an episode soon: with probability `share` the move that shortens the BFS distance to the goal
    (fields: int16 [B, cells] from the goal), otherwise a uniform draw from the 15 actions."""
    n = len(agent_cells)
    actions = rng.integers(0, 15, n)
    for e in np.nonzero(rng.random(n) < share)[0]:
        actions[e] = MAZE_STEP_ACTIONS[probe_of(fields[e], side, side, int(agent_cells[e]))[1]]
    return actions


# ---------------------------------------------------------------------------------------------------------------------
# The oracle's levels in an engine made with other seeds: frames, rewards, dones and rows, step by step.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_oracle_transplant(mode):
    """(The generator may put the cheese on the mouse's own cell — an episode of one step, common in the smallest mazes.  The
    install refuses such a row, status 4; those envs stay out of the comparison.)"""
    n, side = 65, SIDE[mode]
    o, levels = oracle_levels(mode, n, seed_base=1000 + mode, render=True)
    engines = [make(mode, n, seed_base=5, debug=d) for d in (0, REPLAY, NO_PREPASS)]
    want = {"obs": o.reset_obs().copy(), "state": oracle_dumps(o)[0].view(np.uint32), "tiles": oracle_dumps(o)[1]}
    taken = levels.goal_cell != levels.agent_cell
    assert taken.sum() > n // 2
    for env in engines:
        before = rows_of(env)
        assert not np.array_equal(before["tiles"], want["tiles"]), "other seeds, other levels"
        assert np.array_equal(install(env, levels, ids=np.arange(n) + 7), np.where(taken, 0, STATUS["bad_goal"]))
        got = rows_of(env)
        assert_same(got, want, "the installed level's first frame and rows", rows=taken, keys=("obs", "state", "tiles"))
        assert_same(got, before, "the refused rows", rows=~taken)
        assert not got["reward"].any() and not got["done"].any()
        assert (got["number"][taken] == (np.arange(n) + 7)[taken]).all() and (got["known"][taken] == KNOWN_CUSTOM).all()
    fields = np.stack([bfs(levels.tiles[e], side, side, int(levels.goal_cell[e]), {0}) for e in range(n)])
    rng = np.random.default_rng(mode)
    alive = taken.copy()
    agent = levels.agent_cell.copy()
    steps = 0
    while alive.any():
        assert steps < TIMEOUT
        actions = guided_actions(rng, fields, agent, side)
        obs, reward, done = o.step(actions)
        st, tl = oracle_dumps(o)
        want = {"obs": obs, "reward": reward.view(np.uint32), "done": done, "state": st.view(np.uint32), "tiles": tl}
        for env in engines:
            env.step(torch.from_numpy(actions).to(env.device))
            assert_same(rows_of(env), want, "step %d" % steps, rows=alive, keys=tuple(want))
        alive &= done == 0
        steps += 1
        live = np.nonzero(alive)[0]
        agent[live] = (side - 1 - np.floor(st[live, AY]).astype(np.int64)) + np.floor(st[live, AX]).astype(np.int64) * side
    assert steps >= 8
    o.close()
    for env in engines:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# Round trips.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_get_is_the_symbolic_observations(mode):
    """The law of pgv_get_levels: every field is what pgv_tile_rows and pgv_state_rows give through the cell rule — at a
    reset, mid-episode (the agent's current cell), for any indices, with any output left out, twice the same."""
    n, side = 131, SIDE[mode]
    env = make(mode, n)
    for step in range(6):
        if step:
            env.step_synthetic(3)
        envs = None if step % 2 == 0 else [130, 0, 64, 7, 7, -1, n, 65]
        got = env.get_levels(envs)
        idx = np.arange(n) if envs is None else np.asarray(envs)
        inside = (idx >= 0) & (idx < n)
        state, tiles = env.state_obs(envs)[0].cpu().numpy(), env.tile_obs(envs).cpu().numpy()
        want = levels_of_dumps(state[inside], tiles[inside], side)
        for name, g, w in zip(Levels._fields, got, want):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype, name
            assert np.array_equal(g[inside].view(np.uint32) if g.dtype == np.float32 else g[inside], w.view(np.uint32) if w.dtype == np.float32 else w), (name, step)
        out = [g.cpu().numpy()[~inside] for g in got]
        assert not out[0].any() and (out[1] == -1).all() and (out[2] == -1).all() and not out[3].any() and not out[4].view(np.uint32).any()
        again = env.get_levels(envs)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        host = env.get_levels(envs, host=True)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, host))
    # any output may be left out (the C ABI: NULL pointers); a tile pointer that is on no grid
    cells = side * side
    slab = torch.zeros(3 + n * cells, dtype=torch.uint8, device=env.device)
    for shift in (1, 2, 3):
        rows = pglib.level_rows(tiles=slab.data_ptr() + shift)
        env._before()
        pglib.check(env.L, env.L.pgv_get_levels(env._h, None, n, ctypes.byref(rows)), "pgv_get_levels")
        env._after()
        assert torch.equal(slab[shift:shift + n * cells].view(n, cells), env.tile_obs()) and not slab[:shift].any() and not slab[shift + n * cells:].any()
        slab.zero_()
    cell = torch.full((n,), -5, dtype=torch.int32, device=env.device)
    rows = pglib.level_rows(goal_cell=cell.data_ptr())
    env._before()
    pglib.check(env.L, env.L.pgv_get_levels(env._h, None, n, ctypes.byref(rows)), "pgv_get_levels")
    env._after()
    assert torch.equal(cell, env.get_levels().goal_cell)
    env.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_round_trip(mode):
    """get from engine A after a reset, set into engine B: B's rows and frames are A's.  set(get(x)) on the same envs at an
    episode start changes no byte of state or obs."""
    n = 131
    a, b = make(mode, n, seed_base=1), make(mode, n, seed_base=777)
    levels = a.get_levels()
    # (a generated level whose cheese lies on the mouse's own cell is refused, status 4: such rows stay out)
    taken = (levels.goal_cell != levels.agent_cell).cpu().numpy()
    want_status = np.where(taken, 0, STATUS["bad_goal"])
    assert taken.sum() > n // 2
    assert np.array_equal(b.set_levels(levels).cpu().numpy(), want_status)
    assert_same(rows_of(b), rows_of(a), "B after set(get(A))", rows=taken, keys=("state", "tiles", "obs", "reward", "done"))
    before = rows_of(a)
    assert np.array_equal(a.set_levels(a.get_levels()).cpu().numpy(), want_status)
    assert_same(rows_of(a), before, "A after set(get(A))", keys=("state", "tiles", "obs", "reward", "done"))
    # … through the host forms too, for a few envs in another order
    envs = np.nonzero(taken)[0][[5, -1, 0, 30]]
    host = a.get_levels(envs, host=True)
    status = b.set_levels(host, indices=envs[::-1].copy(), ids=np.array([1, 2, 3, 2 ** 32 - 1], np.uint32))
    assert isinstance(status, np.ndarray) and (status == 0).all()
    got, want = rows_of(b), rows_of(a)
    for key in ("state", "tiles", "obs"):
        assert np.array_equal(got[key][envs[::-1]], want[key][envs]), key
    assert list(got["number"][envs[::-1]].view(np.uint32)) == [1, 2, 3, 2 ** 32 - 1]
    # and both go on alike under the same actions
    a.set_levels(a.get_levels())
    b.set_levels(a.get_levels())
    rng = np.random.default_rng(0)
    alive = taken.copy()  # (behind its first done an env is in a level of its own engine's making)
    for s in range(12):
        actions = torch.from_numpy(rng.integers(0, 15, n)).to(a.device)
        a.step(actions), b.step(actions)
        assert_same(rows_of(b), rows_of(a), "step %d" % s, rows=alive, keys=("state", "tiles", "obs", "reward", "done"))
        alive &= a.done.cpu().numpy() == 0
    assert alive.any()
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------------
# Maps the generator never makes.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_random_maps_against_the_model(mode):
    """(a) Random actions: rewards, dones and state rows are the numpy model's, bit for bit, through every env's first done."""
    n = 131
    levels, reachable = random_levels(mode, n)
    assert 0.25 <= reachable.mean() <= 0.90
    env = make(mode, n)
    assert (install(env, levels) == 0).all()
    model = MazeModel(mode, levels)
    got = rows_of(env)
    assert np.array_equal(got["state"], model.rows.view(np.uint32)) and np.array_equal(got["tiles"], model.tiles)
    rng = np.random.default_rng(100 + mode)
    alive = np.ones(n, bool)
    goals = 0
    for s in range(TIMEOUT):
        actions = rng.integers(0, 15, n)
        env.step(torch.from_numpy(actions).to(env.device))
        reward, done = model.step(actions)
        want = {"reward": reward.view(np.uint32), "done": done, "state": model.rows.view(np.uint32), "tiles": model.tiles}
        assert_same(rows_of(env), want, "step %d" % s, rows=alive, keys=tuple(want))
        goals += int((reward[alive] > 0).sum())
        alive &= done == 0
    assert not alive.any(), "every episode ends by the step cap"
    assert goals > 0
    env.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_random_maps_paths_and_the_policy(mode):
    """(b) tile_paths over the installed bytes is the queue BFS; the policy read off probe_step ends a reachable row in exactly
    probe_dist steps with reward 10, an unreachable row at step 500 with reward 0."""
    n, side = 131, SIDE[mode]
    levels, reachable = random_levels(mode, n)
    assert 0.25 <= reachable.mean() <= 0.90
    env = make(mode, n)
    assert (install(env, levels) == 0).all()
    paths = env.tile_paths(source="goal", probe="agent")
    fields = np.stack([bfs(levels.tiles[e], side, side, int(levels.goal_cell[e]), {0}) for e in range(n)])
    assert np.array_equal(paths.dist.cpu().numpy(), fields)
    dist = fields[np.arange(n), levels.agent_cell].astype(np.int32)
    assert np.array_equal(paths.probe_dist.cpu().numpy(), dist) and np.array_equal(dist >= 0, reachable)
    assert np.array_equal(paths.cells.cpu().numpy(), np.stack([levels.goal_cell, levels.agent_cell], axis=1))
    table = torch.tensor(MAZE_STEP_ACTIONS, device=env.device)
    ended_at, ended_reward = np.zeros(n, np.int64), np.zeros(n, np.float32)
    alive = np.ones(n, bool)
    for s in range(1, TIMEOUT + 1):
        env.step(table[env.tile_paths(source="goal", probe="agent", dist=False).probe_step.long()])
        reward, done = env.reward.cpu().numpy(), env.done.cpu().numpy()
        now = alive & (done != 0)
        ended_at[now], ended_reward[now] = s, reward[now]
        assert not reward[alive & ~now].any()
        alive &= ~now
        if not alive[reachable].any() and s < TIMEOUT - 1:  # the rest only wait for the cap: without frames, in one call
            rest = TIMEOUT - 1 - s
            res = env.step_sequence(steps=rest, actions=torch.full((n,), 4, dtype=torch.int32, device=env.device), frames="none")
            assert not res.dones.cpu().numpy()[:, alive].any() and not res.rewards.cpu().numpy()[:, alive].any()
            s += rest
            env.step(torch.full((n,), 4, dtype=torch.int32, device=env.device))
            reward, done = env.reward.cpu().numpy(), env.done.cpu().numpy()
            assert done[alive].all() and not reward[alive].any()
            ended_at[alive], alive[:] = TIMEOUT, False
            break
    assert not alive.any()
    assert np.array_equal(ended_at[reachable], dist[reachable]) and (ended_reward[reachable] == 10.0).all()
    assert (ended_at[~reachable] == TIMEOUT).all() and not ended_reward[~reachable].any()
    env.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_random_maps_across_the_renderers(mode):
    """(c) The row composer against the blit-at-a-time path and the path without a pre-pass, byte for byte, on maps with open
    cells on the world border and (memory mode) the camera next to the edge."""
    n = 131
    levels, _ = random_levels(mode, n)
    engines = [make(mode, n, debug=d) for d in (0, REPLAY, NO_PREPASS)]
    for env in engines:
        assert (install(env, levels) == 0).all()
    rng = np.random.default_rng(mode)
    frames = set()
    for s in range(41):
        if s:
            actions = rng.integers(0, 9, n)
            for env in engines:
                env.step(torch.from_numpy(actions).to(env.device))
        first = rows_of(engines[0])
        alive = first["known"] == KNOWN_CUSTOM  # (an env that ended is in a level of its own again: equal too, not the point)
        for env, name in zip(engines[1:], ("draw-list replay", "no pre-pass")):
            assert_same(rows_of(env), first, "%s, step %d" % (name, s), keys=("obs", "state", "reward", "done"))
        frames.add(first["obs"][alive].tobytes())
    assert len(frames) == 41 and alive.sum() > n // 2
    for env in engines:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# Refusals.
# ---------------------------------------------------------------------------------------------------------------------
def test_every_status_and_nothing_else_is_touched():
    mode, n, side = 2, 65, SIDE[2]
    a, twin = make(mode, n), make(mode, n)
    for s in range(5):  # mid-episode: rewards, dones and frames that a stray write would show in
        a.step_synthetic(9), twin.step_synthetic(9)
    good, _ = random_levels(mode, 20)
    lv = Levels(*(x.copy() for x in good))
    wall = lambda k: int(np.nonzero(lv.tiles[k] == 1)[0][0])
    want = np.zeros(20, np.int32)  # (rows 0 and 16 .. 19 are installed)
    indices = np.arange(20, dtype=np.int32) * 3  # envs 0, 3, …, 57; the others are not named
    indices[1], want[1] = n, STATUS["no_env"]
    indices[2], want[2] = -1, STATUS["no_env"]
    lv.tiles[3, side * side - 1], want[3] = 2, STATUS["bad_tile"]           # the row's last byte: off the word grid
    lv.tiles[4, 0], want[4] = 255, STATUS["bad_tile"]
    lv.agent_cell[5], want[5] = wall(5), STATUS["bad_agent"]
    lv.agent_cell[6], want[6] = side * side, STATUS["bad_agent"]
    lv.agent_cell[7], want[7] = -1, STATUS["bad_agent"]
    lv.goal_cell[8], want[8] = wall(8), STATUS["bad_goal"]
    lv.goal_cell[9], want[9] = lv.agent_cell[9], STATUS["bad_goal"]
    lv.goal_cell[10], want[10] = 2 ** 31 - 1, STATUS["bad_goal"]
    lv.background[11], want[11] = 9, STATUS["bad_floor"]
    lv.background[12], want[12] = -1, STATUS["bad_floor"]
    lv.background_shift[13], want[13] = 1.0, STATUS["bad_floor"]
    lv.background_shift[14], want[14] = np.nan, STATUS["bad_floor"]
    lv.tiles[15, 7], lv.agent_cell[15], want[15] = 3, -7, STATUS["bad_tile"]  # the first code that applies
    status = install(a, lv, indices=indices, ids=np.arange(20) + 100)
    assert np.array_equal(status, want), status
    installed = indices[want == 0]
    others = np.setdiff1d(np.arange(n), installed)
    got, untouched = rows_of(a), rows_of(twin)
    assert_same(got, untouched, "refused rows and rows not named", rows=others)
    model = MazeModel(mode, Levels(*(x[want == 0] for x in lv)))
    assert np.array_equal(got["state"][installed], model.rows.view(np.uint32)) and np.array_equal(got["tiles"][installed], model.tiles)
    assert (got["known"][installed] == KNOWN_CUSTOM).all() and np.array_equal(got["number"][installed], np.arange(20)[want == 0] + 100)
    for shift in (np.inf, -np.inf, -0.25, np.float32(1.0) + np.float32(2.0 ** -23)):
        lv2 = Levels(*(x[:1].copy() for x in good))
        lv2.background_shift[0] = shift
        assert list(install(a, lv2, indices=[1])) == [STATUS["bad_floor"]], shift
    assert_same(rows_of(a), untouched, "after more refusals", rows=others)
    # without background / background_shift an env keeps the floor it has; the largest shift below 1 is fine
    floor = got["state"][1, 6:8].copy()
    lv2 = Levels(good.tiles[:1], good.agent_cell[:1], good.goal_cell[:1], None, None)
    assert list(a.set_levels(tiles=torch.from_numpy(lv2.tiles).to(a.device), agent_cell=[int(lv2.agent_cell[0])], goal_cell=[int(lv2.goal_cell[0])],
                             indices=[1]).cpu().numpy()) == [0]
    after = rows_of(a)
    assert np.array_equal(after["state"][1, 6:8], floor) and after["known"][1] == KNOWN_CUSTOM and after["number"][1] == 0
    lv2 = Levels(*(x[:1].copy() for x in good))
    lv2.background_shift[0], lv2.background[0] = np.nextafter(np.float32(1.0), np.float32(0.0)), 8
    assert list(install(a, lv2, indices=[2])) == [0]
    # two rows that name one env: one wins whole, nothing faults
    two = Levels(*(x[:2].copy() for x in good))
    assert list(install(a, two, indices=[3, 3])) == [0, 0]
    st, tl = rows_of(a)["state"][3], rows_of(a)["tiles"][3]
    winners = [MazeModel(mode, Levels(*(x[k:k + 1] for x in two))) for k in (0, 1)]
    assert any(np.array_equal(st, w.rows[0].view(np.uint32)) and np.array_equal(tl, w.tiles[0]) for w in winners)
    a.close(), twin.close()


def test_host_refusals():
    mode, n = 1, 1
    env = make(mode, n)
    L, h = env.L, env._h
    error = lambda: (L.pgv_last_error() or b"").decode()
    good, _ = random_levels(mode, 1)
    lv = on_device(env, good)
    before = rows_of(env)
    full = lambda **kw: pglib.level_rows(**dict(dict(tiles=lv.tiles.data_ptr(), agent_cell=lv.agent_cell.data_ptr(), goal_cell=lv.goal_cell.data_ptr()), **kw))
    for name in ("pgv_set_levels", "pgv_get_levels"):
        fn = getattr(L, name)
        assert fn(h, None, 1, None) != 0 and name + ":" in error() and "NULL" in error()
        small = full()
        small.struct_size -= 8
        assert fn(h, None, 1, ctypes.byref(small)) != 0 and "struct_size" in error()
        assert fn(h, None, -1, ctypes.byref(full())) != 0 and "count" in error()
        assert fn(h, None, 1, ctypes.byref(full(status=lv.agent_cell.data_ptr() + 2))) != 0 and "aligned" in error()
        assert fn(h, None, 0, ctypes.byref(pglib.level_rows())) == 0  # count = 0 succeeds and writes nothing
    for missing in ("tiles", "agent_cell", "goal_cell"):
        assert L.pgv_set_levels(h, None, 1, ctypes.byref(full(**{missing: None}))) != 0 and missing in error() and "NULL" in error()
        assert L.pgv_set_levels_host(h, None, 1, ctypes.byref(full(**{missing: None}))) != 0 and missing in error()
    assert L.pgv_set_levels(h, None, 0, ctypes.byref(full(tiles=None))) == 0
    env.sync()
    assert_same(rows_of(env), before, "after the host's refusals")
    with pytest.raises(ValueError):
        env.set_levels(tiles=lv.tiles)
    with pytest.raises(ValueError):
        env.set_levels(lv, indices=[0, 0])
    env.close()
    for game in ("coinrun", "chaser"):
        other = make(0, 3, game=game)
        assert not other.level_layout.supported
        rows = pglib.level_rows(tiles=other.obs.data_ptr(), agent_cell=other.reward.data_ptr(), goal_cell=other.reward.data_ptr())
        for name in ("pgv_set_levels", "pgv_get_levels", "pgv_set_levels_host", "pgv_get_levels_host"):
            assert getattr(other.L, name)(other._h, None, 1, ctypes.byref(rows)) != 0
            assert "no caller-made levels for this game" in (other.L.pgv_last_error() or b"").decode(), name
        with pytest.raises(pglib.EngineError):
            other.get_levels()
        other.close()


# ---------------------------------------------------------------------------------------------------------------------
# What an install does not touch.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_the_levels_behind_a_custom_episode(mode):
    """Env i of A plays a custom level, env i of the twin its own; both end at the step cap.  From there A is the twin: the
    same stream, the same prefetched level, level after level.  A pending assignment survives the install and is consumed
    by the next build."""
    n = 65
    a, twin = make(mode, n), make(mode, n)
    own = twin.get_levels()  # (a level whose cheese lies on the mouse's own cell ends at its first step, not at the cap: not named)
    named = np.nonzero((own.goal_cell != own.agent_cell).cpu().numpy())[0][::2]
    assert named.size > n // 4
    assigned = named[::3]
    numbers = (assigned + 4000).astype(np.int32)
    for env in (a, twin):
        env.assign_levels(torch.from_numpy(numbers).to(env.device), torch.from_numpy(assigned.astype(np.int32)).to(env.device))
    levels, _ = random_levels(mode, named.size)
    launches = a.L.pgv_generator_launches(a._h)
    assert (install(a, levels, indices=named) == 0).all()
    assert a.L.pgv_generator_launches(a._h) == launches, "an install launches no generator"
    assert_same(rows_of(a), rows_of(twin), "the envs not named", rows=np.setdiff1d(np.arange(n), named))
    stay = torch.full((n,), 4, dtype=torch.int32, device=a.device)
    for env in (a, twin):
        res = env.step_sequence(steps=TIMEOUT, actions=stay, frames="none")
        dones = res.dones.cpu().numpy()[:, named]
        assert dones[TIMEOUT - 1].all() and not dones[:TIMEOUT - 1].any()
    rng = np.random.default_rng(mode)
    for s in range(60):
        actions = torch.from_numpy(rng.integers(0, 15, n)).to(a.device)
        if s:
            paths = [env.tile_paths(source="goal", probe="agent", dist=False).probe_step for env in (a, twin)]
            assert torch.equal(paths[0], paths[1])
            follow = torch.from_numpy(rng.random(n) < 0.8).to(a.device)
            actions = torch.where(follow, torch.tensor(MAZE_STEP_ACTIONS, device=a.device)[paths[0].long()], actions)
        a.step(actions), twin.step(actions)
        got = rows_of(a)
        assert_same(got, rows_of(twin), "step %d behind the custom episodes" % s)
        if s == 0:  # the step that serves the resets: the assigned levels are built now, in both
            assert np.array_equal(got["number"][assigned], numbers) and (got["known"][assigned] == 1).all()
            rest = np.setdiff1d(named, assigned)
            assert not got["known"][rest].any() and not got["number"][rest].any()
    a.close(), twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# Neighbours.
# ---------------------------------------------------------------------------------------------------------------------
def test_policy_observations_and_history_restart():
    """An installed env's stack is K copies of the level's first frame and its began byte is set: the numpy models of both
    features, driven as for a masked reset."""
    mode, n, K, T = 2, 65, 3, 4
    env = make(mode, n, reset=False, policy_obs=dict(stack=K, gray=True, dtype="uint8"), history=dict(capacity=T, gray=True))
    model = Frames(n, T, True, policy=(K, "uint8"))
    model.reset(env.reset().cpu().numpy())
    rng = np.random.default_rng(1)
    levels, _ = random_levels(mode, n)
    named = np.zeros(n, np.uint8)

    def check(what):
        assert np.array_equal(env.policy_obs.cpu().numpy(), model.stack.out), what + ": policy_obs"
        assert np.array_equal(env.policy_restart.cpu().numpy(), model.stack.restart), what
        h = env.history
        assert h.head == model.ring.head and np.array_equal(h.frames.cpu().numpy(), model.ring.frames), what + ": history frames"
        assert np.array_equal(h.began.cpu().numpy(), model.ring.began) and np.array_equal(h.pending.cpu().numpy(), model.ring.pending), what

    for round_ in range(3):
        for s in range(3):
            model.flag(env.done.cpu().numpy())
            obs, _, _ = env.step(torch.from_numpy(rng.integers(0, 15, n)).to(env.device))
            model.push(obs.cpu().numpy())
            check("step")
        idx = np.where(rng.random(n) < 0.4, np.arange(n), -1).astype(np.int32)  # the fixed-size call
        idx[0] = 0
        status = install(env, levels, indices=idx)
        assert np.array_equal(status, np.where(idx >= 0, 0, 1))
        named = (idx >= 0).astype(np.uint8)
        model.reset(env.obs.cpu().numpy(), named)
        check("install %d" % round_)
        first = env.obs.cpu().numpy().reshape(n, 64, 64, 3)[named != 0].astype(np.uint32)
        gray = ((77 * first[..., 0] + 150 * first[..., 1] + 29 * first[..., 2] + 128) >> 8).astype(np.uint8)
        stack = env.policy_obs.cpu().numpy()[named != 0]
        assert all(np.array_equal(stack[:, k], gray) for k in range(K))
        assert env.history.began.cpu().numpy()[(env.history.head - 1) % T][named != 0].all()
    env.close()


def test_install_on_ended_behind_same_step_episodes():
    """indices = where(ended, arange, -1) behind a same-step step_episodes, with no look from the host: every env plays
    custom levels only; ended_level / ended_level_known report the caller's ids with known 2; rewards, returns and lengths
    are the numpy model's."""
    mode, n, limit = 1, 131, 6
    env = make(mode, n, autoreset_mode="same_step", max_episode_steps=limit)
    levels, _ = random_levels(mode, n)
    dev = on_device(env, levels)
    arange = torch.arange(n, dtype=torch.int32, device=env.device)
    ids = arange + 10000
    assert (env.set_levels(dev, ids=ids).cpu().numpy() == 0).all()
    model = MazeModel(mode, levels)
    label = ids.cpu().numpy().astype(np.int64)
    ret, length = np.zeros(n, np.float32), np.zeros(n, np.int32)
    assert not env.episode.running_length.cpu().numpy().any()
    rng = np.random.default_rng(2)
    fields = np.stack([bfs(levels.tiles[e], SIDE[mode], SIDE[mode], int(levels.goal_cell[e]), {0}) for e in range(n)])
    total = goals = 0
    for s in range(50):
        agent = (SIDE[mode] - 1 - np.floor(model.rows[:, AY]).astype(np.int64)) + np.floor(model.rows[:, AX]).astype(np.int64) * SIDE[mode]
        actions = guided_actions(rng, fields, agent, SIDE[mode], share=0.6)
        obs, ep = env.step_episodes(torch.from_numpy(actions).to(env.device))
        ids = ids + n
        status = env.set_levels(dev, ids=ids, indices=torch.where(ep.ended != 0, arange, torch.full_like(arange, -1)))
        reward, done = model.step(actions)
        ret, length = ret + reward, length + 1
        ended = (done != 0) | (length >= limit)
        where = np.nonzero(ended)[0]
        c = int(ep.counts.cpu().numpy()[0])
        assert np.array_equal(ep.reward.cpu().numpy().view(np.uint32), reward.view(np.uint32)), s
        assert np.array_equal(ep.terminated.cpu().numpy(), done) and np.array_equal(ep.ended.cpu().numpy() != 0, ended), s
        assert c == where.size and np.array_equal(ep.ended_env.cpu().numpy()[:c], where)
        assert np.array_equal(ep.ended_return.cpu().numpy()[:c].view(np.uint32), ret[where].view(np.uint32))
        assert np.array_equal(ep.ended_length.cpu().numpy()[:c], length[where])
        assert np.array_equal(ep.ended_level.view(torch.int32).cpu().numpy()[:c].astype(np.int64), label[where]), s
        assert (ep.ended_level_known.cpu().numpy()[:c] == KNOWN_CUSTOM).all()
        assert np.array_equal(status.cpu().numpy(), np.where(ended, 0, 1))
        model.install(where, Levels(*(x[where] for x in levels)))
        label[where] = ids.cpu().numpy().astype(np.int64)[where]
        ret[where], length[where] = 0.0, 0
        got = rows_of(env)
        assert np.array_equal(got["state"], model.rows.view(np.uint32)) and np.array_equal(got["tiles"], model.tiles), s
        assert np.array_equal(got["number"].astype(np.int64), label) and (got["known"] == KNOWN_CUSTOM).all()
        assert np.array_equal(env.episode.running_length.cpu().numpy(), length)
        assert np.array_equal(env.episode.running_return.cpu().numpy().view(np.uint32), ret.view(np.uint32))
        total += c
        goals += int((reward > 0).sum())
    assert total > n and goals > 0
    env.close()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_fork_snapshot_and_frameless_sequences(mode):
    """A custom level is live state and nothing else: a fork of an env on one goes on equal to its source, a snapshot resumes
    in a fresh engine, and step_sequence(frames="none") gives the model's rewards and dones."""
    n, T = 65, 24
    env = make(mode, n)
    half = n // 2
    levels, _ = random_levels(mode, half)
    record_bytes = env.env_record_bytes
    assert (install(env, levels, indices=np.arange(half), ids=np.arange(half) + 1) == 0).all()
    assert env.env_record_bytes == record_bytes
    model = MazeModel(mode, levels)
    rng = np.random.default_rng(mode)
    actions = rng.integers(0, 9, (3, n))
    alive = np.ones(half, bool)  # (the custom envs still in their custom episode: the model's)
    for t in range(3):
        env.step(torch.from_numpy(actions[t]).to(env.device))
        alive &= model.step(actions[t, :half])[1] == 0
    # fork: envs 0 .. half-1 (custom, mid-episode) into the slots behind them
    src, dst = np.arange(half), np.arange(half) + half
    env.fork(torch.from_numpy(src).to(env.device), torch.from_numpy(dst).to(env.device))
    got = rows_of(env)
    for key in got:
        assert np.array_equal(got[key][dst], got[key][src]), key
    assert (got["known"][dst] == KNOWN_CUSTOM).all()
    # a snapshot of the lot, into a fresh engine with other seeds' levels
    fresh = make(mode, n)
    fresh.load_state(env.save_state())
    assert_same(rows_of(fresh), got, "the loaded snapshot")
    # frameless sub-steps: both engines, against each other and against the model through each env's first done
    seq = rng.integers(0, 15, (T, n))
    seq[:, dst] = seq[:, src]
    results = [e.step_sequence(torch.from_numpy(seq).to(e.device), frames="none") for e in (env, fresh)]
    rewards, dones = results[0].rewards.cpu().numpy(), results[0].dones.cpu().numpy()
    assert np.array_equal(rewards.view(np.uint32), results[1].rewards.cpu().numpy().view(np.uint32)) and np.array_equal(dones, results[1].dones.cpu().numpy())
    assert np.array_equal(rewards[:, dst].view(np.uint32), rewards[:, src].view(np.uint32)) and np.array_equal(dones[:, dst], dones[:, src])
    assert alive.sum() > half // 2
    for t in range(T):
        reward, done = model.step(seq[t, :half])
        assert np.array_equal(rewards[t, :half][alive].view(np.uint32), reward[alive].view(np.uint32)), t
        assert np.array_equal(dones[t, :half][alive], done[alive]), t
        alive &= done == 0
    env.render_obs(), fresh.render_obs()
    got = rows_of(env)
    assert_same(rows_of(fresh), got, "behind the sequence")
    assert np.array_equal(got["state"][:half][alive], model.rows.view(np.uint32)[alive])
    for key in ("state", "tiles", "obs"):
        assert np.array_equal(got[key][dst], got[key][src]), key
    env.close(), fresh.close()


def test_one_env():
    """A batch of one: the whole loop — get, edit in torch, set, play to the goal."""
    env = make(1, 1)
    lv = env.get_levels()
    side = SIDE[1]
    lv.tiles.fill_(1)
    lv.tiles[0, 3 + 2 * side:3 + 9 * side:side] = 0  # a corridor along x at y = 3, x = 2 .. 8
    lv = lv._replace(agent_cell=torch.tensor([3 + 2 * side], dtype=torch.int32, device=env.device),
                     goal_cell=torch.tensor([3 + 8 * side], dtype=torch.int32, device=env.device))
    assert list(env.set_levels(lv, ids=[42]).cpu().numpy()) == [0]
    assert int(env.level_numbers.view(torch.int32)[0]) == 42 and int(env.level_known[0]) == KNOWN_CUSTOM
    assert int(env.tile_paths().probe_dist[0]) == 6
    for s in range(6):
        _, reward, done = env.step([7])  # x + 1
        assert (float(reward[0]), int(done[0])) == ((10.0, 1) if s == 5 else (0.0, 0))
    env.step([4])
    assert int(env.level_known[0]) == 0 and int(env.level_numbers.view(torch.int32)[0]) == 0  # the env's own next level
    env.close()
