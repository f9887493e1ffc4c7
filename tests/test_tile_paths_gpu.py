"""Path distances on the device (include/procgen2_vec.h pgv_tile_paths_rows), held bit for bit to the queue BFS of
tests/path_util.py: every tile game and mode at the checkpoints of the oracle run, every passable set, caller-given cells,
any indices and counts, each output alone, behind resets, frameless sequences and same-step auto-resets, the refusals, the
host form, and the maze law: the policy read off the field ends every episode when the field says."""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

import procgen2_amd
from path_util import (AGENT, CELLS, GOAL, GOAL_COLS, NONE, TILE_GAMES, manhattan, model_at, model_rows)
from state_obs_util import MODE_NAMES, N, NON_DEFAULT, RUN_SEED, SEED_BASE, checkpoints

from procgen2_amd import lib as pglib

pytestmark = pytest.mark.gpu

KINDS = {NONE: "none", AGENT: "agent", GOAL: "goal", CELLS: "cells"}
TILE_NON_DEFAULT = tuple((g, m) for g, m in NON_DEFAULT if g in TILE_GAMES)
THIRDS = (checkpoints()[0:5], checkpoints()[5:10], checkpoints()[10:])


def make(game, n=N, **kw):
    from procgen2_amd.vec_env import ProcgenVecEnv
    env = ProcgenVecEnv(game, n, seed_base=SEED_BASE, **kw)
    env.reset()
    return env


def ask(env, source, probe, passable=(0,), envs=None, source_cells=None, probe_cells=None):
    """tile_paths → the four outputs as numpy."""
    res = env.tile_paths(KINDS[source], KINDS[probe], passable, envs, source_cells, probe_cells)
    return res.dist.cpu().numpy(), res.probe_dist.cpu().numpy(), res.probe_step.cpu().numpy(), res.cells.cpu().numpy()


def assert_equal(got, want, what):
    for name, g, w in zip(("dist", "probe_dist", "probe_step", "cells_out"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s, the model's %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
            raise AssertionError("%s: %s differs in rows %s" % (what, name, rows[:8]))


def dumps_of(env, envs=None):
    """The state and tile dumps of the envs, from the symbolic observations (which test_state_obs_gpu.py holds to the
    oracle); None for an index outside the batch."""
    rows, lengths = env.state_obs(envs)
    tiles = env.tile_obs(envs).cpu().numpy()
    rows, lengths = rows.cpu().numpy(), lengths.cpu().numpy()
    idx = np.arange(env.num_envs) if envs is None else np.asarray(envs, np.int64).reshape(-1)
    inside = (idx >= 0) & (idx < env.num_envs)
    return ([rows[k, :lengths[k]] if inside[k] else None for k in range(idx.size)],
            [tiles[k] if inside[k] else None for k in range(idx.size)])


def model_of(env, game, source, probe, passable=(0,), envs=None, source_cells=None, probe_cells=None):
    lay = env.path_layout
    states, tiles = dumps_of(env, envs)
    return model_rows(game, states, tiles, lay.tile_w, lay.tile_h, source, probe, passable, source_cells, probe_cells)


def check_sources(env, game, mode, step, what, n_steps=None):
    lay = env.path_layout
    want = model_at(game, mode, step, lay.tile_w, lay.tile_h, AGENT, NONE, (0,), n_steps)
    assert_equal(ask(env, AGENT, NONE), want, "%s, source = agent" % what)
    if game in GOAL_COLS:
        want = model_at(game, mode, step, lay.tile_w, lay.tile_h, GOAL, AGENT, (0,), n_steps)
        assert_equal(ask(env, GOAL, AGENT), want, "%s, source = goal, probe = agent" % what)
        return int(want.probe_dist.max())
    return int(want.dist.max())


@pytest.mark.parametrize("third", range(3))
@pytest.mark.parametrize("game", TILE_GAMES)
def test_parity_with_the_model(game, third):
    env = make(game)
    longest = 0
    for s in range(THIRDS[third][-1] + 1):
        if s:
            env.step_synthetic(RUN_SEED)
        if s in THIRDS[third]:
            longest = max(longest, check_sources(env, game, 0, s, "%s step %d" % (game, s)))
    env.close()
    assert longest >= 8, "short paths only: %d" % longest


@pytest.mark.parametrize("game,mode", TILE_NON_DEFAULT, ids=["%s-%s" % (g, MODE_NAMES[m]) for g, m in TILE_NON_DEFAULT])
def test_every_other_mode(game, mode):
    env = make(game, distribution_mode=mode)
    assert pglib.MODES[env.distribution_mode] == mode
    for s in range(8 + 1):
        if s:
            env.step_synthetic(RUN_SEED)
        if s in (0, 8):
            check_sources(env, game, mode, s, "%s mode %d step %d" % (game, mode, s))
    env.close()


def settled(game, steps=8, n=N, **kw):
    env = make(game, n, **kw)
    for _ in range(steps):
        env.step_synthetic(RUN_SEED)
    return env


@pytest.mark.parametrize("game", ["coinrun", "climber"])  # 64 x 64: the full wave and bit 63; 20 x 64: not square
def test_every_id_passable_is_the_manhattan_distance(game):
    env = settled(game)
    lay = env.path_layout
    assert (lay.tile_w, lay.tile_h) == {"coinrun": (64, 64), "climber": (20, 64)}[game]
    for passable in (0xFFFFFFFF, tuple(range(32))):
        dist, probe_dist, probe_step, cells = ask(env, AGENT, NONE, passable)
        assert (cells[:, 0] >= 0).all() and (cells[:, 1] == -1).all() and (probe_dist == -1).all() and not probe_step.any()
        for e in range(N):
            assert np.array_equal(dist[e], manhattan(lay.tile_w, lay.tile_h, int(cells[e, 0]))), (game, e)
    # … and from the four corners, with the opposite corner as the probe: w - 1 + h - 1 steps, the first along x
    corners = [0, lay.tile_h - 1, (lay.tile_w - 1) * lay.tile_h, lay.cells - 1]
    dist, probe_dist, probe_step, cells = ask(env, CELLS, CELLS, 0xFFFFFFFF, [0, 1, 2, 3], corners, corners[::-1])
    for k in range(4):
        assert np.array_equal(dist[k], manhattan(lay.tile_w, lay.tile_h, corners[k])), (game, k)
    assert (probe_dist == lay.tile_w + lay.tile_h - 2).all() and list(probe_step) == [1, 1, 2, 2]
    assert_equal((dist, probe_dist, probe_step, cells), model_of(env, game, CELLS, CELLS, range(32), [0, 1, 2, 3], corners, corners[::-1]), game)
    env.close()


@pytest.mark.parametrize("game,passable", [("maze", ()), ("coinrun", ()), ("chaser", (0, 2)), ("chaser", (2,)), ("coinrun", (0, 5)),
                                           ("jumper", (0, 1, 40))])
def test_passable_sets(game, passable):
    env = settled(game)
    if any(t >= 32 for t in passable):  # an id of 32 and above cannot be said, and is never passable
        with pytest.raises(ValueError):
            env.tile_paths(passable=passable)
        passable = tuple(t for t in passable if t < 32)
    got = ask(env, AGENT, NONE, passable)
    assert_equal(got, model_of(env, game, AGENT, NONE, passable), "%s %s" % (game, passable))
    if not passable:  # the source alone
        assert ((got[0] == 0).sum(axis=1) == 1).all() and ((got[0] == -1).sum(axis=1) == env.path_layout.cells - 1).all()
    mask = sum(1 << t for t in passable)
    assert_equal(ask(env, AGENT, NONE, mask), got, "%s mask %d" % (game, mask))
    env.close()


@pytest.mark.parametrize("game", ["maze", "chaser", "climber"])
def test_given_cells(game):
    env = settled(game, 0)
    lay = env.path_layout
    tiles = env.tile_obs().cpu().numpy()
    wall = int(np.nonzero(tiles[0] != 0)[0][0])
    special = [-1, lay.cells, 0, lay.cells - 1, lay.tile_h - 1, (lay.tile_w - 1) * lay.tile_h, wall, 2 ** 31 - 1, -(2 ** 31)]
    envs = [0] * len(special) + [5, 6]
    source_cells = special + [wall, 0]
    probe_cells = special[::-1] + [0, wall]
    for source, probe in ((CELLS, CELLS), (CELLS, AGENT), (AGENT, CELLS), (CELLS, NONE)):
        sc, pc = source_cells if source == CELLS else None, probe_cells if probe == CELLS else None
        got = ask(env, source, probe, (0,), envs, sc, pc)
        assert_equal(got, model_of(env, game, source, probe, (0,), envs, sc, pc), "%s %s %s" % (game, KINDS[source], KINDS[probe]))
        if source == CELLS:
            assert list(got[3][:9, 0]) == [-1, -1, 0, lay.cells - 1, lay.tile_h - 1, (lay.tile_w - 1) * lay.tile_h, wall, -1, -1]
            assert (got[0][[0, 1, 7, 8]] == -1).all() and got[0][6, wall] == 0
    with pytest.raises(ValueError):
        env.tile_paths("cells", "none", envs=envs)
    with pytest.raises(ValueError):
        env.tile_paths("cells", "none", envs=envs, source_cells=[0, 1])
    env.close()


def raw(env, count, idx=None, passable=1, source=AGENT, probe=NONE, source_cells=None, probe_cells=None, dist=None, probe_dist=None,
        probe_step=None, cells_out=None, size=None, host=False):
    """pgv_tile_paths_rows itself, on tensors (or, host=True, numpy arrays) given as they are; returns the status."""
    ptr = (lambda x: None if x is None else x if isinstance(x, int) else x.ctypes.data) if host else (
        lambda x: None if x is None else x if isinstance(x, int) else x.data_ptr())
    q = pglib.TilePathsStruct(ctypes.sizeof(pglib.TilePathsStruct) if size is None else size, passable, source, ptr(source_cells),
                              probe, ptr(probe_cells), ptr(dist), ptr(probe_dist), ptr(probe_step), ptr(cells_out))
    call = env.L.pgv_tile_paths_rows_host if host else env.L.pgv_tile_paths_rows
    return call(env._h, c_void_p(ptr(idx)) if idx is not None else None, count, ctypes.byref(q))


@pytest.mark.parametrize("game", ["chaser", "maze"])  # chaser, easy: rows of 242 bytes, which straddle the 16-byte grid
def test_indices_and_counts(game):
    import torch
    env = settled(game)
    lay = env.path_layout
    source, probe = (GOAL, AGENT) if game in GOAL_COLS else (AGENT, CELLS)
    every_probe = [(7 * e) % lay.cells for e in range(N)]
    whole = model_of(env, game, source, probe, (0,), None, None, every_probe)
    assert_equal(ask(env, source, probe, (0,), None, None, every_probe if probe == CELLS else None), whole, "%s NULL indices" % game)
    rng = np.random.default_rng(5)
    for count in (1, 3, 5, 65, 131, 150):
        idx = rng.integers(0, N, size=count).astype(np.int32)  # with repeats
        outside = {}
        if count >= 5:
            outside = {1: -1, count - 2: N, count // 2: 2 ** 31 - 1}
            for k, v in outside.items():
                idx[k] = v
            idx[0] = idx[4]
        pc = [every_probe[i] if 0 <= i < N else 0 for i in idx]
        # one more row than asked for, behind the rows, filled with a canary
        dist = torch.full((count + 1, lay.cells), 0x5A5A, dtype=torch.int16, device=env.device)
        probe_dist = torch.full((count + 1,), -7, dtype=torch.int32, device=env.device)
        probe_step = torch.full((count + 1,), 77, dtype=torch.uint8, device=env.device)
        cells_out = torch.full((count + 1, 2), -7, dtype=torch.int32, device=env.device)
        d_idx = torch.as_tensor(idx, device=env.device)
        d_pc = torch.as_tensor(np.asarray(pc, np.int32), device=env.device)
        torch.cuda.synchronize()
        assert raw(env, count, d_idx, 1, source, probe, None, d_pc if probe == CELLS else None, dist, probe_dist, probe_step, cells_out) == 0, env.L.pgv_last_error()
        env.sync()
        got = tuple(x.cpu().numpy() for x in (dist, probe_dist, probe_step, cells_out))
        for k in range(count):
            e = int(idx[k])
            if k in outside:
                assert (got[0][k] == -1).all() and got[1][k] == -1 and got[2][k] == 0 and tuple(got[3][k]) == (-1, -1), (game, count, k)
            else:
                assert np.array_equal(got[0][k], whole.dist[e]) and got[1][k] == whole.probe_dist[e], (game, count, k)
                assert got[2][k] == whole.probe_step[e] and tuple(got[3][k]) == tuple(whole.cells[e]), (game, count, k)
        assert (got[0][count] == 0x5A5A).all() and got[1][count] == -7 and got[2][count] == 77 and (got[3][count] == -7).all(), (game, count)
        # each output alone, the others NULL
        for alone in range(4):
            outs = [dist, probe_dist, probe_step, cells_out]
            for x, fill in zip(outs, (0x5A5A, -7, 77, -7)):
                x.fill_(fill)
            torch.cuda.synchronize()
            args = [x if k == alone else None for k, x in enumerate(outs)]
            assert raw(env, count, d_idx, 1, source, probe, None, d_pc if probe == CELLS else None, *args) == 0, env.L.pgv_last_error()
            env.sync()
            again = outs[alone].cpu().numpy()
            assert np.array_equal(again, got[alone]), (game, count, alone)
    env.close()


@pytest.mark.parametrize("game", ["maze", "coinrun"])
def test_the_call_changes_nothing(game):
    import torch
    watched, plain = settled(game, 4), settled(game, 4)
    source, probe = (GOAL, AGENT) if game in GOAL_COLS else (AGENT, NONE)
    first = ask(watched, source, probe)
    assert_equal(ask(watched, source, probe), first, "%s: a second call" % game)
    for s in range(32):
        a, b = watched.step_synthetic(RUN_SEED), plain.step_synthetic(RUN_SEED)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (game, s)
        for x, y in zip(watched.state_obs(), plain.state_obs()):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (game, s)
        if s % 4 == 0:
            watched.tile_paths(KINDS[source], KINDS[probe])
    watched.close(), plain.close()


@pytest.mark.parametrize("game", ["maze", "jumper"])
def test_behind_resets_and_frameless_sequences(game):
    n = 65
    env = settled(game, 8, n)
    before = ask(env, GOAL, AGENT)
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    env.reset(mask)
    after = ask(env, GOAL, AGENT)
    assert_equal(after, model_of(env, game, GOAL, AGENT), "%s behind reset(mask)" % game)
    changed = (after[0] != before[0]).any(axis=1)
    assert changed[mask == 1].sum() >= mask.sum() - 2 and not changed[mask == 0].any()
    for call in range(3):
        env.step_sequence(steps=5, frames="none", run_seed=RUN_SEED)
        assert_equal(ask(env, GOAL, AGENT), model_of(env, game, GOAL, AGENT), "%s behind frameless sequence %d" % (game, call))
    env.close()


def test_behind_same_step_autoresets():
    import torch
    from episodes_util import synthetic_actions
    n, limit = 65, 6
    env = make("maze", n, autoreset_mode="same_step", max_episode_steps=limit)
    fields = []
    for t in range(2 * limit):
        env.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, n)))
        got = ask(env, GOAL, AGENT)
        assert_equal(got, model_of(env, "maze", GOAL, AGENT), "maze step %d" % t)
        fields.append(got[0])
    # the step that hits the limit shows the NEW episode's map: the fields (from the goal: the agent is not in them) change there
    changed = [int((fields[t] != fields[t - 1]).any(axis=1).sum()) for t in range(1, 2 * limit)]
    assert max(changed) >= n // 2 and min(changed) <= n // 8, changed
    env.close()


def test_refusals_leave_everything_as_it_was():
    import torch
    env, plain = settled("maze", 4), settled("maze", 4)
    chaser = settled("chaser", 0, 4)
    boss = make("bossfight", 4)
    lay = env.path_layout
    dist = torch.full((4, lay.cells), 0x5A5A, dtype=torch.int16, device=env.device)
    pd = torch.full((4,), -7, dtype=torch.int32, device=env.device)
    torch.cuda.synchronize()
    size = ctypes.sizeof(pglib.TilePathsStruct)
    L = env.L
    refused = [
        ("struct_size", dict(size=size - 8, dist=dist)),
        ("count", dict(count=-1, dist=dist)),
        ("source", dict(source=NONE, dist=dist)),
        ("source", dict(source=4, dist=dist)),
        ("source", dict(source=-1, dist=dist)),
        ("probe", dict(probe=4, dist=dist)),
        ("probe", dict(probe=-1, dist=dist)),
        ("source_cells", dict(source=CELLS, dist=dist)),
        ("probe_cells", dict(probe=CELLS, dist=dist)),
        ("aligned", dict(dist=dist.data_ptr() + 2)),
        ("aligned", dict(dist=dist.data_ptr() + 8)),
        ("aligned", dict(probe_dist=pd.data_ptr() + 2)),
        ("aligned", dict(cells_out=pd.data_ptr() + 1)),
        ("output", dict()),
    ]
    for word, kw in refused:
        count = kw.pop("count", 4)
        assert raw(env, count, **kw) != 0, (word, kw)
        err = L.pgv_last_error().decode()
        assert word in err and "pgv_tile_paths_rows:" in err, err
    assert L.pgv_tile_paths_rows(env._h, None, 4, None) != 0 and "NULL" in L.pgv_last_error().decode()
    assert L.pgv_tile_paths_rows(None, None, 4, None) != 0 and "NULL" in L.pgv_last_error().decode()
    for source, probe in ((GOAL, NONE), (AGENT, GOAL)):  # a game without a goal
        assert raw(chaser, 4, source=source, probe=probe, dist=torch.zeros((4, chaser.path_layout.cells), dtype=torch.int16, device=env.device)) != 0
        assert "goal" in L.pgv_last_error().decode()
    with pytest.raises(pglib.EngineError):
        chaser.tile_paths()
    assert raw(boss, 4, dist=dist) != 0 and "tile map" in L.pgv_last_error().decode()  # a game without a tile map
    assert raw(boss, 0, dist=dist) != 0
    # count = 0 succeeds and writes nothing, whatever the pointers
    assert raw(env, 0, dist=dist, probe_dist=pd) == 0 and raw(env, 0) == 0 and raw(env, 0, source=CELLS, probe=CELLS) == 0
    env.sync()
    assert (dist == 0x5A5A).all() and (pd == -7).all()
    for s in range(8):  # the engine goes on as one that was never asked
        for x, y in zip(env.step_synthetic(RUN_SEED), plain.step_synthetic(RUN_SEED)):
            assert torch.equal(x, y), s
    for e in (env, plain, chaser, boss):
        e.close()


@pytest.mark.parametrize("game", ["jumper", "chaser"])
def test_the_host_form(game):
    env = settled(game)
    lay = env.path_layout
    source = GOAL if game in GOAL_COLS else AGENT
    idx = np.array([5, 0, 130, -1, 5, 131, 64], np.int32)
    k = idx.size
    pc = np.array([0, lay.cells - 1, 17, 3, -1, 0, lay.cells], np.int32)
    want = ask(env, source, CELLS, (0,), idx, None, pc)
    raw_dist = np.full(k * lay.cells + 1, 0x5A5A, np.int16)
    h_dist = raw_dist[1:].reshape(k, lay.cells)  # (a host buffer off the 16-byte grid is fine)
    h_pd, h_ps, h_cells = np.full(k, -7, np.int32), np.full(k, 77, np.uint8), np.full((k, 2), -7, np.int32)
    assert raw(env, k, idx, 1, source, CELLS, None, pc, h_dist, h_pd, h_ps, h_cells, host=True) == 0, env.L.pgv_last_error()
    assert_equal((h_dist, h_pd, h_ps, h_cells), want, "%s host form" % game)
    assert raw_dist[0] == 0x5A5A
    # NULL indices, the probe distances alone
    h_pd[:] = -7
    assert raw(env, k, None, 1, source, AGENT, probe_dist=h_pd, host=True) == 0, env.L.pgv_last_error()
    assert np.array_equal(h_pd, ask(env, source, AGENT)[1][:k])
    assert raw(env, 0, host=True) == 0 and raw(env, k, host=True) != 0 and raw(env, -1, probe_dist=h_pd, host=True) != 0
    assert raw(env, k, source=CELLS, probe_dist=h_pd, host=True) != 0 and "pgv_tile_paths_rows_host:" in env.L.pgv_last_error().decode()
    env.close()


def test_the_maze_law_on_the_engine():
    """tile_paths → MAZE_STEP_ACTIONS → step, nothing copied to the host inside the loop: every env's first done arrives at
    its reset-time probe_dist (a distance of 0: at step 1) with reward 10."""
    import torch
    env = make("maze")
    table = torch.tensor(procgen2_amd.MAZE_STEP_ACTIONS, dtype=torch.int32, device=env.device)
    d0 = env.tile_paths().probe_dist.clone()
    assert (d0 >= 0).all()
    due = torch.where(d0 >= 1, d0, torch.ones_like(d0))
    steps = int(due.max())
    first_done = torch.zeros_like(d0)
    first_reward = torch.zeros((N,), dtype=torch.float32, device=env.device)
    on_course = torch.ones((N,), dtype=torch.bool, device=env.device)
    for t in range(1, steps + 1):
        paths = env.tile_paths(dist=False)
        live = first_done == 0
        on_course &= ~live | (paths.probe_dist == torch.clamp(d0 - (t - 1), min=0))
        _, reward, done = env.step(table[paths.probe_step.long()])
        now = live & (done != 0)
        first_done = torch.where(now, torch.full_like(first_done, t), first_done)
        first_reward = torch.where(now, reward, first_reward)
    assert torch.equal(first_done, due), "first dones at %s, the field said %s" % (first_done.tolist(), due.tolist())
    assert (first_reward == 10.0).all() and on_course.all()
    assert steps >= 40, "short mazes only: %d" % steps
    env.close()


@pytest.mark.parametrize("game", ["caveflyer", "coinrun"])
def test_python_surface(game):
    import torch
    from procgen2_amd.vec_env import TilePaths
    n = 9
    env = settled(game, 2, n)
    lay = env.path_layout
    assert lay == pglib.path_layout(env.L, game, env.distribution_mode) == pglib.path_layout(env.L, game)
    assert lay.cells == env.state_layout.cells and lay.has_goal == (game in GOAL_COLS)
    source = "goal" if lay.has_goal else "agent"
    res = env.tile_paths(source)
    assert isinstance(res, TilePaths)
    for x, dtype, shape in ((res.dist, torch.int16, (n, lay.cells)), (res.probe_dist, torch.int32, (n,)), (res.probe_step, torch.uint8, (n,)),
                            (res.cells, torch.int32, (n, 2))):
        assert x.dtype == dtype and tuple(x.shape) == shape and x.device == env.device and x.is_contiguous()
    assert env.tile_paths(source, dist=False).dist is None
    assert tuple(env.tile_paths(source, envs=[]).dist.shape) == (0, lay.cells)
    as_list = env.tile_paths(source, envs=[4, 4, 8, -1])
    as_tensor = env.tile_paths(source, envs=torch.tensor([4, 4, 8, -1], device=env.device))
    for name in ("dist", "probe_dist", "probe_step", "cells"):
        assert torch.equal(getattr(as_list, name), getattr(as_tensor, name)), name
        assert torch.equal(getattr(as_list, name)[:3], getattr(res, name)[[4, 4, 8]]), name
    assert (as_list.dist[3] == -1).all() and as_list.cells[3].tolist() == [-1, -1]
    out = torch.full((n, lay.cells), 7, dtype=torch.int16, device=env.device)
    back = env.tile_paths(source, out=out)
    assert back.dist is out and torch.equal(out, res.dist)
    for bad in (torch.zeros((n, lay.cells + 1), dtype=torch.int16, device=env.device),
                torch.zeros((n, lay.cells), dtype=torch.int32, device=env.device), torch.zeros((n, lay.cells), dtype=torch.int16)):
        with pytest.raises(ValueError):
            env.tile_paths(source, out=bad)
    for kw in (dict(source="none"), dict(source="cheese"), dict(probe="mouse"), dict(source=source, out=out, dist=False)):
        with pytest.raises(ValueError):
            env.tile_paths(**kw)
    env.close()
