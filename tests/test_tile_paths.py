"""Path distances (include/procgen2_vec.h pgv_tile_paths_rows), the part that needs no GPU: the row routine of
procgen2_amd/csrc/pg_paths.h compiled for the CPU (tests/cpp/test_tile_paths.cpp), pgv_path_layout_of against the table of
the specification, the refusals, the exported symbols and the bindings — and the rule itself held to the oracle with the
model of tests/path_util.py: the agent's centre cell is free, the goal's cell is free and reached, and in maze the policy
read off the field ends every episode in exactly as many steps as the field says."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import procgen2_amd
from oracle_util import OracleVec
from path_util import (AGENT, AGENT_DY, GOAL, GOAL_COLS, MAZE_STEP_ACTIONS, TILE_GAMES, agent_cell, bfs, goal_cell, model_at,
                       model_rows)
from state_obs_util import GAMES, MODE_NAMES, TABLE, oracle_run

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pgv_tile_paths_rows", "pgv_tile_paths_rows_host", "pgv_path_layout_of")
EVERY_MODE = tuple((g, m) for g in TILE_GAMES for m in TABLE[g][1])


def _error(L):
    return (L.pgv_last_error() or b"").decode()


def _layout(L, game, mode):
    out = pglib.PathLayoutStruct(ctypes.sizeof(pglib.PathLayoutStruct))
    assert L.pgv_path_layout_of(L.pgv_game_id(game.encode()), mode, ctypes.byref(out)) == 0, _error(L)
    return out


def test_pg_paths_on_the_host(tmp_path):
    """pg_paths.h under g++, 64 emulated lanes: path_row and path_probe against a queue BFS over random boards of every
    size, the open boards from each corner, a source in a wall, an empty passable set; the cell rule."""
    exe = str(tmp_path / "test_tile_paths")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_tile_paths.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK random boards", "OK open boards", "OK special cases", "OK cells", "ALL OK"):
        assert section in out.stdout, section


@pytest.mark.parametrize("game", GAMES)
def test_path_layout(engine_lib, game):
    L = engine_lib
    default, modes = TABLE[game]
    for mode in (0,) + tuple(modes):
        lay = _layout(L, game, mode)
        state = pglib.state_layout(L, game, mode)
        assert (lay.cells, lay.tile_w, lay.tile_h) == (state.cells, state.tile_w, state.tile_h), (game, mode)
        assert lay.agent_dx == 0.0
        if game == "bossfight":
            assert (lay.cells, lay.has_goal, lay.agent_dy) == (0, 0, 0.0)
        else:
            assert lay.cells > 0 and lay.tile_w <= 64 and lay.tile_h <= 64, (game, mode)
            assert np.float32(lay.agent_dy) == np.float32(AGENT_DY[game]), (game, mode)
            assert lay.has_goal == (1 if game in GOAL_COLS else 0), (game, mode)
        if mode == 0:  # PGV_MODE_DEFAULT is the mode the game is compiled with
            named = _layout(L, game, default)
            assert all(getattr(lay, f) == getattr(named, f) for f, _ in pglib.PathLayoutStruct._fields_), game
        got = pglib.path_layout(L, game, mode)
        assert got == (lay.cells, lay.tile_w, lay.tile_h, bool(lay.has_goal), lay.agent_dx, lay.agent_dy)
    assert {g for g in GAMES if _layout(L, g, 0).has_goal} == {"maze", "jumper", "caveflyer"}


def test_refusals(engine_lib):
    L = engine_lib
    out = pglib.PathLayoutStruct(ctypes.sizeof(pglib.PathLayoutStruct))
    maze, chaser = L.pgv_game_id(b"maze"), L.pgv_game_id(b"chaser")
    for gid, mode, word in ((maze, 4, "mode"), (chaser, 3, "mode"), (maze, 9, "mode"), (maze, -1, "mode"), (7, 0, "game"), (-1, 0, "game")):
        assert L.pgv_path_layout_of(gid, mode, ctypes.byref(out)) != 0, (gid, mode)
        assert word in _error(L) and "pgv_path_layout_of" in _error(L), _error(L)
    small = pglib.PathLayoutStruct(ctypes.sizeof(pglib.PathLayoutStruct) - 4)
    assert L.pgv_path_layout_of(maze, 0, ctypes.byref(small)) != 0 and "struct_size" in _error(L)
    assert small.cells == 0
    assert L.pgv_path_layout_of(maze, 0, None) != 0 and "NULL" in _error(L)
    # a NULL env, for the two row calls (nothing is touched: the buffers need not exist)
    q = pglib.TilePathsStruct(ctypes.sizeof(pglib.TilePathsStruct), 1, 1)
    for name in ("pgv_tile_paths_rows", "pgv_tile_paths_rows_host"):
        assert getattr(L, name)(None, None, 1, ctypes.byref(q)) != 0, name
        assert name + ":" in _error(L) and "NULL" in _error(L), _error(L)


def test_symbols_are_declared_and_bound(engine_lib):
    header = open(os.path.join(ROOT, "include", "procgen2_vec.h")).read()
    for name in NEW_SYMBOLS:
        assert (" " + name + "(") in header, name
        assert name in pglib.EXPORTED_VEC_SYMBOLS, name
        assert getattr(engine_lib, name).argtypes is not None, name
    for libname in ("libprocgen2_hip.so", "libMaze.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pglib.LIB_DIR, libname)], capture_output=True, text=True, check=True).stdout
        assert set(NEW_SYMBOLS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, libname
    assert "typedef struct pgv_tile_paths {" in header and "typedef struct pgv_path_layout {" in header
    for k, name in enumerate(("PGV_PATH_NONE", "PGV_PATH_AGENT", "PGV_PATH_GOAL", "PGV_PATH_CELLS")):
        assert "#define %s %d" % (name, k) in header
    assert pglib.PATH_POINTS == {"none": 0, "agent": 1, "goal": 2, "cells": 3}
    # the structs as the header lays them out (LP64)
    S = pglib.TilePathsStruct
    assert [f for f, _ in S._fields_] == ["struct_size", "passable", "source", "source_cells", "probe", "probe_cells", "dist",
                                          "probe_dist", "probe_step", "cells_out"]
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64] and ctypes.sizeof(S) == 72
    P = pglib.PathLayoutStruct
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16, 20, 24] and ctypes.sizeof(P) == 28
    assert procgen2_amd.MAZE_STEP_ACTIONS == (4, 1, 7, 3, 5) == MAZE_STEP_ACTIONS
    assert pglib.passable_mask((0,)) == 1 and pglib.passable_mask(()) == 0 and pglib.passable_mask([0, 2, 31]) == 0x80000005
    assert pglib.passable_mask(0xFFFFFFFF) == 0xFFFFFFFF
    for bad in ((32,), (-1,), 2 ** 32, -1):
        with pytest.raises(ValueError):
            pglib.passable_mask(bad)


@pytest.mark.parametrize("game,mode", EVERY_MODE, ids=["%s-%s" % (g, MODE_NAMES[m]) for g, m in EVERY_MODE])
def test_the_rule_on_the_oracle(engine_lib, game, mode):
    """The model and the specification, no engine: the agent's centre cell is inside the map and free (id 0) in every sample
    — but for at most 2 per coinrun run (measured: 1 of 1 834, a crate) — and where there is a goal, its cell is free and
    the agent reaches it over free cells, in every sample."""
    lay = _layout(engine_lib, game, mode)
    w, h = lay.tile_w, lay.tile_h
    at, _ = oracle_run(game, mode)
    samples = occupied = 0
    for step, sample in sorted(at.items()):
        goal_model = model_at(game, mode, step, w, h, GOAL, AGENT) if game in GOAL_COLS else None
        for e, (st, tl) in enumerate(zip(sample.states, sample.tiles)):
            a = agent_cell(game, st, w, h)
            assert 0 <= a < lay.cells, (game, mode, step, e)
            samples += 1
            occupied += int(tl[a] != 0)
            if goal_model is not None:
                g = goal_cell(game, st, w, h)
                assert 0 <= g < lay.cells and tl[g] == 0, (game, mode, step, e)
                assert tuple(goal_model.cells[e]) == (g, a)
                assert goal_model.probe_dist[e] >= 0, "%s mode %d step %d env %d: the agent does not reach the goal" % (game, mode, step, e)
                assert (goal_model.probe_step[e] == 0) == (goal_model.probe_dist[e] == 0)
    assert samples == 131 * len(at)
    assert occupied <= (2 if game == "coinrun" else 0), "%s mode %d: %d of %d agent cells are not free" % (game, mode, occupied, samples)


@pytest.mark.parametrize("mode", TABLE["maze"][1], ids=[MODE_NAMES[m] for m in TABLE["maze"][1]])
def test_the_maze_law_on_the_oracle(engine_lib, mode):
    """33 mazes, seed_base 1: play MAZE_STEP_ACTIONS[step code] of the model (source = goal, probe = agent).  An env whose
    distance at reset is d >= 1 reports its first done at step d with reward 10.0; a d = 0 env at step 1."""
    n = 33
    lay = _layout(engine_lib, "maze", mode)
    w, h = lay.tile_w, lay.tile_h
    o = OracleVec("maze", n, seed_base=1, render=False, mode=mode)
    first = model_rows("maze", [o.state(e) for e in range(n)], [o.tiles(e) for e in range(n)], w, h, GOAL, AGENT, (0,))
    d0 = first.probe_dist.astype(np.int64)
    assert (d0 >= 0).all()
    due = np.where(d0 >= 1, d0, 1)
    done_at = np.zeros(n, np.int64)
    for t in range(1, int(due.max()) + 1):
        live = [e for e in range(n) if not done_at[e]]
        m = model_rows("maze", [o.state(e) for e in live], [o.tiles(e) for e in live], w, h, GOAL, AGENT, (0,))
        actions = np.full(n, MAZE_STEP_ACTIONS[0], np.int32)
        for k, e in enumerate(live):
            assert m.probe_dist[k] == max(int(d0[e]) - (t - 1), 0), "env %d step %d: the field does not fall by one a step" % (e, t)
            actions[e] = MAZE_STEP_ACTIONS[m.probe_step[k]]
        _, reward, done = o.step(actions)
        for e in live:
            if done[e]:
                assert t == due[e] and reward[e] == 10.0, "env %d: done at step %d with reward %r, the field said %d" % (e, t, reward[e], due[e])
                done_at[e] = t
            else:
                assert t < due[e], "env %d: no done at step %d, the field said %d" % (e, t, due[e])
    o.close()
    assert (done_at == due).all()
    assert d0.max() >= {1: 20, 2: 40, 3: 60}[mode], "short mazes only: %d" % d0.max()


def test_model_is_a_bfs():
    """The model's own sanity: an open board is the Manhattan distance; a wall splits it; the source counts whatever it is."""
    w, h = 5, 4
    tiles = np.zeros(w * h, np.uint8)
    d = bfs(tiles, w, h, 0, {0}).reshape(w, h)
    assert all(d[x, y] == x + y for x in range(w) for y in range(h))
    tiles.reshape(w, h)[2, :] = 1  # a wall column
    d = bfs(tiles, w, h, 0, {0}).reshape(w, h)
    assert (d[:2] >= 0).all() and (d[2:] == -1).all()
    d = bfs(tiles, w, h, 2 * h + 1, {0}).reshape(w, h)  # from inside the wall: both sides
    assert d[2, 1] == 0 and d[1, 1] == 1 and d[3, 1] == 1 and d[2, 0] == -1 and d[4, 3] == 4
    assert (bfs(tiles, w, h, -1, {0}) == -1).all()
    assert (bfs(np.full(w * h, 40, np.uint8), w, h, 3, set(range(64))) == np.where(np.arange(w * h) == 3, 0, -1)).all()
