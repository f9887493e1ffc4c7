"""Caller-made levels, the part that needs no GPU (include/procgen2_vec.h pgv_level_layout_of, pgv_get_levels,
pgv_set_levels): the layout query and its refusals, the exported symbols and the structs as the header lays them out, and
the yardstick of the GPU tests — custom_levels_util.MazeModel, one maze step in numpy — held bit for bit to the CPU oracle on
the oracle's own levels in all three modes; the share of reachable goals among the random maps the GPU tests install."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import procgen2_amd
from custom_levels_util import (AX, AY, BACKGROUNDS, FORWARD, MODES, MODE_NAMES, OTHER_GAMES, SIDE, STATUS, STEPS, MazeModel, oracle_dumps,
                                oracle_levels, random_levels)

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pgv_level_layout_of", "pgv_get_levels", "pgv_set_levels", "pgv_get_levels_host", "pgv_set_levels_host")


def _error(L):
    return (L.pgv_last_error() or b"").decode()


def _layout(L, gid, mode):
    out = pglib.LevelLayoutStruct(ctypes.sizeof(pglib.LevelLayoutStruct))
    assert L.pgv_level_layout_of(gid, mode, ctypes.byref(out)) == 0, _error(L)
    return out


def test_level_layout(engine_lib):
    L = engine_lib
    maze = L.pgv_game_id(b"maze")
    assert L.pgv_game_modes(maze) == sum(1 << m for m in MODES)
    for mode in MODES:
        lay = _layout(L, maze, mode)
        assert (lay.supported, lay.cells, lay.tile_w, lay.tile_h, lay.backgrounds) == (1, SIDE[mode] ** 2, SIDE[mode], SIDE[mode], BACKGROUNDS)
        state = pglib.state_layout(L, "maze", mode)
        assert (lay.cells, lay.tile_w, lay.tile_h) == (state.cells, state.tile_w, state.tile_h)
        assert pglib.level_layout(L, "maze", mode) == (True, lay.cells, lay.tile_w, lay.tile_h, BACKGROUNDS)
    default = _layout(L, maze, 0)  # PGV_MODE_DEFAULT is the mode the game is compiled with: hard
    assert (default.supported, default.cells, default.tile_w, default.tile_h) == (1, 625, 25, 25)
    assert [SIDE[m] for m in (1, 2, 3)] == [15, 25, 31]
    for game in OTHER_GAMES:
        gid = L.pgv_game_id(game.encode())
        for mode in range(5):
            if mode and not (L.pgv_game_modes(gid) >> mode) & 1:
                continue
            lay = _layout(L, gid, mode)
            assert (lay.supported, lay.cells, lay.tile_w, lay.tile_h, lay.backgrounds) == (0, 0, 0, 0, 0), (game, mode)
        assert not pglib.level_layout(L, game).supported


def test_refusals(engine_lib):
    L = engine_lib
    out = pglib.LevelLayoutStruct(ctypes.sizeof(pglib.LevelLayoutStruct))
    maze, chaser = L.pgv_game_id(b"maze"), L.pgv_game_id(b"chaser")
    for gid, mode, word in ((maze, 4, "mode"), (chaser, 3, "mode"), (maze, 9, "mode"), (maze, -1, "mode"), (7, 0, "game"), (-1, 0, "game")):
        assert L.pgv_level_layout_of(gid, mode, ctypes.byref(out)) != 0, (gid, mode)
        assert word in _error(L) and "pgv_level_layout_of" in _error(L), _error(L)
    small = pglib.LevelLayoutStruct(ctypes.sizeof(pglib.LevelLayoutStruct) - 4)
    assert L.pgv_level_layout_of(maze, 0, ctypes.byref(small)) != 0 and "struct_size" in _error(L)
    assert small.cells == 0 and small.supported == 0
    assert L.pgv_level_layout_of(maze, 0, None) != 0 and "NULL" in _error(L)
    # a NULL env, for the four row calls (nothing is touched: the buffers need not exist)
    rows = pglib.level_rows()
    for name in NEW_SYMBOLS[1:]:
        assert getattr(L, name)(None, None, 1, ctypes.byref(rows)) != 0, name
        assert name + ":" in _error(L) and "NULL" in _error(L), _error(L)


def test_symbols_are_declared_and_bound(engine_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "procgen2_vec.h")).read()
    for name in NEW_SYMBOLS:
        assert "PGV_API" in header and (" " + name + "(") in header, name
        assert name in pglib.EXPORTED_VEC_SYMBOLS, name
        assert getattr(engine_lib, name).argtypes is not None, name
    for libname in ("libprocgen2_hip.so", "libMaze.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(pglib.LIB_DIR, libname)], capture_output=True, text=True, check=True).stdout
        assert set(NEW_SYMBOLS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}, libname
    for name, k in (("PGV_LEVEL_INSTALLED", 0), ("PGV_LEVEL_NO_ENV", 1), ("PGV_LEVEL_BAD_TILE", 2), ("PGV_LEVEL_BAD_AGENT", 3),
                    ("PGV_LEVEL_BAD_GOAL", 4), ("PGV_LEVEL_BAD_FLOOR", 5)):
        assert "#define %s %d" % (name, k) in header
    assert pglib.LEVEL_STATUS == STATUS and procgen2_amd.LEVEL_STATUS == tuple(STATUS) and pglib.LEVEL_KNOWN_CUSTOM == 2
    # the structs as the header lays them out: a C program that includes it says the sizes and offsets
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "procgen2_vec.h"\n'
                   "#define O(s, f) printf(\"%zu \", offsetof(s, f))\n"
                   "int main(void) {\n"
                   "  O(pgv_level_layout, struct_size); O(pgv_level_layout, supported); O(pgv_level_layout, cells); O(pgv_level_layout, tile_w);\n"
                   "  O(pgv_level_layout, tile_h); O(pgv_level_layout, backgrounds); printf(\"%zu\\n\", sizeof(pgv_level_layout));\n"
                   "  O(pgv_level_rows, struct_size); O(pgv_level_rows, tiles); O(pgv_level_rows, agent_cell); O(pgv_level_rows, goal_cell);\n"
                   "  O(pgv_level_rows, background); O(pgv_level_rows, background_shift); O(pgv_level_rows, ids); O(pgv_level_rows, status);\n"
                   "  printf(\"%zu\\n\", sizeof(pgv_level_rows));\n  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for S, line in zip((pglib.LevelLayoutStruct, pglib.LevelRowsStruct), lines):
        assert [int(x) for x in line.split()] == [getattr(S, f).offset for f, _ in S._fields_] + [ctypes.sizeof(S)], S.__name__
    assert ctypes.sizeof(pglib.LevelLayoutStruct) == 24 and ctypes.sizeof(pglib.LevelRowsStruct) == 64


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_model_against_the_oracle(mode):
    """The numpy step on the oracle's own levels: 65 envs, 300 random-action steps, the model fed from the oracle's dumps at
    every episode start.  Rewards, dones, the agent's position, agent_forward and steps, bit for bit, at every step — and
    the whole state row with them."""
    n, steps = 65, 300
    o, levels = oracle_levels(mode, n, seed_base=11)
    states, tiles = oracle_dumps(o)
    model = MazeModel(mode, levels)
    assert np.array_equal(model.rows.view(np.uint32), states.view(np.uint32)), "the installed rows are the oracle's reset rows"
    assert np.array_equal(model.tiles, tiles)
    rng = np.random.default_rng(mode)
    resets = np.zeros(n, bool)  # the envs whose next step serves their reset
    episodes = goals = moved = 0
    for s in range(steps):
        actions = rng.integers(0, 15, n)
        _, reward, done = o.step(actions)
        want_reward, want_done = model.step(actions, ~resets)
        if resets.any():  # an episode start: the model takes the oracle's new level
            fresh = np.nonzero(resets)[0]
            st, tl = oracle_dumps(o, fresh)
            model.load(fresh, st, tl)
        assert np.array_equal(reward.view(np.uint32), want_reward.view(np.uint32)), "reward, step %d" % s
        assert np.array_equal(done, want_done), "done, step %d" % s
        st, tl = oracle_dumps(o)
        for col in (AX, AY, FORWARD, STEPS):
            assert np.array_equal(st[:, col].view(np.uint32), model.rows[:, col].view(np.uint32)), "column %d, step %d" % (col, s)
        assert np.array_equal(st.view(np.uint32), model.rows.view(np.uint32)), "state rows, step %d" % s
        assert np.array_equal(tl, model.tiles)
        episodes += int(done.sum())
        goals += int((reward > 0).sum())
        moved += int((st[:, STEPS] > 0).sum())
        resets = done != 0
    o.close()
    assert moved > 0 and (goals > 0 or mode != 1), "the run must mean something: %d episodes, %d goals" % (episodes, goals)


def test_model_reaches_the_step_cap():
    """500 steps against a wall: done at step 500 and not before, reward 0; the oracle's envs do the same (action 4 stays)."""
    o, levels = oracle_levels(2, 3, seed_base=5)
    model = MazeModel(2, levels)
    for s in range(1, 501):
        actions = np.full(3, 4)
        _, reward, done = o.step(actions)
        want_reward, want_done = model.step(actions)
        assert np.array_equal(done, want_done) and np.array_equal(reward, want_reward) and not reward.any()
        assert done.all() == (s == 500) and done.any() == (s == 500)
    o.close()


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_random_maps_have_both_kinds_of_rows(mode):
    """The maps the GPU tests install: between 25 % and 90 % of the goals are reachable, so neither branch there is vacuous;
    open cells on the world border, which the generator never makes, are among them."""
    levels, reachable = random_levels(mode, 131)
    share = reachable.mean()
    print("mode %s: %d of 131 goals reachable" % (MODE_NAMES[mode], reachable.sum()))
    assert 0.25 <= share <= 0.90, share
    side = SIDE[mode]
    border = np.zeros((side, side), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    assert (levels.tiles[:, border.reshape(-1)] == 0).any(axis=1).all()
    x, y = np.divmod(levels.agent_cell, side)
    assert ((x == 0) | (x == side - 1) | (y == 0) | (y == side - 1)).any(), "an agent next to the edge"
    assert (levels.tiles[np.arange(131), levels.agent_cell] == 0).all() and (levels.tiles[np.arange(131), levels.goal_cell] == 0).all()
    assert (levels.agent_cell != levels.goal_cell).all() and set(np.unique(levels.tiles)) == {0, 1}
    assert ((levels.background >= 0) & (levels.background < BACKGROUNDS)).all()
    assert ((levels.background_shift >= 0) & (levels.background_shift < 1)).all()
    again, _ = random_levels(mode, 131)
    assert all(np.array_equal(a, b) for a, b in zip(levels, again))
