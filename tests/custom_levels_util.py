"""Shared by test_custom_levels.py (CPU) and test_custom_levels_gpu.py: what caller-made levels (include/procgen2_vec.h
pgv_get_levels / pgv_set_levels) are held to.

* MazeModel: one maze step in numpy, a restatement of the game's step — movement, the box test, the 500-step cap, reward and
  done — over any tile maps.  test_custom_levels.py holds it to the CPU oracle on the oracle's own levels, bit for bit; the
  GPU tests then use it on maps the generator never makes.  Nothing of the engine's code is used.
* levels_of: the levels of oracle envs as values, from their dumps, by the cell rule written out again here.
* random_levels: independent wall draws, a random open agent cell, a random open goal cell, and which rows' goals a queue BFS
  (path_util.bfs) reaches.
"""
import collections

import numpy as np

from oracle_util import OracleVec
from path_util import bfs

EASY, HARD, MEMORY = 1, 2, 3
MODES = (EASY, HARD, MEMORY)
MODE_NAMES = {EASY: "easy", HARD: "hard", MEMORY: "memory"}
SIDE = {EASY: 15, HARD: 25, MEMORY: 31}   # the world is SIDE x SIDE cells
FOLLOWS = {EASY: False, HARD: False, MEMORY: True}  # the camera follows the agent (else it rests on the world centre)
BACKGROUNDS = 9
TIMEOUT = 500
OTHER_GAMES = ("coinrun", "bossfight", "climber", "caveflyer", "chaser", "jumper")
STATUS = {"installed": 0, "no_env": 1, "bad_tile": 2, "bad_agent": 3, "bad_goal": 4, "bad_floor": 5}
KNOWN_CUSTOM = 2
# the columns of a maze state row (the oracle's dump)
AX, AY, FORWARD, GX, GY, STEPS, FLOOR, SHIFT, CAMX, CAMY = range(10)
RANDOM_SEED = 7       # random_levels' draws in the GPU tests: test_custom_levels.py asserts the share of reachable goals it gives
DENSITY = 0.3

f32 = np.float32
Levels = collections.namedtuple("Levels", "tiles agent_cell goal_cell background background_shift")


def cell_of(wx, wy, side):
    """The cell of a world point inside the map: x = floor(wx), y = side - 1 - floor(wy), cell = y + x * side."""
    x, y = np.floor(wx).astype(np.int64), side - 1 - np.floor(wy).astype(np.int64)
    assert ((x >= 0) & (x < side) & (y >= 0) & (y < side)).all()
    return (y + x * side).astype(np.int32)


def point_of(cell, side):
    """The world point on the centre of a cell: (x + 0.5, side - 1 - y + 0.5), float32."""
    x, y = np.divmod(np.asarray(cell, np.int64), side)
    return x.astype(f32) + f32(0.5), (side - 1 - y).astype(f32) + f32(0.5)


def levels_of_dumps(states, tiles, side):
    """Levels from state rows (float32 [B, 10]) and tile rows (uint8 [B, side * side])."""
    states = np.asarray(states, f32)
    return Levels(np.ascontiguousarray(tiles, np.uint8), cell_of(states[:, AX], states[:, AY], side), cell_of(states[:, GX], states[:, GY], side),
                  states[:, FLOOR].astype(np.int32), states[:, SHIFT].copy())


def oracle_dumps(o, envs=None):
    envs = range(o.n) if envs is None else envs
    return np.stack([o.state(e) for e in envs]), np.stack([o.tiles(e) for e in envs])


class MazeModel:
    """B mazes over caller-given maps, in numpy: state rows as the oracle dumps them, steps as the game takes them."""

    def __init__(self, mode, levels):
        self.side, self.follows = SIDE[mode], FOLLOWS[mode]
        self.tiles = np.array(levels.tiles, np.uint8)
        self.n = self.tiles.shape[0]
        assert self.tiles.shape == (self.n, self.side * self.side)
        self.rows = np.zeros((self.n, 10), f32)
        self.install(np.arange(self.n), levels)

    def install(self, envs, levels):
        """The rows of `levels` become the levels of the envs `envs`: the start of an episode."""
        envs = np.asarray(envs, np.int64)
        r = self.rows
        self.tiles[envs] = levels.tiles
        r[envs, AX], r[envs, AY] = point_of(levels.agent_cell, self.side)
        r[envs, GX], r[envs, GY] = point_of(levels.goal_cell, self.side)
        r[envs, FORWARD], r[envs, STEPS] = 1.0, 0.0
        r[envs, FLOOR], r[envs, SHIFT] = np.asarray(levels.background, f32), np.asarray(levels.background_shift, f32)
        r[envs, CAMX] = r[envs, CAMY] = f32(self.side) * f32(0.5) * f32(16.0)

    def load(self, envs, states, tiles):
        """The oracle's dumps become the state of the envs `envs`."""
        self.rows[envs] = states
        self.tiles[envs] = tiles

    def _tile(self, x, y):
        side = self.side
        inside = (x >= 0) & (x < side) & (y >= 0) & (y < side)
        at = np.where(inside, y + x * side, 0)
        return np.where(inside, self.tiles[np.arange(self.n), at], 1)

    def step(self, actions, envs=None):
        """One step of every env (or of the envs whose entry of `envs` is true; the others keep their rows and report 0, 0):
        (reward float32 [B], done uint8 [B])."""
        a = np.asarray(actions, np.int64)
        r, side = self.rows.copy(), self.side
        ax, ay = r[:, AX], r[:, AY]
        mx = a // 3 - 1
        my = np.where(mx != 0, 0, -(a % 3 - 1))
        # (int)(ax + mx): one float32 addition, truncated towards zero
        nx = np.trunc(ax + mx.astype(f32)).astype(np.int64)
        ny = np.trunc(ay + my.astype(f32)).astype(np.int64)
        cx, cy = np.trunc(ax).astype(np.int64), np.trunc(ay).astype(np.int64)
        go_x = (mx != 0) & (self._tile(nx, side - 1 - cy) == 0)
        go_y = (mx == 0) & (my != 0) & (self._tile(cx, side - 1 - ny) == 0)
        ax = np.where(go_x, nx.astype(f32) + f32(0.5), ax).astype(f32)
        ay = np.where(go_y, ny.astype(f32) + f32(0.5), ay).astype(f32)
        half, one = f32(-0.5), f32(1.0)
        bx, by, qx, qy = ax + half, ay + half, r[:, GX] + half, r[:, GY] + half
        reached = (bx < qx + one) & (bx + one > qx) & (by < qy + one) & (by + one > qy)  # strict overlap of two unit boxes
        r[:, AX], r[:, AY] = ax, ay
        r[:, FORWARD] = np.where(mx > 0, 1.0, np.where(mx < 0, 0.0, r[:, FORWARD]))
        r[:, STEPS] += 1.0
        if self.follows:
            r[:, CAMX], r[:, CAMY] = ax * f32(16.0), ay * f32(16.0)
        reward = np.where(reached, f32(10.0), f32(0.0)).astype(f32)
        done = (reached | (r[:, STEPS] >= TIMEOUT)).astype(np.uint8)
        if envs is not None:
            envs = np.asarray(envs, bool)
            r[~envs] = self.rows[~envs]
            reward[~envs], done[~envs] = 0.0, 0
        self.rows = r
        return reward, done


def random_levels(mode, count, seed=RANDOM_SEED, density=DENSITY):
    """(Levels, reachable bool [count]): every cell a wall with probability `density`, independently — border cells included,
    which the generator never opens; the agent on a random open cell, the goal on another.  reachable: the goal's distance
    from the agent over open cells, by a queue BFS, is not -1."""
    side = SIDE[mode]
    rng = np.random.default_rng([seed, mode])
    tiles = (rng.random((count, side * side)) < density).astype(np.uint8)
    agent, goal = np.zeros(count, np.int32), np.zeros(count, np.int32)
    reachable = np.zeros(count, bool)
    for k in range(count):
        open_cells = np.nonzero(tiles[k] == 0)[0]
        agent[k], goal[k] = rng.choice(open_cells, 2, replace=False)
        reachable[k] = bfs(tiles[k], side, side, int(agent[k]), {0})[goal[k]] >= 0
    return Levels(tiles, agent, goal, rng.integers(0, BACKGROUNDS, count).astype(np.int32), rng.random(count).astype(f32)), reachable


def oracle_levels(mode, n, seed_base, render=False):
    """(OracleVec after its reset, Levels of its envs at that reset)."""
    o = OracleVec("maze", n, seed_base=seed_base, render=render, mode=mode)
    o.reset()
    return o, levels_of_dumps(*oracle_dumps(o), SIDE[mode])


def status_of(levels, indices, n, side):
    """The status pgv_set_levels gives every row (numpy fields; indices None: row k into env k), the first code that applies:
    1 no such env, 2 a tile byte that is neither 0 nor 1, 3 / 4 the agent's / the goal's cell outside the map or on a wall (or
    the goal on the agent), 5 a background outside 0 .. BACKGROUNDS - 1 or a shift outside [0, 1) — NaN included."""
    tiles = np.asarray(levels.tiles)
    rows, cells = np.arange(tiles.shape[0]), side * side
    idx = rows if indices is None else np.asarray(indices, np.int64)
    agent, goal = np.asarray(levels.agent_cell, np.int64), np.asarray(levels.goal_cell, np.int64)
    agent_in, goal_in = (agent >= 0) & (agent < cells), (goal >= 0) & (goal < cells)
    shift = np.asarray(levels.background_shift, f32)
    background = np.asarray(levels.background, np.int64)
    status = np.zeros(rows.size, np.int32)
    status[(background < 0) | (background >= BACKGROUNDS) | ~((shift >= 0) & (shift < 1))] = STATUS["bad_floor"]
    status[~goal_in | (tiles[rows, np.where(goal_in, goal, 0)] != 0) | (goal == agent)] = STATUS["bad_goal"]
    status[~agent_in | (tiles[rows, np.where(agent_in, agent, 0)] != 0)] = STATUS["bad_agent"]
    status[(tiles > 1).any(axis=1)] = STATUS["bad_tile"]
    status[(idx < 0) | (idx >= n)] = STATUS["no_env"]
    return status
