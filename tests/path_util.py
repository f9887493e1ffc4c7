"""Shared by test_tile_paths.py (CPU) and test_tile_paths_gpu.py: the model the path distances (include/procgen2_vec.h
pgv_tile_paths_rows) are held to.  A plain queue BFS over the oracle's tiles() and state(), with the cell rule, the table of
agent offsets, the goal's columns and the step-code rule written out again here — nothing of the engine's code is used.
The runs are state_obs_util.oracle_run's: 131 envs, 96 steps, checkpoints 0, 1, 8, 16, …
"""
import collections
import functools
import math

import numpy as np

from state_obs_util import FIXED_RECORD, oracle_run

NONE, AGENT, GOAL, CELLS = 0, 1, 2, 3
TILE_GAMES = ("coinrun", "maze", "climber", "caveflyer", "chaser", "jumper")
# the centre of the agent's body box is (agent_x, agent_y + AGENT_DY): oracle/pgo_*.cpp, the agents' bounds
AGENT_DY = {"maze": 0.0, "chaser": 0.0, "caveflyer": 0.0, "coinrun": -0.5, "climber": -0.5, "jumper": -0.4}
# the state columns of the goal's point; caveflyer: x and y of record 0 (alive kind x y vel_x vel_y), entity 0 being the goal
GOAL_COLS = {"maze": (3, 4), "jumper": (18, 19), "caveflyer": (FIXED_RECORD["caveflyer"][0] + 2, FIXED_RECORD["caveflyer"][0] + 3)}
MAZE_STEP_ACTIONS = (4, 1, 7, 3, 5)  # step code → maze action: stay, x-1, x+1, world up, world down

Model = collections.namedtuple("Model", "dist probe_dist probe_step cells")


def cell_of(wx, wy, tile_w, tile_h):
    """The cell of a world point, -1 where it has none: x = floor(wx), y = tile_h - 1 - floor(wy)."""
    wx, wy = float(wx), float(wy)
    if math.isnan(wx) or math.isnan(wy) or math.isinf(wx) or math.isinf(wy):
        return -1
    x, y = math.floor(wx), tile_h - 1 - math.floor(wy)
    if not (0 <= x < tile_w and 0 <= y < tile_h):
        return -1
    return y + x * tile_h


def agent_cell(game, state, tile_w, tile_h):
    return cell_of(state[0], np.float32(state[1]) + np.float32(AGENT_DY[game]), tile_w, tile_h)  # one float32 addition


def goal_cell(game, state, tile_w, tile_h):
    gx, gy = GOAL_COLS[game]
    if gy >= state.size:  # (caveflyer without entities)
        return -1
    return cell_of(state[gx], state[gy], tile_w, tile_h)


def bfs(tiles, tile_w, tile_h, source, passable):
    """int16 [cells]: the source 0 whatever its tile; d + 1 for a passable cell not yet reached with a 4-neighbour at d; no
    wrap; -1 elsewhere.  passable: a set of tile ids (ids >= 32 never count)."""
    dist = [-1] * (tile_w * tile_h)
    if source >= 0:
        may = [t < 32 and t in passable for t in range(256)]
        ok = [may[t] for t in np.asarray(tiles, np.uint8).tolist()]
        dist[source] = 0
        queue = collections.deque([source])
        while queue:
            c = queue.popleft()
            x, y = divmod(c, tile_h)
            d = dist[c] + 1
            if x > 0 and ok[c - tile_h] and dist[c - tile_h] < 0:
                dist[c - tile_h] = d
                queue.append(c - tile_h)
            if x < tile_w - 1 and ok[c + tile_h] and dist[c + tile_h] < 0:
                dist[c + tile_h] = d
                queue.append(c + tile_h)
            if y > 0 and ok[c - 1] and dist[c - 1] < 0:
                dist[c - 1] = d
                queue.append(c - 1)
            if y < tile_h - 1 and ok[c + 1] and dist[c + 1] < 0:
                dist[c + 1] = d
                queue.append(c + 1)
    return np.array(dist, np.int16)


def probe_of(dist, tile_w, tile_h, probe):
    """(distance at the probe cell, step code): 0 where the distance is <= 0, else the first of x-1 (1), x+1 (2), y-1 (3),
    y+1 (4) whose distance is one less."""
    if probe < 0:
        return -1, 0
    d = int(dist[probe])
    if d <= 0:
        return d, 0
    x, y = divmod(probe, tile_h)
    for code, inside, c in ((1, x > 0, probe - tile_h), (2, x < tile_w - 1, probe + tile_h), (3, y > 0, probe - 1),
                            (4, y < tile_h - 1, probe + 1)):
        if inside and int(dist[c]) == d - 1:
            return d, code
    raise AssertionError("a reached cell at distance %d without a nearer neighbour" % d)


def point_cell(game, kind, state, tile_w, tile_h, given):
    if kind == AGENT:
        return agent_cell(game, state, tile_w, tile_h)
    if kind == GOAL:
        return goal_cell(game, state, tile_w, tile_h)
    if kind == CELLS:
        return int(given) if 0 <= int(given) < tile_w * tile_h else -1
    return -1


def model_rows(game, states, tiles, tile_w, tile_h, source, probe, passable, source_cells=None, probe_cells=None):
    """The four outputs for rows whose envs have the dumps `states` / `tiles` (a None entry: an env outside the batch)."""
    passable = set(int(t) for t in passable)
    cells = tile_w * tile_h
    B = len(states)
    out = Model(np.full((B, cells), -1, np.int16), np.full(B, -1, np.int32), np.zeros(B, np.uint8), np.full((B, 2), -1, np.int32))
    for k, (st, tl) in enumerate(zip(states, tiles)):
        if st is None:
            continue
        s = point_cell(game, source, st, tile_w, tile_h, None if source_cells is None else source_cells[k])
        p = point_cell(game, probe, st, tile_w, tile_h, None if probe_cells is None else probe_cells[k])
        out.dist[k] = bfs(tl, tile_w, tile_h, s, passable)
        out.probe_dist[k], out.probe_step[k] = probe_of(out.dist[k], tile_w, tile_h, p)
        out.cells[k] = (s, p)
    return out


@functools.lru_cache(maxsize=None)
def model_at(game, mode, step, tile_w, tile_h, source, probe, passable=(0,), n_steps=None):
    """The model over every env of oracle_run(game, mode) at checkpoint `step`; made once and kept unchanged.  n_steps: the
    (steps, every) of a shorter run, as test_state_obs_gpu.py's other modes use."""
    at, _ = oracle_run(game, mode) if n_steps is None else oracle_run(game, mode, 131, n_steps[0], n_steps[1])
    sample = at[step]
    res = model_rows(game, sample.states, sample.tiles, tile_w, tile_h, source, probe, passable)
    for a in res:
        a.setflags(write=False)
    return res


def manhattan(tile_w, tile_h, source):
    """int16 [cells]: |dx| + |dy| from the source cell (every cell passable), all -1 without one."""
    if source < 0:
        return np.full(tile_w * tile_h, -1, np.int16)
    sx, sy = divmod(source, tile_h)
    x, y = np.divmod(np.arange(tile_w * tile_h), tile_h)
    return (np.abs(x - sx) + np.abs(y - sy)).astype(np.int16)
