"""Shared by test_state_obs.py (CPU) and test_state_obs_gpu.py: the oracle run the symbolic observations are held to, the
layout constants the oracle's dumps imply, and the comparison of device rows with oracle dumps.

The run: 131 envs (two wavefronts and a ragged three), seed_base 1, synthetic actions with run_seed 2, 96 steps, dumps
after the reset, after step 1 and after every 8th step.  Every game finishes episodes inside it, and the games with records
show many row lengths.  One oracle run per (game, mode, n, steps) is made and kept unchanged for every test that asks.
"""
import functools

import numpy as np

from oracle_util import OracleVec

EASY, HARD, MEMORY, EXTREME = 1, 2, 3, 4
# game → (default mode, every mode it offers): the engine's (game, mode) table
TABLE = {
    "coinrun": (HARD, (EASY, HARD)),
    "maze": (HARD, (EASY, HARD, MEMORY)),
    "bossfight": (HARD, (EASY, HARD)),
    "climber": (HARD, (EASY, HARD)),
    "caveflyer": (HARD, (EASY, HARD, MEMORY)),
    "chaser": (EASY, (EASY, HARD, EXTREME)),
    "jumper": (HARD, (EASY, HARD, MEMORY)),
}
GAMES = tuple(TABLE)
MODE_NAMES = {EASY: "easy", HARD: "hard", MEMORY: "memory", EXTREME: "extreme"}
NON_DEFAULT = tuple((g, m) for g, (d, ms) in TABLE.items() for m in ms if m != d)
# game → (fixed, record): the floats every dump has, the floats per variable record behind them
FIXED_RECORD = {"coinrun": (14, 5), "maze": (10, 0), "bossfight": (313, 0), "climber": (14, 6), "caveflyer": (141, 6),
                "chaser": (13, 8), "jumper": (51, 2)}
VARIABLE = ("coinrun", "climber", "caveflyer", "jumper")  # the games whose rows have many lengths in the run

N, SEED_BASE, RUN_SEED, STEPS, EVERY = 131, 1, 2, 96, 8


def checkpoints(steps=STEPS, every=EVERY):
    """The steps after which the run is sampled: 0 is the reset."""
    return [0, 1] + list(range(every, steps + 1, every))


class Sample:
    """The oracle's dumps of every env at one point of a run."""

    def __init__(self, o):
        self.states = [o.state(e) for e in range(o.n)]
        self.tiles = [o.tiles(e) for e in range(o.n)]


@functools.lru_cache(maxsize=None)
def oracle_run(game, mode=0, n=N, steps=STEPS, every=EVERY):
    """{step: Sample} at the checkpoints, and the step at which the oracle first set a `done` (None: never).  Drawing is
    off: the logic does not depend on it."""
    o = OracleVec(game, n, seed_base=SEED_BASE, render=False, mode=mode)
    at, first_done = {0: Sample(o)}, None
    marks = set(checkpoints(steps, every))
    for s in range(1, steps + 1):
        _, _, done = o.step(None, run_seed=RUN_SEED)
        if first_done is None and done.any():
            first_done = s
        if s in marks:
            at[s] = Sample(o)
    o.close()
    return at, first_done


def assert_rows(rows, lengths, tiles, states, tile_dumps, what):
    """Device rows (numpy: float32 [B, width], int32 [B], uint8 [B, cells]) against the oracle's dumps of the same envs:
    the length, the dump bit for bit, zero bits behind it, the tile bytes."""
    bits = np.ascontiguousarray(rows).view(np.uint32)
    assert rows.shape[0] == lengths.shape[0] == tiles.shape[0] == len(states), what
    for k, (st, tl) in enumerate(zip(states, tile_dumps)):
        L = int(lengths[k])
        assert L == st.size, "%s row %d: length %d, the oracle's dump has %d" % (what, k, L, st.size)
        assert np.array_equal(bits[k, :L], st.view(np.uint32)), "%s row %d: state" % (what, k)
        assert not bits[k, L:].any(), "%s row %d: not +0.0 behind the dump" % (what, k)
        assert tiles.shape[1] == tl.size and np.array_equal(tiles[k], tl), "%s row %d: tiles" % (what, k)


class FakeStateEngine:
    """The adapter's engine contract with state_obs / tile_obs, on the CPU: numpy rows that count the calls, so that a test
    can tell which call an info came from."""

    def __init__(self, n=5, width=7, cells=6):
        self.num_envs, self.width, self.cells, self.calls = n, width, cells, 0
        self.obs = np.zeros((n, 64, 64, 3), np.uint8)

    def reset(self, mask=None, seeds=None):
        self.calls += 1
        return self.obs

    def step(self, actions):
        self.calls += 1
        done = np.zeros(self.num_envs, np.uint8)
        done[0] = self.calls % 2  # (same_step mode then resets env 0 on every other step)
        return self.obs, np.zeros(self.num_envs, np.float32), done

    def state_obs(self, envs=None, out=None, lengths_out=None):
        assert envs is None
        out = np.zeros((self.num_envs, self.width), np.float32) if out is None else out
        lengths_out = np.zeros(self.num_envs, np.int32) if lengths_out is None else lengths_out
        out[:] = self.calls
        lengths_out[:] = self.width - 1
        return out, lengths_out

    def tile_obs(self, envs=None, out=None):
        assert envs is None
        out = np.zeros((self.num_envs, self.cells), np.uint8) if out is None else out
        out[:] = self.calls
        return out

    def close(self):
        pass
