"""Assigned levels (include/procgen2_vec.h pgv_assign_levels): the reference model the tests hold the engine to, and the
schedule of assignments the lock-step tests run.

The model is the semantics of the header written down in Python on top of SINGLE oracle envs (oracle/pgo_api.cpp pgo_make /
pgo_present / pgo_step / pgo_reset), one per env of the batch:

  * a level with a number — level-seed mode, or an assigned level — is a fresh `pgo_make(game, number)` whose level 0 is
    presented: fresh containers, fresh camera, rng.seed(number);
  * a free-mode level is `pgo_reset(h, 0, 0)` on the env as it stands: its stream and containers go on — also after an
    assigned level, whose env is then simply the one made with that number;
  * one pending assignment per env, consumed by the next level the env builds (auto-reset, or a reset without seeds),
    overwritten by a later one, dropped by a reset with seeds; it takes no place in the env's own sequence (k stays).

tests/test_assign_levels.py holds the model itself to the oracle's vector (OracleVec) where the two overlap.
"""
import ctypes

import numpy as np

from oracle_util import OBS_BYTES, oracle, oracle_state, register_textures, _dump
from test_levels import level_number, mix32

# the step counts and the action stream of tests/test_levels.py::test_engine_level_mode_matches_oracle
GAME_STEPS = [("coinrun", 300), ("maze", 520), ("bossfight", 250), ("climber", 250), ("caveflyer", 250), ("chaser", 200),
              ("jumper", 250)]
RUN_SEED = 11


def actions_of(step, n):
    L = oracle()
    return np.array([L.pgo_synthetic_action(RUN_SEED, step, e) for e in range(n)], np.int32)


class AssignModel:
    """N envs with the engine's auto-reset policy, level set and assignments; after construction every env has had its
    first reset (as OracleVec has)."""

    def __init__(self, game, n, seed_base=1, num_levels=0, start_level=0):
        register_textures(game)
        self.L = oracle()
        self.game, self.n = game, n
        self.num_levels, self.start_level = num_levels, start_level
        self.h = [self.L.pgo_make(game.encode(), (seed_base + i) & 0xFFFFFFFF, 1) for i in range(n)]  # level 0, never observed
        self.chain_seed = [(seed_base + i) & 0xFFFFFFFF for i in range(n)]
        self.drawn = [1 if num_levels > 0 else 0] * n  # (the engine's make draws a number for its hidden level too)
        self.assigned = [None] * n
        self.pending_reset = [False] * n
        self.level_numbers = np.zeros(n, np.uint32)
        self.level_known = np.zeros(n, np.uint8)
        self.obs = np.zeros((n, OBS_BYTES), np.uint8)
        self.reward = np.zeros(n, np.float32)
        self.done = np.zeros(n, np.uint8)
        self.assigned_by_reset = 0  # assigned levels installed by an explicit reset / by an auto-reset
        self.assigned_by_auto = 0
        for i in range(n):
            self._new_level(i, False, 0)
        self.assigned_by_reset = 0

    def _remake(self, i, number):
        self.L.pgo_close(self.h[i])
        self.h[i] = self.L.pgo_make(self.game.encode(), number, 1)
        self.L.pgo_present(self.h[i])

    def _new_level(self, i, restart, seed, auto=False):
        if restart:  # a reset with seeds: the env's own sequence starts over, a pending assignment is dropped
            self.chain_seed[i], self.drawn[i] = seed & 0xFFFFFFFF, 0
            self.assigned[i] = None
        if self.assigned[i] is not None:
            number, self.assigned[i] = self.assigned[i], None
            self._remake(i, number)
            self.level_numbers[i], self.level_known[i] = number, 1
            if auto:
                self.assigned_by_auto += 1
            else:
                self.assigned_by_reset += 1
        elif self.num_levels > 0:
            number = level_number(self.num_levels, self.start_level, self.chain_seed[i], self.drawn[i])
            self.drawn[i] += 1
            self._remake(i, number)
            self.level_numbers[i], self.level_known[i] = number, 1
        else:
            self.L.pgo_reset(self.h[i], 1 if restart else 0, ctypes.c_int32(seed & 0xFFFFFFFF).value if restart else 0)
            self.level_numbers[i], self.level_known[i] = 0, 0
        self._row(i)

    def _row(self, i):
        self.obs[i] = np.ctypeslib.as_array(self.L.pgo_obs(self.h[i]), shape=(OBS_BYTES,))

    def assign(self, indices, levels):
        for i, number in zip(indices, levels):
            if 0 <= int(i) < self.n:
                self.assigned[int(i)] = int(number) & 0xFFFFFFFF

    def reset(self, mask=None, seeds=None):
        for i in range(self.n):
            if mask is not None and not mask[i]:
                continue
            self._new_level(i, seeds is not None, int(seeds[i]) if seeds is not None else 0)
            self.reward[i], self.done[i], self.pending_reset[i] = 0.0, 0, False
        return self.obs

    def reset_obs(self):
        return self.obs

    def first_reset(self):
        """The first reset after make: the model had it when it was made, its frames stand."""
        return self.obs

    def step(self, actions):
        for i in range(self.n):
            if self.pending_reset[i]:
                self._new_level(i, False, 0, auto=True)
                self.reward[i], self.done[i], self.pending_reset[i] = 0.0, 0, False
            else:
                self.L.pgo_step(self.h[i], int(actions[i]))
                self.reward[i] = self.L.pgo_reward(self.h[i])
                self.done[i] = self.L.pgo_terminated(self.h[i])
                self.pending_reset[i] = bool(self.done[i])
                self._row(i)
        return self.obs, self.reward, self.done

    def state(self, i):
        return oracle_state(self.h[i])

    def tiles(self, i):
        return _dump(lambda buf, m: self.L.pgo_dump_tiles(self.h[i], buf, m), ctypes.c_uint8, np.uint8)

    def close(self):
        for h in self.h:
            self.L.pgo_close(h)
        self.h = []


# ---------------------------------------------------------------------------------------------------------------------
# The lock-step schedule: which env is assigned what, and when.  A function of (env, how many assignments the env has had)
# alone, so the model on the CPU and the engine on the GPU are driven by one script.
# ---------------------------------------------------------------------------------------------------------------------
EARLY, LATE, TWICE, DROPPED = 2, 3, 4, 5  # env index mod 6; 0 and 1: never named (a third of the batch)


def scheduled_level(env, count):
    """The count-th level assigned to env: a few dozen distinct numbers, every seventh one with the top bit set (a level
    number is a 32-bit pattern)."""
    number = 1000 + mix32(env * 7919 + count) % 40
    return (number | 0x80000000) if (env + count) % 7 == 0 else number


class Schedule:
    """Call after_reset(envs) with the envs whose reset frame has just been shown and after_done(envs) with those that have
    just reported done; each returns (indices, levels) lists of the assignment calls to make now, in order."""

    def __init__(self, n):
        self.count = [0] * n

    def _next(self, env):
        self.count[env] += 1
        return scheduled_level(env, self.count[env])

    def after_reset(self, envs):
        calls = []
        first = [e for e in envs if e % 6 in (EARLY, TWICE, DROPPED)]
        if first:
            calls.append((first, [self._next(e) for e in first]))
        again = [e for e in envs if e % 6 == TWICE]  # overwritten before use
        if again:
            calls.append((again, [self._next(e) for e in again]))
        return calls

    def after_done(self, envs):
        late = [e for e in envs if e % 6 == LATE]  # the step before the reset: the level is generated inside the step
        return [(late, [self._next(e) for e in late])] if late else []


def run_schedule(vec, assign, steps, n, check=None):
    """The lock-step script: the first reset, `steps` steps of test_levels.py's action stream with the schedule's assignments
    between them, a masked reset WITHOUT seeds at a third (it consumes pending assignments) and a masked reseeding reset at
    two thirds (it drops them).  vec: AssignModel, or an engine with the same first_reset / reset / step; assign(indices, levels) makes
    one assignment call; check(what) is called after every reset and step."""
    sched = Schedule(n)
    everyone = list(range(n))

    def make(calls):
        for indices, levels in calls:
            assign(indices, levels)

    vec.first_reset()
    if check:
        check("first reset")
    make(sched.after_reset(everyone))
    pending = np.zeros(n, bool)
    for s in range(steps):
        _, _, done = vec.step(actions_of(s, n))
        if check:
            check("step %d" % s)
        make(sched.after_reset([e for e in everyone if pending[e]]))
        pending = np.asarray(done).astype(bool).copy()
        make(sched.after_done([e for e in everyone if pending[e]]))
        if s == steps // 3:
            mask = (np.arange(n) % 4 == 2).astype(np.uint8)
            vec.reset(mask=mask)
            if check:
                check("masked reset without seeds")
            pending &= mask == 0
            make(sched.after_reset([e for e in everyone if mask[e]]))
        if s == 2 * steps // 3:
            mask = (np.arange(n) % 3 == 2).astype(np.uint8)
            seeds = (np.arange(n, dtype=np.int32) % 4) - 1
            vec.reset(mask=mask, seeds=seeds)
            if check:
                check("masked reseeding reset")
            pending &= mask == 0
            make(sched.after_reset([e for e in everyone if mask[e]]))
