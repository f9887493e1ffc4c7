"""The model of the engine's frame history (include/procgen2_vec.h pgv_history_enable) in pure numpy: the ring of planar u8
frames with its began bytes and pending flags, a plain-Python gather that follows point 6 of the header literally, and
drivers that compose the ring with the models of the calls that push (OracleVec, SequenceModel, EpisodeModel).  The values
and the gray rule are tests/policy_obs_util.py's.  The GPU tests trust this model, not the engine; tests/test_history.py holds
it to the PolicyStack of the policy observations (the law that ties the two features) and the walk to a deque per env
(tests/cpp/test_history.cpp).

A driver sets a pending flag where the engine's contract says one is set: from the `done` row as each (sub-)step finds it,
from reset masks, from a same-step reset's `ended`, from loads.  `Frames` carries the ring and, optionally, a PolicyStack fed
by the same events, for the law.
"""
import numpy as np

from episodes_util import SAME_STEP, EpisodeModel
from oracle_util import OracleVec
from policy_obs_util import DTYPES, PolicyStack, gray, value_table
from sequence_util import SequenceModel


# The GPU tests' sizes (tests/test_history_gpu.py): two wavefronts of envs plus a ragged tail; a ring that wraps eight times.
N, T, CALLS, RUN_SEED = 131, 5, 40, 7
# … and their episode runs (game, autoreset mode, step limit): tests/test_history.py counts what they reach on the oracle.
EPISODE_RUNS = [("maze", SAME_STEP, 3), ("bossfight", SAME_STEP, 3), ("maze", "next_step", 0), ("bossfight", "next_step", 0)]


def planes(obs, gray_rule):
    """Frames u8 [N, 12288] or [N, 64, 64, 3] → the stored planes u8 [N, C, 64, 64]."""
    o = np.asarray(obs, np.uint8).reshape(-1, 64, 64, 3)
    return gray(o)[:, None] if gray_rule else np.ascontiguousarray(o.transpose(0, 3, 1, 2))


class HistoryRing:
    def __init__(self, n, T, gray_rule, frames=None):
        self.n, self.T, self.gray, self.C = n, T, bool(gray_rule), 1 if gray_rule else 3
        self.frames = np.zeros((T, n, self.C, 64, 64), np.uint8) if frames is None else frames
        self.began = np.zeros((T, n), np.uint8)
        self.pending = np.ones(n, np.uint8)  # (enable sets every flag)
        self.head = 0

    def flag(self, where):
        """where: a mask [n] (non-zero = set), or None = all."""
        self.pending[:] = 1 if where is None else self.pending | (np.asarray(where) != 0)

    def push(self, frame):
        """Point 2: all envs into a new slot."""
        slot = self.head % self.T
        self.frames[slot] = planes(frame, self.gray)
        self.began[slot] = self.pending
        self.pending[:] = 0
        self.head += 1

    def reset(self, frame, mask=None):
        """Point 5: pgv_reset rewrites the named envs' rows of the newest slot (slot 0, opened, where there is none)."""
        if self.head == 0:
            self.head = 1
        slot = (self.head - 1) % self.T
        named = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.frames[slot][named] = planes(frame, self.gray)[named]
        self.began[slot][named] = 1
        self.pending[named] = 0

    def held(self, p):
        return self.head - self.T <= p < self.head and p >= 0

    def walk(self, p, i, K):
        """Point 6: the frames f_0 .. f_(K-1) of the entry (p, i), p held."""
        f = [p]
        for j in range(1, K):
            last = f[-1]
            f.append(last if self.began[last % self.T][i] or not self.held(last - 1) else last - 1)
        return f

    def gather(self, pushes, envs, K, dtype):
        """Bit patterns [B, K*C, 64, 64]: row slot K-1-j is frame f_j; zeros where p is not held or the env is outside."""
        table, C = value_table(dtype), self.C
        out = np.zeros((len(pushes), K * C, 64, 64), DTYPES[dtype])
        for b, (p, i) in enumerate(zip(pushes, envs)):
            p, i = int(p), int(i)
            if not self.held(p) or not 0 <= i < self.n:
                continue
            for j, f in enumerate(self.walk(p, i, K)):
                out[b, (K - 1 - j) * C:(K - j) * C] = table[self.frames[f % self.T][i]]
        return out

    def newest(self, K, dtype):
        """gather(head - 1, every env): what the law holds against pgv_policy_obs."""
        return self.gather([self.head - 1] * self.n, range(self.n), K, dtype)


class Frames:
    """The ring and, with policy=(K, dtype), a PolicyStack beside it — both fed by the same events."""

    def __init__(self, n, T, gray_rule, policy=None, ring=True):
        self.args = (n, T, gray_rule)
        self.ring = HistoryRing(n, T, gray_rule) if ring else None
        self.stack = PolicyStack(n, policy[0], gray_rule, policy[1]) if policy else None

    def enable_ring(self):
        self.ring = HistoryRing(*self.args)

    def flag(self, where):
        if self.ring is not None:
            self.ring.flag(where)
        if self.stack is not None:
            self.stack.flag(where)

    def push(self, frame):
        if self.ring is not None:
            self.ring.push(frame)
        if self.stack is not None:
            self.stack.push(frame)

    def reset(self, frame, mask=None):
        if self.ring is not None:
            self.ring.reset(frame, mask)
        if self.stack is not None:
            self.stack.flag(mask)
            self.stack.push(frame, mask)


class HistoryVec:
    """OracleVec + the ring: pgv_reset and pgv_step."""

    def __init__(self, game, n, T, gray_rule, policy=None, ring=True, seed_base=1, env_offset=0):
        self.o = OracleVec(game, n, seed_base=seed_base, env_offset=env_offset)  # (env_offset=a: rows [a, a + n) of a larger engine)
        self.env_offset = env_offset
        self.n = n
        self.f = Frames(n, T, gray_rule, policy, ring)

    obs = property(lambda self: self.o.obs)
    ring = property(lambda self: self.f.ring)
    stack = property(lambda self: self.f.stack)

    def first_reset(self):
        """The engine's first full pgv_reset after make: an OracleVec had it when it was made."""
        self.o.reset_obs()
        return self._reset_done(None)

    def reset(self, mask=None):
        self.o.reset(mask=mask)
        return self._reset_done(mask)

    def _reset_done(self, mask):
        named = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.o.reward[named] = 0.0
        self.o.done[named] = 0
        self.f.reset(self.o.obs, mask)
        return self.o.obs

    def step(self, actions):
        self.f.flag(self.o.done)  # the done row as the step finds it
        res = self.o.step(actions)
        self.f.push(self.o.obs)
        return res

    def close(self):
        self.o.close()


class HistorySequence:
    """SequenceModel + the ring: pgv_step_sequence."""

    def __init__(self, game, n, T, gray_rule, policy=None):
        self.m = SequenceModel(game, n)
        self.f = Frames(n, T, gray_rule, policy)

    obs = property(lambda self: self.m.obs)
    ring = property(lambda self: self.f.ring)
    stack = property(lambda self: self.f.stack)

    def first_reset(self):
        self.m.first_reset()
        self.m.o.reward[:] = 0.0
        self.m.o.done[:] = 0
        self.f.reset(self.m.obs)

    def sequence(self, actions, frames_last=True, draw=None):
        """frames_last: PGV_FRAMES_LAST (the call pushes).  draw: whether the model draws the last sub-step (default: as
        frames_last) — True with frames_last False is what pgv_render_obs(NULL) leaves afterwards, and push() then what
        pgv_history_push does."""
        T = len(actions)
        before = self.m.o.done.copy()
        self.m.sequence(actions, draw_last=frames_last if draw is None else draw)
        found = np.vstack([before[None], self.m.dones[:T - 1]]) != 0  # the done row as sub-step t finds it
        self.f.flag(found.any(axis=0))
        if frames_last:
            self.f.push(self.m.obs)

    def push(self):
        self.f.push(self.m.obs)

    def close(self):
        self.m.close()


class HistoryEpisodes:
    """EpisodeModel + the ring: pgv_step_episodes."""

    def __init__(self, game, n, mode, T, gray_rule, policy=None, max_episode_steps=0):
        self.m = EpisodeModel(game, n, mode, max_episode_steps, 0)
        self.f = Frames(n, T, gray_rule, policy)
        self.mode = mode

    obs = property(lambda self: self.m.obs)
    ring = property(lambda self: self.f.ring)
    stack = property(lambda self: self.f.stack)

    def first_reset(self):
        self.m.first_reset()
        self.m.o.reward[:] = 0.0
        self.m.o.done[:] = 0
        self.f.reset(self.m.obs)

    def step(self, actions):
        self.f.flag(self.m.engine_done)
        self.m.step(actions)
        if self.mode == SAME_STEP:
            self.f.flag(self.m.ended)
        self.f.push(self.m.obs)

    def close(self):
        self.m.close()


def cut_and_wrapped(ring, K):
    """Over every held push and env: how many K-stacks were cut by a began byte (the walk stopped on a set byte with frames
    held in front of it), and how many crossed the slot wrap (hold a push of slot 0 and the push in front of it, of slot T-1)."""
    cut = wrapped = 0
    for p in range(max(0, ring.head - ring.T), ring.head):
        for i in range(ring.n):
            f = ring.walk(p, i, K)
            distinct = sorted(set(f))
            oldest = distinct[0]
            if len(distinct) < K and ring.began[oldest % ring.T][i] and ring.held(oldest - 1):
                cut += 1
            if any(x % ring.T == 0 and x - 1 in distinct for x in distinct):
                wrapped += 1
    return cut, wrapped
