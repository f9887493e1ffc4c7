"""The model of the engine's policy-ready observations (include/procgen2_vec.h pgv_policy_obs_enable) in pure numpy: the
value and gray rules as bit patterns, the frame stack with its restart flags, and drivers that compose it with the models of
the calls that push (OracleVec, SequenceModel, EpisodeModel).  The GPU tests trust this model, not the engine;
tests/test_policy_obs.py holds the model itself to independent formulations (torch on the CPU, a deque per env).

A driver sets a restart flag where the engine's contract says one is set: from the `done` row as each (sub-)step finds it,
from reset masks, from a same-step reset's `ended`, from loads.  Only a push that touches the env clears it.
"""
import numpy as np

from episodes_util import SAME_STEP, EpisodeModel
from oracle_util import OracleVec
from sequence_util import SequenceModel

DTYPES = {"uint8": np.uint8, "float16": np.uint16, "bfloat16": np.uint16, "float32": np.uint32}  # name → the bit pattern's type


def value_table(dtype):
    """The 256 output bit patterns of a dtype name."""
    v = np.arange(256, dtype=np.uint8)
    if dtype == "uint8":
        return v
    f = v.astype(np.float32) / np.float32(255)  # one correctly rounded IEEE division
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)  # numpy rounds to nearest even
    assert dtype == "bfloat16"
    u = f.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def gray(obs):
    """y = (77 R + 150 G + 29 B + 128) >> 8 of frames [..., 3], in integers."""
    o = obs.astype(np.uint32)
    return ((77 * o[..., 0] + 150 * o[..., 1] + 29 * o[..., 2] + 128) >> 8).astype(np.uint8)


def transform(obs, gray_rule, dtype):
    """Frames u8 [N, 12288] or [N, 64, 64, 3] → bit patterns [N, C, 64, 64]."""
    o = np.asarray(obs, np.uint8).reshape(-1, 64, 64, 3)
    planes = gray(o)[:, None] if gray_rule else o.transpose(0, 3, 1, 2)
    return value_table(dtype)[planes]


class PolicyStack:
    """[n, K*C, 64, 64] bit patterns, slot 0 the oldest frame, and the pending restart flags."""

    def __init__(self, n, K, gray_rule, dtype, restart=1):
        self.n, self.K, self.C, self.gray, self.dtype = n, K, 1 if gray_rule else 3, bool(gray_rule), dtype
        self.out = np.zeros((n, K * self.C, 64, 64), DTYPES[dtype])
        self.restart = np.full(n, restart, np.uint8)  # (enable sets every flag)

    def flag(self, where):
        """where: a mask [n] (non-zero = set), or None = all."""
        self.restart[:] = 1 if where is None else self.restart | (np.asarray(where) != 0)

    def push(self, frame, mask=None):
        new = transform(frame, self.gray, self.dtype)
        touched = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        fresh = touched & (self.restart != 0)
        moved = touched & ~fresh
        C = self.C
        self.out[moved, :-C] = self.out[moved, C:]
        self.out[moved, -C:] = new[moved]
        self.out[fresh] = np.tile(new[fresh], (1, self.K, 1, 1))
        self.restart[touched] = 0
        return self.out


class PolicyVec:
    """OracleVec + the stack: pgv_reset and pgv_step on an engine with policy observations."""

    def __init__(self, game, n, K, gray_rule, dtype, seed_base=1, enabled=True, env_offset=0):
        self.o = OracleVec(game, n, seed_base=seed_base, env_offset=env_offset)  # (env_offset=a: rows [a, a + n) of a larger engine)
        self.env_offset = env_offset
        self.n = n
        self.stack = PolicyStack(n, K, gray_rule, dtype) if enabled else None
        self.args = (n, K, gray_rule, dtype)

    obs = property(lambda self: self.o.obs)
    out = property(lambda self: self.stack.out)
    restart = property(lambda self: self.stack.restart)

    def enable(self):
        self.stack = PolicyStack(*self.args)

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
        if self.stack is not None:
            self.stack.flag(mask)
            self.stack.push(self.o.obs, mask)
        return self.o.obs

    def step(self, actions, push=True):
        if self.stack is not None:
            self.stack.flag(self.o.done)  # the done row as the step finds it
        res = self.o.step(actions)
        if self.stack is not None and push:
            self.stack.push(self.o.obs)
        return res

    def close(self):
        self.o.close()


class PolicySequence:
    """SequenceModel + the stack: pgv_step_sequence."""

    def __init__(self, game, n, K, gray_rule, dtype):
        self.m = SequenceModel(game, n)
        self.stack = PolicyStack(n, K, gray_rule, dtype)
        self.flagged_inside = self.flagged_last = 0

    obs = property(lambda self: self.m.obs)

    def first_reset(self):
        self.m.first_reset()
        self.m.o.reward[:] = 0.0
        self.m.o.done[:] = 0
        self.stack.flag(None)
        self.stack.push(self.m.obs)

    def sequence(self, actions, frames_last=True, draw=None):
        """frames_last: PGV_FRAMES_LAST (the call pushes).  draw: whether the model draws the last sub-step (default: as
        frames_last) — True with frames_last False is what pgv_render_obs(NULL) leaves afterwards, and push() then what
        pgv_policy_obs_push(NULL) does."""
        T = len(actions)
        before = self.m.o.done.copy()
        self.m.sequence(actions, draw_last=frames_last if draw is None else draw)
        found = np.vstack([before[None], self.m.dones[:T - 1]]) != 0  # the done row as sub-step t finds it
        self.stack.flag(found.any(axis=0))
        if frames_last:
            self.stack.push(self.m.obs)

    def push(self):
        self.stack.push(self.m.obs)

    def close(self):
        self.m.close()


class PolicyEpisodes:
    """EpisodeModel + the stack: pgv_step_episodes."""

    def __init__(self, game, n, mode, K, gray_rule, dtype, max_episode_steps=0, final_capacity=0):
        self.m = EpisodeModel(game, n, mode, max_episode_steps, final_capacity)
        self.stack = PolicyStack(n, K, gray_rule, dtype)
        self.mode = mode

    obs = property(lambda self: self.m.obs)

    def first_reset(self):
        self.m.first_reset()
        self.m.o.reward[:] = 0.0
        self.m.o.done[:] = 0
        self.stack.flag(None)
        self.stack.push(self.m.obs)

    def step(self, actions):
        self.stack.flag(self.m.engine_done)
        self.m.step(actions)
        if self.mode == SAME_STEP:
            self.stack.flag(self.m.ended)
        self.stack.push(self.m.obs)

    def close(self):
        self.m.close()
