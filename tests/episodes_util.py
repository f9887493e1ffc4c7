"""The model of the engine's episode bookkeeping (include/procgen2_vec.h pgv_step_episodes): an OracleVec plus numpy
counters.  OracleVec.step and OracleVec.reset(mask) are the whole specification of the games; what is added here is the
caller's loop the engine call stands for:

    next_step:  step(actions); an env whose `done` row was set before the step is on its reset step and is not counted.
    same_step:  step(actions); count; ended = done | (length == T); keep the terminal rows and frames; reset(mask = ended).

Returns are accumulated in np.float32, one addition a step.  Level words: the tests run in free mode (num_levels = 0),
where every level has number 0 and known 0.
"""
import numpy as np

from oracle_util import OBS_BYTES, OracleVec, oracle

NEXT_STEP, SAME_STEP = "next_step", "same_step"


def synthetic_actions(run_seed, step, n, env_offset=0):
    """pgo_synthetic_action(run_seed, step, env) for every env, computed on the host."""
    L = oracle()
    return np.array([L.pgo_synthetic_action(run_seed, step, env_offset + i) for i in range(n)], np.int32)


class EpisodeModel:
    def __init__(self, game, n, mode, max_episode_steps=0, final_capacity=0, seed_base=1, distribution_mode=0, render=True,
                 env_offset=0, threads=1):
        """`mode` is the autoreset mode; `distribution_mode` (0: the game's default) is OracleVec's `mode`.  render=False: the
        counters alone (the frames are then meaningless).  env_offset=a: the model of rows [a, a + n) of a larger engine
        (`ended_env` and the ring stay the slice's own: rows 0 .. n-1); threads: OracleVec's."""
        assert mode in (NEXT_STEP, SAME_STEP)
        self.o = OracleVec(game, n, seed_base=seed_base, mode=distribution_mode, render=render, env_offset=env_offset, threads=threads)
        self.env_offset = env_offset
        self.n, self.mode, self.T, self.capacity = n, mode, int(max_episode_steps), int(final_capacity)
        self.running_return = np.zeros(n, np.float32)
        self.running_length = np.zeros(n, np.int32)
        self.longest = 0  # the longest episode seen so far

    # the engine's own rows
    obs = property(lambda self: self.o.obs)
    engine_reward = property(lambda self: self.o.reward)
    engine_done = property(lambda self: self.o.done)

    def first_reset(self):
        """The engine's first reset() after make: an OracleVec had it when it was made."""
        return self.o.reset_obs()

    def reset(self, mask=None):
        self.o.reset(mask=mask)
        named = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.o.reward[named] = 0.0  # (what pgv_reset leaves in the rows of the envs it names)
        self.o.done[named] = 0
        self.running_return[named] = 0.0
        self.running_length[named] = 0
        return self.o.obs

    def plain_step(self, actions):
        """pgv_step: not counted."""
        return self.o.step(actions)

    def step(self, actions):
        prev_done = self.o.done.copy()
        obs, reward, done = self.o.step(actions)
        counted = prev_done == 0
        ret = np.where(counted, (self.running_return + reward).astype(np.float32), self.running_return).astype(np.float32)
        length = self.running_length + counted.astype(np.int32)
        self.reward = reward.copy()
        self.terminated = (done != 0).astype(np.uint8)
        self.truncated = (counted & (done == 0) & (self.T > 0) & (length >= self.T)).astype(np.uint8)
        self.ended = self.terminated | self.truncated
        self.ended_env = np.nonzero(self.ended)[0].astype(np.int32)
        self.counts = np.array([self.ended_env.size, min(self.ended_env.size, self.capacity)], np.int32)
        self.ended_return = ret[self.ended_env]
        self.ended_length = length[self.ended_env]
        self.ended_level = np.zeros(self.ended_env.size, np.uint32)
        self.ended_level_known = np.zeros(self.ended_env.size, np.uint8)
        self.final_obs = obs[self.ended_env[:self.counts[1]]].copy()
        if self.ended_env.size:
            self.longest = max(self.longest, int(self.ended_length.max()))
        ended = self.ended != 0
        self.running_return = np.where(ended, np.float32(0), ret).astype(np.float32)
        self.running_length = np.where(ended, 0, length).astype(np.int32)
        if self.mode == SAME_STEP and ended.any():
            self.o.reset(mask=self.ended)
            self.o.reward[ended] = 0.0
            self.o.done[ended] = 0
        return self.o.obs

    def close(self):
        self.o.close()


class OracleEpisodeEngine:
    """The adapter's engine contract with step_episodes, on the CPU: what ProcgenVecEnv(autoreset_mode=...) offers, made of
    the model (numpy arrays where the real one has device tensors)."""

    class _Outputs:
        pass

    def __init__(self, game, n, autoreset_mode, max_episode_steps=0, final_obs_capacity=0, seed_base=1):
        self.m = EpisodeModel(game, n, autoreset_mode, max_episode_steps, final_obs_capacity, seed_base)
        self.game, self.num_envs, self.autoreset_mode = game, n, autoreset_mode
        self.episode = self._Outputs()
        self.calls = []
        self.fresh = True

    def reset(self, mask=None, seeds=None):
        assert seeds is None
        self.calls.append("reset")
        first, self.fresh = self.fresh and mask is None, False
        return (self.m.first_reset() if first else self.m.reset(mask)).reshape(self.num_envs, 64, 64, 3)

    def step(self, actions):
        self.calls.append("step")
        obs, reward, done = self.m.plain_step(np.asarray(actions))
        return obs.reshape(self.num_envs, 64, 64, 3), reward, done

    def step_episodes(self, actions):
        self.calls.append("step_episodes")
        m, ep, n = self.m, self.episode, self.num_envs
        obs = m.step(np.asarray(actions)).reshape(n, 64, 64, 3)
        ep.reward, ep.terminated, ep.truncated, ep.ended, ep.counts = m.reward, m.terminated, m.truncated, m.ended, m.counts

        def padded(x, rows, fill):  # the engine's lists have N rows (the ring: capacity); what lies past the counts is anything
            out = np.full((rows,) + x.shape[1:], fill, x.dtype)
            out[:x.shape[0]] = x
            return out
        ep.ended_env = padded(m.ended_env, n, -7)
        ep.ended_return = padded(m.ended_return, n, np.float32(-7))
        ep.ended_length = padded(m.ended_length, n, -7)
        ep.ended_level = padded(m.ended_level, n, 7)
        ep.ended_level_known = padded(m.ended_level_known, n, 7)
        ep.final_obs = padded(m.final_obs.reshape(-1, 64, 64, 3), m.capacity, 7)
        return obs, ep

    def close(self):
        self.m.close()
