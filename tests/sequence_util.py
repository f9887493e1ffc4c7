"""The model of pgv_step_sequence (include/procgen2_vec.h): an OracleVec stepped T times, drawing switched off
(OracleVec.set_render(False): logic is unaffected) on the sub-steps that draw nothing, plus the summary folded in numpy.
The GPU tests trust this model, not the engine; tests/test_sequence.py holds the model itself to T drawn oracle steps.

The protocol every GPU test runs: PROTOCOL_N envs, seed_base 1, one full reset, pgo_synthetic_action with run seed
PROTOCOL_SEED as explicit actions, PROTOCOL_STEPS steps cut into sequences of PROTOCOL_LENGTHS.
"""
import numpy as np

from episodes_util import synthetic_actions
from oracle_util import OracleVec

GAMES = ("coinrun", "maze", "bossfight", "climber", "caveflyer", "chaser", "jumper")
PROTOCOL_N, PROTOCOL_SEED = 300, 7
PROTOCOL_LENGTHS = (1, 2, 3, 5, 8, 13) * 5
PROTOCOL_STEPS = sum(PROTOCOL_LENGTHS)  # 160


def fold(rewards, dones):
    """(seq_return, seq_length, seq_done) of rows [T, N]: the sub-steps up to and including the env's first done — all T
    without one — and the float32 sum of their rewards in step order from 0.0f, one rounding a step."""
    T, n = dones.shape
    ret, length, done = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for t in range(T):
        live = done == 0
        ret = np.where(live, (ret + rewards[t]).astype(np.float32), ret).astype(np.float32)
        length = length + live.astype(np.int32)
        done = np.where(live, (dones[t] != 0).astype(np.uint8), done).astype(np.uint8)
    return ret, length, done


def protocol_calls(n=PROTOCOL_N, lengths=PROTOCOL_LENGTHS, run_seed=PROTOCOL_SEED, first_step=0):
    """The protocol's calls in order: (index of the call's first step, actions int32 [T, n])."""
    t = first_step
    for T in lengths:
        yield t, np.stack([synthetic_actions(run_seed, t + k, n) for k in range(T)])
        t += T


def count_protocol(game, mode=0):
    """The ground the protocol covers in one (game, mode), counted on the oracle without drawing: dones inside a sequence, and
    chaser's late-pass rows — envs reset in a call's last sub-step (test_sequence_gpu.run_frames_none) — summed over every
    third call and over every call."""
    m = SequenceModel(game, PROTOCOL_N, render=False, mode=mode)
    m.reset()
    inside = third = every = 0
    due = np.zeros(PROTOCOL_N, bool)
    for k, (_, actions) in enumerate(protocol_calls()):
        _, dones = m.sequence(actions)
        inside += int((dones[:-1] != 0).sum())
        reset_last = dones[-2] != 0 if len(actions) >= 2 else due
        due = dones[-1] != 0
        every += int(reset_last.sum())
        third += int(reset_last.sum()) if k % 3 == 2 else 0
    m.close()
    return inside, third, every


# chaser's late-pass rows per distribution mode (0: the default, easy), on the oracle: (in every third call, in every call);
# tests/test_variant_paths.py holds the table to count_protocol
CHASER_LATE_ROWS = {0: (8, 27), 2: (17, 33), 4: (15, 35)}


def chaser_late_rows(mode):
    """(rows the GPU test will see, whether it looks at every call, its floor).  Every third call where that gives six
    rows or more, else every call; the floor is half the oracle's count (the default mode keeps the 5 of 8 it always had)."""
    third, every = CHASER_LATE_ROWS[mode]
    every_call = third < 6
    count = every if every_call else third
    return count, every_call, 5 if mode == 0 else (count + 1) // 2


class SequenceModel:
    def __init__(self, game, n, seed_base=1, render=True, mode=0, env_offset=0, threads=1):
        """env_offset=a: the model of rows [a, a + n) of a larger engine; threads: OracleVec's."""
        self.o = OracleVec(game, n, seed_base=seed_base, render=render, mode=mode, env_offset=env_offset, threads=threads)
        self.env_offset = env_offset
        self.n, self.can_draw = n, render

    obs = property(lambda self: self.o.obs)
    engine_reward = property(lambda self: self.o.reward)
    engine_done = property(lambda self: self.o.done)

    def first_reset(self):
        """The engine's first pgv_reset after make: an OracleVec had it when it was made."""
        return self.o.reset_obs()

    def reset(self):
        """pgv_reset(NULL, NULL) — the protocol's one full reset: what it leaves in the engine's rows included."""
        self.o.reset()
        self.o.reward[:] = 0.0
        self.o.done[:] = 0
        return self.o.obs

    def sequence(self, actions, draw_last=True):
        """T sub-steps, actions [T, N]; only the last is drawn, and that one only if draw_last.  With draw_last, `obs` is then
        what PGV_FRAMES_LAST leaves — and what pgv_render_obs(NULL) leaves after PGV_FRAMES_NONE."""
        actions = np.asarray(actions, np.int32)
        T = actions.shape[0]
        self.rewards, self.dones = np.zeros((T, self.n), np.float32), np.zeros((T, self.n), np.uint8)
        for t in range(T):
            if self.can_draw:
                self.o.set_render(draw_last and t == T - 1)
            _, self.rewards[t], self.dones[t] = self.o.step(actions[t])
        if self.can_draw:
            self.o.set_render(True)
        self.seq_return, self.seq_length, self.seq_done = fold(self.rewards, self.dones)
        return self.rewards, self.dones

    def plain_step(self, actions):
        return self.o.step(actions)

    def close(self):
        self.o.close()
