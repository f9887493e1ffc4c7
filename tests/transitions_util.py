"""The model of the engine's transitions (include/procgen2_vec.h pgv_transitions_enable) in numpy, on top of the frame
history's model (tests/history_util.py): the [T, N] record ring filled from the oracle's rewards and dones and EpisodeModel's
terminated / truncated, the n-step walk and the GAE recurrence, each following the header's points literally in np.float32 —
every product and every sum its own rounding.  The GPU tests trust this model, not the engine; tests/test_transitions.py
holds the header's host half to a deque per env and a straight loop (tests/cpp/test_transitions.cpp) and counts what the
GPU runs reach on the oracle.
"""
import numpy as np

from episodes_util import SAME_STEP, synthetic_actions
from history_util import CALLS, N, RUN_SEED, T, HistoryEpisodes, HistorySequence, HistoryVec

RECORDED, TERMINATED, TRUNCATED, VOID, CUT = 1, 2, 4, 8, 16
VALID = 1

# The GPU tests' runs (game, autoreset mode, step limit); tests/test_transitions.py counts what they reach on the oracle.
RUNS = [("maze", SAME_STEP, 7), ("bossfight", "next_step", 0), ("chaser", SAME_STEP, 7)]
# The GAE engine: a ring of 17 slots holds a stretch of 16 rows.
GAE_T, GAE_L = 17, 16
GAE_PARAMS = [(0.99, 0.95), (1.0, 1.0)]
GATHER_PARAMS = [(n, gamma) for n in (1, 3, 6) for gamma in (0.99, 1.0)]

f32 = np.float32


class TransitionModel:
    """The record ring beside a HistoryRing `h` (its head, its began bytes).  record() and unrecorded() are called BEHIND the
    push of the same call, so the row they write is head - 2: the call that made push head - 1."""

    def __init__(self, h):
        self.h = h
        self.action = np.zeros((h.T, h.n), np.int32)
        self.reward = np.zeros((h.T, h.n), np.float32)
        self.flags = np.zeros((h.T, h.n), np.uint8)

    def record(self, action, reward, terminated, truncated, void):
        q = self.h.head - 2
        if q < 0:
            return
        s = q % self.h.T
        self.action[s] = action
        self.reward[s] = reward
        self.flags[s] = (RECORDED | np.where(np.asarray(terminated) != 0, TERMINATED, 0) | np.where(np.asarray(truncated) != 0, TRUNCATED, 0)
                         | np.where(np.asarray(void) != 0, VOID, 0)).astype(np.uint8)

    def unrecorded(self):
        q = self.h.head - 2
        if q < 0:
            return
        s = q % self.h.T
        self.action[s], self.reward[s], self.flags[s] = 0, 0.0, 0

    # -- the derived terms, over arrays of rows q and envs i (i inside the batch) ---------------------
    def held(self, q):
        h = self.h
        return (q >= 0) & (q >= h.head - h.T) & (q + 1 < h.head)

    def rows(self, q, i):
        """(complete, flags, reward, ends) of rows (q[b], i[b]); ends = TERMINATED | TRUNCATED | CUT bits; zeros where not held."""
        h = self.h
        held = self.held(q)
        s, s1 = np.where(held, q % h.T, 0), np.where(held, (q + 1) % h.T, 0)
        flags = np.where(held, self.flags[s, i], 0).astype(np.uint8)
        reward = np.where(held, self.reward[s, i], f32(0)).astype(np.float32)
        began = np.where(held, h.began[s1, i], 0)
        complete = held & ((flags & RECORDED) != 0)
        own = flags & (TERMINATED | TRUNCATED)
        cut = complete & (own == 0) & ((flags & VOID) == 0) & (began != 0)
        ends = np.where(complete, np.where(cut, CUT, own), 0).astype(np.uint8)
        return complete, flags, reward, ends

    def walk(self, pushes, envs, n, gamma):
        """Point 4, over all entries at once and row by row: dict of action, nstep_return, discount, steps, status."""
        h = self.h
        p, i = np.asarray(pushes, np.int64), np.asarray(envs, np.int64)
        inside = (i >= 0) & (i < h.n) & (p >= 0) & (p < h.head)
        p0, i0 = np.where(inside, p, 0), np.where(inside, i, 0)
        B = p.size
        m = np.zeros(B, np.int32)
        ret, disc = np.zeros(B, np.float32), np.ones(B, np.float32)
        last = np.zeros(B, np.uint8)
        going = inside.copy()
        g = f32(gamma)
        for k in range(n):
            complete, flags, reward, ends = self.rows(p0 + k, i0)
            going = going & complete & ((flags & VOID) == 0)
            t = (disc * reward).astype(np.float32)
            ret = np.where(going, (ret + t).astype(np.float32), ret).astype(np.float32)
            disc = np.where(going, (disc * g).astype(np.float32), disc).astype(np.float32)
            m = m + going.astype(np.int32)
            last = np.where(going, ends, last).astype(np.uint8)
            going = going & (ends == 0)
        valid = m > 0
        action = np.where(valid, self.action[np.where(valid, p0 % h.T, 0), i0], 0).astype(np.int32)
        discount = np.where(valid, np.where((last & TERMINATED) != 0, f32(0), disc), f32(0)).astype(np.float32)
        return dict(action=action, nstep_return=np.where(valid, ret, f32(0)).astype(np.float32), discount=discount, steps=m,
                    status=np.where(valid, VALID | last, 0).astype(np.uint8))

    def walk_one(self, p, i, n, gamma):
        """The same walk for one entry in plain Python scalars: what the vectorised form is held to (tests/test_transitions.py)."""
        h = self.h
        zero = dict(action=0, nstep_return=f32(0), discount=f32(0), steps=0, status=0)
        if not (0 <= i < h.n):
            return zero
        m, ret, disc, last = 0, f32(0), f32(1), 0
        for k in range(n):
            q = p + k
            if not (q >= 0 and h.head - h.T <= q and q + 1 < h.head):
                break
            fl = int(self.flags[q % h.T][i])
            if not fl & RECORDED or fl & VOID:
                break
            t = f32(disc * self.reward[q % h.T][i])
            ret = f32(ret + t)
            disc = f32(disc * f32(gamma))
            m += 1
            last = fl & (TERMINATED | TRUNCATED)
            if not last and h.began[(q + 1) % h.T][i]:
                last = CUT
            if last:
                break
        if m == 0:
            return zero
        return dict(action=int(self.action[p % h.T][i]), nstep_return=ret, discount=f32(0) if last & TERMINATED else disc, steps=m,
                    status=VALID | last)

    def gather(self, pushes, envs, n, gamma, K=None, dtype=None):
        """walk() plus, with K and dtype, obs = HistoryRing.gather(p) and next_obs = HistoryRing.gather(p + steps), zero rows
        for an invalid entry."""
        out = self.walk(pushes, envs, n, gamma)
        if K is not None:
            valid = out["steps"] > 0
            p = np.asarray(pushes, np.int64)
            i = np.where(valid, np.asarray(envs, np.int64), -1)
            out["obs"] = self.h.gather(np.where(valid, p, 0), i, K, dtype)
            out["next_obs"] = self.h.gather(np.where(valid, p, 0) + out["steps"], i, K, dtype)
        return out

    def gae(self, first, L, values, gamma, lam, trunc_values=None):
        """Point 5: (advantages, returns) float32 [L, N]."""
        h = self.h
        assert first >= 0 and first >= h.head - h.T and first + L - 1 + 1 < h.head
        V = np.asarray(values, np.float32)
        g, c = f32(gamma), f32(f32(gamma) * f32(lam))
        adv, ret = np.zeros((L, h.n), np.float32), np.zeros((L, h.n), np.float32)
        carry = np.zeros(h.n, np.float32)
        envs = np.arange(h.n)
        for t in range(L - 1, -1, -1):
            complete, flags, reward, ends = self.rows(np.full(h.n, first + t, np.int64), envs)
            off = ~complete | ((flags & VOID) != 0)
            tv = np.zeros(h.n, np.float32) if trunc_values is None else np.asarray(trunc_values[t], np.float32)
            nv = np.where(ends == 0, V[t + 1], np.where(ends == TRUNCATED, tv, f32(0))).astype(np.float32)
            a = (g * nv).astype(np.float32)
            b = (reward + a).astype(np.float32)
            delta = (b - V[t]).astype(np.float32)
            d = (c * carry).astype(np.float32)
            row = np.where(ends == 0, (delta + d).astype(np.float32), delta).astype(np.float32)
            row = np.where(off, f32(0), row).astype(np.float32)
            adv[t] = row
            ret[t] = np.where(off, V[t], (row + V[t]).astype(np.float32))
            carry = row
        return adv, ret


def gae_loop(model, first, L, values, gamma, lam, trunc_values, i):
    """Point 5 for env i in plain Python scalars."""
    h = model.h
    c = f32(f32(gamma) * f32(lam))
    carry, adv, ret = f32(0), [None] * L, [None] * L
    for t in range(L - 1, -1, -1):
        q = first + t
        fl, r, v = int(model.flags[q % h.T][i]), model.reward[q % h.T][i], f32(values[t][i])
        if not fl & RECORDED or fl & VOID:
            adv[t], ret[t], carry = f32(0), v, f32(0)
            continue
        ends = fl & (TERMINATED | TRUNCATED)
        if not ends and h.began[(q + 1) % h.T][i]:
            ends = CUT
        nv = f32(values[t + 1][i]) if not ends else (f32(0) if trunc_values is None else f32(trunc_values[t][i])) if ends == TRUNCATED else f32(0)
        a = f32(f32(gamma) * nv)
        b = f32(r + a)
        delta = f32(b - v)
        adv[t] = f32(delta + f32(c * carry)) if not ends else delta
        carry = adv[t]
        ret[t] = f32(adv[t] + v)
    return np.array(adv, np.float32), np.array(ret, np.float32)


# -- drivers: the frame history's, with the record ring filled by the same calls ------------------------

class TransitionsVec(HistoryVec):
    """pgv_reset and pgv_step."""

    def __init__(self, game, n, T, gray_rule, **more):
        super().__init__(game, n, T, gray_rule, **more)
        self.tr = TransitionModel(self.ring)

    def step(self, actions):
        void = self.o.done.copy()  # the done row as the step finds it
        res = super().step(actions)
        self.tr.record(actions, self.o.reward, self.o.done, 0, void)
        return res

    def push(self):
        """pgv_history_push by hand."""
        self.f.push(self.o.obs)
        self.tr.unrecorded()


class TransitionsEpisodes(HistoryEpisodes):
    """pgv_step_episodes: reward, terminated and truncated from the episode outputs."""

    def __init__(self, game, n, mode, T, gray_rule, max_episode_steps=0):
        super().__init__(game, n, mode, T, gray_rule, max_episode_steps=max_episode_steps)
        self.tr = TransitionModel(self.ring)

    def step(self, actions):
        void = self.m.engine_done.copy()
        super().step(actions)
        self.tr.record(actions, self.m.reward, self.m.terminated, self.m.truncated, void)


class TransitionsSequence(HistorySequence):
    """pgv_step_sequence: a drawn sequence opens a slot whose row is not recorded."""

    def __init__(self, game, n, T, gray_rule):
        super().__init__(game, n, T, gray_rule)
        self.tr = TransitionModel(self.ring)

    def sequence(self, actions, frames_last=True, draw=None):
        super().sequence(actions, frames_last, draw)
        if frames_last:
            self.tr.unrecorded()

    def step(self, actions):
        """pgv_step between the sequences."""
        void = self.m.o.done.copy()
        self.f.flag(self.m.o.done)
        self.m.plain_step(actions)
        self.f.push(self.m.obs)
        self.tr.record(actions, self.m.o.reward, self.m.o.done, 0, void)

    def push(self):
        super().push()
        self.tr.unrecorded()


def entries(head, T, n):
    """Every held push plus head - T - 1, head - 1 (held, no successor), head and -1, times every env plus -1 and n."""
    pushes = sorted(set(range(max(0, head - T), head)) | {head - T - 1, head - 1, head, -1})
    envs = list(range(n)) + [-1, n]
    return np.repeat(np.array(pushes, np.int64), len(envs)), np.tile(np.array(envs, np.int32), len(pushes))


def run_counts(game, mode, limit, n=N, T=T, calls=CALLS):
    """What a run reaches on the oracle alone: rows by flag, reward values seen, gathered entries by status."""
    m = TransitionsEpisodes(game, n, mode, T, False, max_episode_steps=limit)
    m.first_reset()
    c = dict(terminated=0, truncated=0, void=0, rewards={}, cut_short=0, rounded=0)
    for t in range(calls):
        m.step(synthetic_actions(RUN_SEED, t, n))
        fl = m.tr.flags[(m.ring.head - 2) % T]
        c["terminated"] += int(((fl & TERMINATED) != 0).sum())
        c["truncated"] += int(((fl & TRUNCATED) != 0).sum())
        c["void"] += int(((fl & VOID) != 0).sum())
        for r in m.tr.reward[(m.ring.head - 2) % T]:
            c["rewards"][float(r)] = c["rewards"].get(float(r), 0) + 1
        p, i = entries(m.ring.head, T, n)
        w = m.tr.walk(p, i, 3, 0.99)
        c["cut_short"] += int(((w["steps"] > 0) & (w["steps"] < 3)).sum())
        exact = m.tr.walk(p, i, 3, 1.0)
        c["rounded"] += int((w["nstep_return"].astype(np.float64) != exact["nstep_return"].astype(np.float64)).sum())
    m.close()
    return c
