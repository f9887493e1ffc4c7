"""Shared by test_feature_scale.py (CPU) and test_feature_scale_gpu.py: the plans of the full-batch tests of the feature
layers — sizes, seeds, slices, index lists — and the whole-batch models that run without drawing, with the conditions that
keep the GPU tests from passing vacuously.  The CPU file establishes the conditions on the oracle alone; the GPU file asserts
them again on its own model run.

How a reference is had at these sizes: rewards, dones and everything folded from them come from an OracleVec(render=False) of
the whole n, stepped by several threads; pixels come from drawn slices of 64 envs, OracleVec(env_offset=a) being the model of
rows [a, a + 64) of a larger engine (an env's stream and synthetic action are functions of its global index).
"""
import numpy as np

from episodes_util import NEXT_STEP, SAME_STEP, EpisodeModel
from history_aug_util import M, mix32
from oracle_util import OracleVec
from sequence_util import SequenceModel

SEED_BASE, RUN_SEED, SLICE = 1, 7, 64
ENV_BYTES = 64 * 64 * 3


def host_threads():
    from test_snapshot import _host_threads
    return _host_threads()


def actions_of(run_seed, step, n, env_offset=0):
    """pgo_synthetic_action(run_seed, step, env_offset + i) for i < n, in numpy (test_feature_scale.py holds it to the C one)."""
    env = np.arange(env_offset, env_offset + n, dtype=np.uint64)
    outer = mix32((step * 0x9E3779B9 + run_seed) & 0xFFFFFFFF)
    h = mix32(outer ^ ((env * np.uint64(0x85EBCA6B) + np.uint64(0xC2B2AE35)) & M))
    return ((h * np.uint64(15)) >> np.uint64(32)).astype(np.int32)


def slices_of(n, around=(), given=()):
    """The drawn slices as (first row, rows): [0, 64), the ragged end [n - 65, n), 64 rows around every env of `around` (32 to
    each side of it) and the `given` ranges of 64."""
    out = [(0, SLICE), (n - SLICE - 1, SLICE + 1)] + [(b - SLICE // 2, SLICE) for b in around] + [(a, SLICE) for a in given]
    assert all(0 <= a and a + k <= n for a, k in out)
    return out


def slice_of(slices, env):
    """(index of the slice that holds the env, its row there), or None."""
    for s, (a, k) in enumerate(slices):
        if a <= env < a + k:
            return s, env - a
    return None


# ---- 1. episodes across many workgroups ---------------------------------------------------------------------------------
EP_N, EP_CALLS, EP_BLOCK = 70001, 27, 256
EP_BLOCKS = (EP_N + EP_BLOCK - 1) // EP_BLOCK  # 274
# (game, autoreset mode, max_episode_steps, final_obs_capacity).  Two settings are not the ones first wished for, because the
# conditions below come first:
#   * the engine refuses a step limit in next_step mode (pgv_episodes_enable), so that case has none — and then nothing can
#     end more than half of maze's envs in one call before the game's own 500-step cap;
#   * bossfight ends 585 envs at most in a call before the limit ends 68 176 at once, whose 1 000th lies in workgroup 3: with
#     a ring of 496 rows the cut of call 22 (585 ends) falls inside workgroup 230, four of whose six ended envs get a row.
EP_CASES = [("maze", NEXT_STEP, 0, 1000), ("maze", SAME_STEP, 24, 1000), ("bossfight", SAME_STEP, 24, 496)]
EP_SLICES = slices_of(EP_N, around=(16384, 65536))  # (workgroups 64 | 65: waves 0 | 1 of the base loop; 256 | 257: its second trip)
# The conditions a case meets (EpisodeGround.met).  `few` (a call that ends fewer than 64 envs) is beyond maze at this n,
# whatever the seed and however many calls: about 2.6 % of fresh mazes end at once and never fewer than 150 envs a call; what
# `few` is wanted for — workgroups without an ended env, in numbers — maze does reach, and every case is held to that (`empty`).
EP_MEETS = {("maze", NEXT_STEP): {"many", "cut", "empty"},
            ("maze", SAME_STEP): {"many", "cut", "half", "empty"},
            ("bossfight", SAME_STEP): {"many", "cut", "half", "few", "empty"}}


class EpisodeGround:
    """What the calls of an episode case reach, from the whole-batch model's ended lists:
    many:  a call ends envs in more than 256 workgroups (the base loop's second trip adds a non-zero count);
    cut:   a call has at least `capacity` ends, the ring's last row belongs to a workgroup numbered >= 64 (a base that waves
           1 .. 3 contribute to) which also has an ended env left out, and the row's env is not the workgroup's lane 0;
    half:  a call ends more than n / 2 envs;
    few:   a call ends fewer than 64 envs;
    empty: a call leaves at least 64 workgroups without an ended env."""

    def __init__(self, n, capacity):
        self.n, self.capacity, self.met = n, capacity, set()

    def add(self, ended_env):
        e = np.asarray(ended_env, np.int64)
        blocks = np.unique(e // EP_BLOCK)
        if blocks.size > 256:
            self.met.add("many")
        if e.size > self.n / 2:
            self.met.add("half")
        if e.size < 64:
            self.met.add("few")
        if EP_BLOCKS - blocks.size >= 64:
            self.met.add("empty")
        if e.size > self.capacity:
            last, left_out = e[self.capacity - 1], e[self.capacity]
            if last // EP_BLOCK >= 64 and last % EP_BLOCK != 0 and left_out // EP_BLOCK == last // EP_BLOCK:
                self.met.add("cut")


def episode_model(game, mode, limit, capacity, n=EP_N, env_offset=0, render=False, threads=None):
    """The case's EpisodeModel: the whole batch without drawing, or a drawn slice of it."""
    return EpisodeModel(game, n, mode, limit, capacity, seed_base=SEED_BASE, render=render, env_offset=env_offset,
                        threads=host_threads() if threads is None else threads)


def ring_spots(ended_env, kept):
    """Up to 8 rows of the terminal-frame ring to hold to a drawn replay of their env: the last row written and its
    neighbour, and the rows on either side of the first, the middle and the last workgroup boundary inside the ring."""
    e = np.asarray(ended_env[:kept], np.int64)
    if not kept:
        return []
    rows = {kept - 1, max(0, kept - 2)}
    edges = np.nonzero(e[1:] // EP_BLOCK != e[:-1] // EP_BLOCK)[0]  # rows r with row r + 1 in another workgroup
    for r in (edges[[0, edges.size // 2, -1]] if edges.size else ()):
        rows |= {int(r), int(r) + 1}
    return sorted(rows)[:8]


# ---- 3. policy observations beyond 2^32 bytes ---------------------------------------------------------------------------
STRIDED = 1 << 26  # pgv_set_debug: the strided store form
PO_STEPS_A, PO_STEPS_B = 9, 2  # reset, 9 steps, a masked reset of every third env, 2 more steps
# (game, dtype, K, n, debug): RGB, 196 608 B (f32, K = 4) or 98 304 B (u8, K = 8) per env, 4.33 GB either way
PO_CASES = [("maze", "float32", 4, 22000, 0), ("maze", "float32", 4, 22000, STRIDED), ("coinrun", "float32", 4, 22000, 0),
            ("maze", "uint8", 8, 44000, 0)]


def straddlers(row_bytes, total_rows):
    """The rows of a tensor of `row_bytes` a row that hold byte 2^31 and byte 2^32 without beginning there."""
    out = [b // row_bytes for b in (1 << 31, 1 << 32) if b % row_bytes and b // row_bytes < total_rows]
    return out


def policy_slices(dtype, K, n):
    es = {"uint8": 1, "float32": 4}[dtype]
    rows = straddlers(K * 3 * 4096 * es, n)
    assert len(rows) == 2
    return slices_of(n, around=rows)


class Flags:
    """The restart flags of the policy observations / the pending flags of the history for a whole batch (PolicyStack's and
    HistoryRing's rule without the frames): flag() sets, a push returns who was flagged among the envs it touches and clears them."""

    def __init__(self, n):
        self.flags = np.ones(n, np.uint8)  # (enable sets every flag)

    def flag(self, where):
        self.flags[:] = 1 if where is None else self.flags | (np.asarray(where) != 0)

    def push(self, mask=None):
        touched = np.ones(self.flags.size, bool) if mask is None else np.asarray(mask) != 0
        fresh = touched & (self.flags != 0)
        self.flags[touched] = 0
        return fresh, touched


class LogicVec:
    """The whole batch without drawing under pgv_reset / pgv_step, with the rows pgv_reset leaves (PolicyVec's and
    HistoryVec's driver without the frames) and the flags."""

    def __init__(self, game, n, threads=None):
        self.o = OracleVec(game, n, seed_base=SEED_BASE, render=False, threads=host_threads() if threads is None else threads)
        self.n, self.f = n, Flags(n)
        self.restarted = np.zeros(n, bool)  # envs a step found done (their episode began anew inside the run)

    done = property(lambda self: self.o.done)
    reward = property(lambda self: self.o.reward)

    def first_reset(self):
        """→ (fresh, touched) of the push the reset makes."""
        return self._reset_done(None)

    def reset(self, mask):
        self.o.reset(mask=mask)
        return self._reset_done(mask)

    def _reset_done(self, mask):
        named = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.o.reward[named] = 0.0
        self.o.done[named] = 0
        self.f.flag(mask)
        return self.f.push(mask)

    def step(self, actions):
        self.restarted |= self.o.done != 0
        self.f.flag(self.o.done)  # the done row as the step finds it
        self.o.step(actions)
        return self.f.push()

    def close(self):
        self.o.close()


def third_mask(n):
    return (np.arange(n) % 3 == 0).astype(np.uint8)


def policy_calls(n):
    """The run's calls in order: ("reset", None) first, ("step", t), ("reset", mask)."""
    calls = [("reset", None)] + [("step", t) for t in range(PO_STEPS_A)] + [("reset", third_mask(n))]
    return calls + [("step", t) for t in range(PO_STEPS_A, PO_STEPS_A + PO_STEPS_B)]


def run_logic(game, n, calls, threads=None):
    """The whole-batch model through `calls`: yields (call, LogicVec, fresh, touched) after each."""
    m = LogicVec(game, n, threads)
    try:
        for kind, arg in calls:
            if kind == "reset":
                fresh, touched = m.first_reset() if arg is None else m.reset(arg)
            else:
                fresh, touched = m.step(actions_of(RUN_SEED, arg, n))
            yield (kind, arg), m, fresh, touched
    finally:
        m.close()


def slices_restart_and_not(restarted, slices):
    """Inside every slice at least one env's episode ended and began anew during the run, and at least one's did not."""
    return all(restarted[a:a + k].any() and not restarted[a:a + k].all() for a, k in slices)


# ---- 4. frame history and gathers beyond 2^32 bytes ---------------------------------------------------------------------
HI_STEPS = 19  # reset + 19 steps: 20 pushes; a ring of 16 or 17 slots wraps and slots 0 .. 2 (or 3) are written again
# (gray, n, T, slices): RGB 22 000 × 16 is 4.33 GB, frame (slot 7, env 20 762) holds byte 2^31 and (slot 15, env 19 525) byte
# 2^32; gray 65 536 × 17 is 4.56 GB, slot 8 begins at byte 2^31 and slot 16 at 2^32 — the end slices lie on both sides.
HI_RGB = (False, 22000, 16, slices_of(22000, given=(19500, 20740)))
HI_GRAY = (True, 65536, 17, slices_of(65536))
HI_CASES = [HI_RGB, HI_GRAY]
GATHER_K, GATHER_DTYPE = 4, "float32"
GATHER_NAMED = (0, 10900, 21820, 22000 - 64)  # the first entries of the four runs of 64 that name envs of drawn slices
GATHER_OUTSIDE = ((100, -1), (15000, 22000))  # (entry, env): outside the batch
AUGMENT = dict(size=64, pad=4, edge="replicate", cutout=(8, 24), cutout_color="random", seed=11)


def history_calls():
    return [("reset", None)] + [("step", t) for t in range(HI_STEPS)]


class BeganRows:
    """The ring's began bytes [T, n] and head for a whole batch, fed with what run_logic yields (HistoryRing's push and reset
    without the frames: a step opens a slot and files who was pending; a reset marks the envs it names in the newest slot)."""

    def __init__(self, n, T):
        self.T, self.head, self.began = T, 0, np.zeros((T, n), np.uint8)

    def add(self, kind, fresh, touched):
        if kind == "step" or self.head == 0:
            self.head += 1
        self.began[(self.head - 1) % self.T][touched] = fresh[touched]


def frame_straddlers(gray, n, T):
    """(slot, env) of the frames that hold byte 2^31 and byte 2^32 of the ring without beginning there."""
    return [(r // n, r % n) for r in straddlers((1 if gray else 3) * 4096, n * T)]


def gather_entries(n, T, head, slices):
    """(pushes int64 [B], envs int32 [B], named [256]) of the gather, B = n: pushes drawn from [head - T - 2, head + 1) — some
    not held —, envs a permutation of the batch with the four named runs of 64 entries rewritten to envs of the drawn slices,
    and one env on either side of the batch."""
    rng = np.random.default_rng(20241)
    pushes = rng.integers(head - T - 2, head + 1, n).astype(np.int64)
    envs = rng.permutation(n).astype(np.int32)
    drawn = np.concatenate([np.arange(a, a + k) for a, k in slices])
    named = np.concatenate([np.arange(b, b + SLICE) for b in GATHER_NAMED])
    envs[named] = rng.choice(drawn, named.size)
    for b, env in GATHER_OUTSIDE:
        envs[b] = env
    return pushes, envs, named


def held(pushes, envs, n, T, head):
    p, i = np.asarray(pushes), np.asarray(envs)
    return (p >= 0) & (p >= head - T) & (p < head) & (i >= 0) & (i < n)


def augment_config(size):
    """history_aug_util's config of AUGMENT at an output size."""
    return dict(H=size, W=size, pad=AUGMENT["pad"], lo=AUGMENT["cutout"][0], hi=AUGMENT["cutout"][1], edge=AUGMENT["edge"],
                color=AUGMENT["cutout_color"], seed=AUGMENT["seed"])


# ---- 2. frameless sequences at batch size -------------------------------------------------------------------------------
SEQ_N = 65536
# game → T.  coinrun (resolve kernel, generator on the side stream) and maze at 24; chaser (level kernel on its own stream,
# late pass) at 40: the oracle's chaser ends no episode before step 42 under these actions, so at T = 24 neither of the two
# calls would hold a done at all.  At 40 the second call has 5 867 first dones in its first third and 5 634 in its last.
SEQ_GAMES = {"coinrun": 24, "chaser": 40, "maze": 24}
SEQ_INSIDE = {"coinrun": 100, "chaser": 256, "maze": 256}  # envs done inside a call (before its last sub-step), at least
SEQ_SLICES = slices_of(SEQ_N, around=(16384,))
SEQ_STRIDE = 4099  # the envs whose state and tile dumps are compared


def sequence_actions(call, T, n, env_offset=0):
    """int32 [T, n]: the actions of the call's sub-steps."""
    return np.stack([actions_of(RUN_SEED, call * T + t, n, env_offset) for t in range(T)])


class SequenceGround:
    """What the two calls reach, from the whole-batch model's rows: envs whose first done lies in the first third of a call,
    in its last third, and dones inside a call (before its last sub-step)."""

    def __init__(self):
        self.early = self.late = self.inside = 0

    def add(self, model, T):
        first = model.seq_done != 0
        self.early += int((first & (model.seq_length <= T // 3)).sum())
        self.late += int((first & (model.seq_length > T - T // 3)).sum())
        self.inside = max(self.inside, int((model.dones[:-1] != 0).sum()))  # (in one call)

    def holds(self, game):
        return self.early >= 1 and self.late >= 1 and self.inside >= SEQ_INSIDE[game]


def sequence_model(game, n=SEQ_N, env_offset=0, render=False, threads=None):
    return SequenceModel(game, n, seed_base=SEED_BASE, render=render, env_offset=env_offset,
                         threads=host_threads() if threads is None else threads)


# ---- 5. the symbolic layer and caller-made levels at batch size ---------------------------------------------------------
SY_N, SY_STEPS, SY_B, SY_SAMPLE = 65536, 12, 100003, 512
SY_GAMES = {"coinrun": ("state",), "chaser": ("state",), "maze": ("paths", "levels"), "caveflyer": ("paths",)}  # state: state_obs and tile_obs
SY_EDGES = (0, 255, 256, 16383, 16384, 65535)  # the ends of a workgroup of 256, of 64 of them, of the batch
SY_OUTSIDE = ((7, -1), (50001, SY_N), (99999, 2 ** 31 - 1), (SY_B - 1, -2 ** 31))  # (place in the index list, index)


def symbolic_indices(n=SY_N, count=SY_B):
    """int32 [count]: draws from the batch with repeats, every edge env at a fixed place, and the four indices outside it."""
    rng = np.random.default_rng(5)
    idx = rng.integers(0, n, count).astype(np.int32)
    idx[1000:1000 + len(SY_EDGES)] = SY_EDGES
    for place, index in SY_OUTSIDE:
        idx[place] = index
    return idx


def symbolic_sample(n=SY_N, count=SY_SAMPLE):
    """The envs whose rows are held to the oracle's dumps: the edges and a fixed random choice, ascending."""
    rng = np.random.default_rng(6)
    return np.unique(np.concatenate([np.asarray(SY_EDGES), rng.choice(n, count - len(SY_EDGES), replace=False)]))


LV_N, LV_A_STEPS, LV_STEPS, LV_EVERY = 65536, 5, 20, 97
LV_SEEDS = (1, 2)  # engine A, whose levels are read; engine B (and its twin), into which they are installed


def spoil_levels(levels, n, side):
    """(levels, indices): every 97th row of `levels` (numpy fields, row k meant for env k) spoiled so that every refusal
    occurs — an index outside the batch, a tile byte of 2, the agent outside the map, the goal on the agent, a floor picture
    that does not exist — in turn."""
    levels = type(levels)(*(np.array(x) for x in levels))
    indices = np.arange(n, dtype=np.int32)
    for j, row in enumerate(range(0, n, LV_EVERY)):
        kind = j % 5
        if kind == 0:
            indices[row] = n if j % 2 else -1
        elif kind == 1:
            levels.tiles[row, side * side - 1] = 2
        elif kind == 2:
            levels.agent_cell[row] = side * side if j % 2 else -1
        elif kind == 3:
            levels.goal_cell[row] = levels.agent_cell[row]
        else:
            levels.background[row] = 9
    return levels, indices


def levels_plan_holds(status):
    """Every refusal status occurs at least 10 times, and at least 90 % of the rows are installed."""
    counts = np.bincount(status, minlength=6)
    return bool((counts[1:6] >= 10).all() and counts[0] >= 0.9 * status.size)
