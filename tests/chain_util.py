"""The protocol "churn, then play", stated once: tests/test_chain_gpu.py runs it on the HIP engine beside the oracle,
tests/test_chain.py runs it on the oracle alone, beside a WRONG oracle (OracleVec.set_fresh_containers), and asserts that
the two part company within the run, so the GPU tests are known not to be vacuous before a GPU is touched.

What is held.  In six of the seven games sprites are drawn in the iteration order of a std::unordered_set<int>; the sets
are clear()ed at every new level and keep their bucket arrays, so an env that once played a level with many entities lists
the sprites of a later, smaller level in another order than a fresh env would.  The engine restates that as carried bucket
counts (pg_setorder.h, the I_HASH_* words, chain_keep / chain_restore in pg_prefetch.h).  Random play rarely takes an env
past its second level, so almost everything else in the suite runs where carried counts equal fresh ones.

Going deep costs no play: Env::reset (oracle/pgo_env.h) is an optional reseed plus new_level() on the containers as they
stand, so every reset of an env moves it one level down its chain.

Churn: R rounds of masked resets with no play between them.  Round r resets the envs with (env + r) % 3 != 0 without seeds
(depths differ across the batch); every fourth round (r % 4 == 3) is instead a reseeding reset of the envs with
env % 5 == 2, the seeds 7 * env - 40 - r (negative for the first envs named); after every fourth round one plain step, so
that some resets find their shadow slot filled by the engine's side stream and others generate inside the call.
Play: P steps of synthetic_actions; auto-resets go on down the chain.

n = 65: one wavefront and one lane.  n = 1 for the default and the complete render path.

R and P per (game, mode) come from tools/chain_census.py (profiles/chain/census.md): R puts the median env at least 20
levels deep, P is the length at which the two oracles differ in at least MIN_WITNESS env-steps spread over MIN_ENVS envs
(chaser and caveflyer with room to spare; climber and coinrun, under the cast, only just: 39 and 41 env-steps in 5 envs —
a change to the agents of scripted_play_util.py moves them, and the CPU half then says so).  A game with no witness at any
affordable length is left out and named in the census file.
"""
import ctypes

import numpy as np

from episodes_util import synthetic_actions
from test_modes import EASY, EXTREME, HARD, MEMORY  # noqa: F401

N, SMALL_N, SEED_BASE, RUN_SEED = 65, 1, 23, 11
MIN_DEPTH, MIN_WITNESS, MIN_ENVS = 20, 20, 5

# (game, mode) -> (R, P, whether the cast plays): profiles/chain/census.md.  R = 44 leaves every env 22 levels deep and the
# reseeded ones 33.  P: the coverage condition is first met at step 15 (chaser), 19 (caveflyer memory) and 191 (climber, under
# the cast; 585 under random play) of the steps counted from the churn's first, 11 of which are the churn's.  Left out, with
# the census's reasons: bossfight, maze and jumper (no witness at all), caveflyer easy and hard (none in 1 200 steps),
# chaser's other modes (no more than the default).  coinrun shows nothing under random play in 1 200 steps; under the cast
# its first witness is at step 346 and the condition is met at step 1 008 (41 env-steps in 5 envs by step 1 110), hence the
# one long case.
CASES = {("chaser", EASY): (44, 40, False), ("caveflyer", MEMORY): (44, 60, False), ("climber", HARD): (44, 230, True),
         ("coinrun", HARD): (44, 1100, True)}
# records and snapshots: coinrun and a room game
RECORD_CASES = [("caveflyer", MEMORY), ("coinrun", HARD)]
# One env: (game, mode) -> env_offset.  The churn's masks, the seeds and the actions are functions of the global env index,
# so a one-env batch at env_offset k is env k of the 65 over again, and k is chosen among the envs that are witnesses there:
# chaser's env 32 is one of the reseeded envs (33 levels deep); caveflyer's reseeded envs are no witnesses, env 20 shows the
# most (24 env-steps).  The bound for one env: it differs from the fresh-containers oracle at least once.  coinrun and climber
# have no one-env case: their cast draws from one random stream for the whole batch, so a batch of one plays another game.
SMALL_CASES = {("chaser", EASY): 32, ("caveflyer", MEMORY): 20}


def cases():
    return sorted(CASES)


def churn_round(r, n=N, env_offset=0):
    """(mask, seeds or None, whether a plain step follows) of churn round r; `env` is the global index env_offset + row."""
    i = np.arange(n) + env_offset
    if r % 4 == 3:
        return (i % 5 == 2).astype(np.uint8), (i * 7 - 40 - r).astype(np.int32), True
    return ((i + r) % 3 != 0).astype(np.uint8), None, False


def actions(t, n=N, env_offset=0):
    return synthetic_actions(RUN_SEED, t, n, env_offset)


class Depth:
    """How many levels down its chain each env is: the resets that named it and the auto-resets it was served."""

    def __init__(self, n):
        self.depth = np.zeros(n, np.int64)
        self.pending = np.zeros(n, bool)
        self.reseeding = 0

    def reset(self, mask, seeds):
        self.depth += mask != 0
        self.pending[mask != 0] = False
        self.reseeding += seeds is not None

    def step(self, done):
        self.depth += self.pending
        self.pending = done != 0

    def median(self):
        return float(np.median(self.depth))


def cast_actions(game, mode):
    """The play phase under the agents of tests/scripted_play_util.py instead of random play: actions_of(t, ora), read
    from the oracle's dumps before the step.  coinrun and climber play so (see CASES)."""
    import scripted_play_util as sp
    c, rng = sp.columns(game, mode), np.random.default_rng(sp.POLICY_SEED)
    return lambda t, ora: sp.choose_actions(game, mode, sp.Dumps(ora, c), t, rng)


def run(ora, R, P, each_reset=None, each_step=None, after_churn=None, n=N, actions_of=None, env_offset=0):
    """The protocol on an OracleVec already made (and so already given its first reset).  actions_of(t, ora): the play
    phase's actions where they are not synthetic_actions (the churn's plain steps always are).  each_reset(r, mask, seeds, obs)
    after every churn reset, each_step(t, actions, obs, reward, done) after every step (t counts the churn's plain steps
    and the play's together), after_churn() between the two.  Returns (Depth after the churn, Depth at the end)."""
    d = Depth(n)
    t = 0

    def step(play=False):
        nonlocal t
        a = actions_of(t, ora) if play and actions_of else actions(t, n, env_offset)
        obs, reward, done = ora.step(a)
        d.step(done)
        if each_step:
            each_step(t, a, obs, reward, done)
        t += 1

    for r in range(R):
        mask, seeds, then_step = churn_round(r, n, env_offset)
        obs = ora.reset(mask=mask, seeds=seeds)
        d.reset(mask, seeds)
        if each_reset:
            each_reset(r, mask, seeds, obs)
        if then_step:
            step()
    churned = Depth(n)
    churned.depth, churned.reseeding = d.depth.copy(), d.reseeding
    if after_churn:
        after_churn()
    for _ in range(P):
        step(play=True)
    return churned, d


# same-step installs (tests/test_chain_gpu.py test_same_step_installs_deep_in_the_chain): the play phase under step_episodes
# with a time limit of 12, so that every env ends at least three times, and a ring of 4.  (game, mode) -> steps of random
# play: the two oracles must differ by the coverage condition in the frames the steps leave AND in a terminal frame of the
# ring.  caveflyer memory: 60 env-steps in 8 envs, a terminal frame at step 44.  chaser: the condition is met at step 59,
# terminal frames at steps 82 and 94.  climber (2 env-steps) and coinrun (none) show nothing under 40 steps of random play
# and their witnesses under the cast are hundreds of steps apart, further than any time limit that ends every env three
# times in an affordable run: they have no same-step case.
EPISODE_LIMIT, EPISODE_RING = 12, 4
SAME_STEP_CASES = {("caveflyer", MEMORY): 40, ("chaser", EASY): 100}


def run_same_step(model, R, play, eng=None, check_step=None, each=None):
    """The churn on an EpisodeModel (and an engine beside it), then `play` steps of step_episodes, everything checked after
    every step by check_step(eng, model, got, t).  Returns the fewest endings any env had during the play."""
    n = model.n
    t = 0
    for r in range(R):
        mask, seeds, then_step = churn_round(r, n)
        model.o.reset(mask=mask, seeds=seeds)
        named = mask != 0
        model.o.reward[named], model.o.done[named] = 0.0, 0  # (what pgv_reset leaves in the rows of the envs it names)
        model.running_return[named], model.running_length[named] = 0.0, 0
        if eng is not None:
            assert np.array_equal(eng.reset(mask=mask, seeds=seeds), model.obs), "churn round %d" % r
        if then_step:
            a = actions(t, n)
            want = model.plain_step(a)
            if eng is not None:
                obs, reward, done = eng.plain_step(a)
                assert np.array_equal(obs, want[0]) and np.array_equal(done, want[2]), "the churn's plain step %d" % t
                assert np.array_equal(reward.view(np.uint32), want[1].view(np.uint32)), "the churn's plain step %d: reward bits" % t
            t += 1
    ended = np.zeros(n, int)
    for _ in range(play):
        a = actions(t, n)
        got = eng.step(a) if eng is not None else None
        model.step(a)
        if eng is not None:
            check_step(eng, model, got, t)
        if each:
            each(t, model)
        ended += model.ended != 0
        t += 1
    return int(ended.min())


def compare_same_step(game, mode, R, play):
    """run_same_step on the model over the good oracle and on one over the fresh-containers oracle (random play: the two
    runs take the same actions).  Returns (Witnesses of the frames the steps leave, the steps at which the ring's terminal
    frames differ, the fewest endings any env had)."""
    from episodes_util import SAME_STEP, EpisodeModel
    rows = []
    for fresh in (False, True):
        m = EpisodeModel(game, N, SAME_STEP, EPISODE_LIMIT, EPISODE_RING, seed_base=SEED_BASE, distribution_mode=mode)
        if fresh:
            m.o.set_fresh_containers(True)
        m.first_reset()
        seen = []
        fewest = run_same_step(m, R, play, each=lambda t, model: seen.append((t, model.obs.copy(), model.final_obs.copy())))
        m.close()
        rows.append(seen)
    w, terminal = Witnesses(N), []
    for (t, obs, final), (_, obs2, final2) in zip(*rows):
        w.add("step %d" % t, frames=(obs != obs2).any(axis=1))
        if final.shape != final2.shape or not np.array_equal(final, final2):
            terminal.append(t)
    return w, terminal, fewest


# Dropped assignments (tests/test_chain_gpu.py test_dropped_assignments_go_back_to_the_carried_counts): after the churn every
# env is assigned a level; after `wait` plain steps — 3: the engine's side stream has built the level ahead on a fresh chain
# and set the env's carried counts aside (chain_keep); 0: the assignment comes right before the reset — a reset WITH seeds of
# the even envs drops the assignment and must go back to the carried counts (chain_restore), and a reset without seeds of
# the odd envs consumes theirs; then P steps of random play, all of it held to AssignModel.  (game, mode) -> P.  caveflyer
# memory stands in for the games the issue names: jumper has no witness at all, and in coinrun a model whose dropped envs got
# fresh containers differs in 3 envs in 2 000 steps of the cast (profiles/chain/census.md); caveflyer has the same
# G::chain_counts behind the same chain_keep / chain_restore of pg_prefetch.h.
DROP_WAITS = (3, 0)
# P = 420: the model whose dropped envs got fresh containers differs in 5 envs from step 158 (wait 3) and step 321 (wait 0)
# on, and in 6 from step 403 on in both (99 and 122 env-steps in 900 steps; no seventh env by then).
DROP_CASES = {("caveflyer", MEMORY): 420}
MIN_DROP_ENVS = 5


def run_dropped(vec, assign, R, wait, P, n=N, check=None, before_drop=None, after_drop=None, each_step=None):
    """vec: an AssignModel, or tests/test_assign_levels_gpu.py's Pair of an engine and a model; assign(indices, levels);
    check(what) after every reset and step; before_drop(mask) / after_drop() round the seeded reset; each_step(t, obs) after
    every step of the play.  Returns the mask of the seeded reset."""
    from assign_util import scheduled_level
    vec.first_reset()
    if check:
        check("first reset")
    t = 0

    def step(what):
        nonlocal t
        out = vec.step(actions(t, n))
        if check:
            check("%s step %d" % (what, t))
        t += 1
        return out

    for r in range(R):
        mask, seeds, then_step = churn_round(r, n)
        vec.reset(mask=mask, seeds=seeds)
        if check:
            check("churn round %d" % r)
        if then_step:
            step("the churn's")
    everyone = list(range(n))
    assign(everyone, [scheduled_level(e, 1) for e in everyone])
    for _ in range(wait):
        step("waiting")
    i = np.arange(n)
    even, seeds = (i % 2 == 0).astype(np.uint8), (i * 5 - 60).astype(np.int32)
    if before_drop:
        before_drop(even)
    vec.reset(mask=even, seeds=seeds)
    if after_drop:
        after_drop()
    if check:
        check("the seeded reset that drops the assignments")
    vec.reset(mask=1 - even)
    if check:
        check("the reset without seeds that consumes the assignments")
    for _ in range(P):
        obs = step("play")[0]
        if each_step:
            each_step(t - 1, obs)
    return even


def compare_dropped(game, mode, R, wait, P):
    """run_dropped on an AssignModel and on one whose envs with a dropped assignment are given fresh containers at the
    seeded reset (and only there).  Returns (Witnesses over the play, envs whose assignment the seeded reset dropped,
    assignments consumed by the reset without seeds)."""
    from assign_util import AssignModel
    seen, dropped, consumed = [], None, 0
    for fresh in (False, True):
        m = AssignModel(game, N, seed_base=SEED_BASE, mode=mode)
        frames, named = [], []

        def before_drop(mask):
            named.extend(e for e in range(N) if mask[e] and m.assigned[e] is not None)
            if fresh:
                for e in named:
                    m.L.pgo_set_fresh_containers(m.h[e], 1)

        def after_drop():
            for e in named:
                m.L.pgo_set_fresh_containers(m.h[e], 0)

        run_dropped(m, m.assign, R, wait, P, before_drop=before_drop, after_drop=after_drop, each_step=lambda t, obs: frames.append((t, obs.copy())))
        dropped, consumed = named, m.assigned_by_reset
        m.close()
        seen.append(frames)
    w = Witnesses(N)
    for (t, a), (_, b) in zip(*seen):
        w.add("step %d" % t, frames=(a != b).any(axis=1))
    return w, dropped, consumed


def churn_steps(R):
    """The plain steps the churn takes: the play's first step has this number."""
    return sum(1 for r in range(R) if r % 4 == 3)


def _dump(fn, h, env, ctype, dtype):
    """A parity dump through a numpy buffer (oracle_util._dump goes through a Python list: every env of every case is too
    many for that)."""
    n = fn(h, env, ctypes.cast(None, ctypes.POINTER(ctype)), 0)
    assert n >= 0
    buf = np.zeros(max(1, n), dtype)
    assert fn(h, env, buf.ctypes.data_as(ctypes.POINTER(ctype)), n) >= n
    return buf[:n]


def _dumps(v):
    """(state dump, tile dump) of an OracleVec or an EngineVec."""
    if hasattr(v, "set_fresh_containers"):
        return v.L.pgo_vec_dump_state, v.L.pgo_vec_dump_tiles
    return v.L.pgv_dump_state, v.L.pgv_dump_tiles


def state_rows(v, n):
    """Every env's state row as bit patterns, of an OracleVec or an EngineVec."""
    fn = _dumps(v)[0]
    return [_dump(fn, v.h, e, ctypes.c_float, np.float32).view(np.uint32) for e in range(n)]


def tile_rows(v, n):
    fn = _dumps(v)[1]
    return [_dump(fn, v.h, e, ctypes.c_uint8, np.uint8) for e in range(n)]


def assert_same_rows(name, eng, ora, n, when, env_in=None):
    """State and tile rows of all envs, engine against oracle: the same lengths, then every value bit for bit.  env_in: slot p
    of the engine holds the oracle's env env_in[p]."""
    for what, rows in (("state", state_rows), ("tiles", tile_rows)):
        wants = rows(ora, n)
        for e, (got, want) in enumerate(zip(rows(eng, n), wants if env_in is None else [wants[i] for i in env_in])):
            assert got.size == want.size, "%s, %s: %s of env %d has %d values, the oracle's %d" % (name, when, what, e, got.size, want.size)
            assert np.array_equal(got, want), "%s, %s: %s of env %d" % (name, when, what, e)


class Witnesses:
    """What differs between two runs of the protocol, per output: env-steps and the envs they lie in."""
    KINDS = ("frames", "state", "reward", "done")

    def __init__(self, n):
        self.n = n
        self.first = {k: None for k in self.KINDS}
        self.count = {k: 0 for k in self.KINDS}
        self.any = np.zeros(n, np.int64)  # env-steps that differ in anything, per env
        self.calls = 0
        self.met_at = None  # the call at which covers() first held

    def add(self, call, **differs):
        every = np.zeros(self.n, bool)
        for k, rows in differs.items():
            rows = np.asarray(rows, bool)
            if rows.any():
                self.count[k] += int(rows.sum())
                if self.first[k] is None:
                    self.first[k] = (call, int(np.nonzero(rows)[0][0]))
                every |= rows
        self.any += every
        self.calls += 1
        if self.met_at is None and self.covers():
            self.met_at = call

    env_steps = property(lambda self: int(self.any.sum()))
    envs = property(lambda self: int((self.any > 0).sum()))

    def covers(self):
        return self.env_steps >= MIN_WITNESS and self.envs >= MIN_ENVS


def compare_oracles(game, mode, R, P, n=N, states=True, threads=1, cast=False, env_offset=0):
    """The protocol on the good oracle and on the fresh-containers one, side by side (under the cast the wrong oracle
    replays the good run's actions).  Calls are named "reset r" and
    "step t".  Returns (Witnesses, Depth after the churn, Depth at the end, auto-resets served)."""
    from oracle_util import OracleVec
    good = OracleVec(game, n, seed_base=SEED_BASE, mode=mode, threads=threads, env_offset=env_offset)
    bad = OracleVec(game, n, seed_base=SEED_BASE, mode=mode, threads=threads, env_offset=env_offset)
    bad.set_fresh_containers(True)
    w = Witnesses(n)
    ends = 0

    def rows():
        if not states:
            return np.zeros(n, bool)
        return np.array([not np.array_equal(a, b) for a, b in zip(state_rows(good, n), state_rows(bad, n))])

    def each_reset(r, mask, seeds, obs):
        other = bad.reset(mask=mask, seeds=seeds)
        w.add("reset %d" % r, frames=(obs != other).any(axis=1), state=rows())

    def each_step(t, a, obs, reward, done):
        nonlocal ends
        ends += int((done != 0).sum())
        o2, r2, d2 = bad.step(a)
        w.add("step %d" % t, frames=(obs != o2).any(axis=1), state=rows(),
              reward=reward.view(np.uint32) != r2.view(np.uint32), done=done != d2)

    try:
        churned, end = run(good, R, P, each_reset, each_step, n=n, actions_of=cast_actions(game, mode) if cast else None, env_offset=env_offset)
    finally:
        good.close(), bad.close()
    return w, churned, end, ends
