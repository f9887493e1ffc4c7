"""pgv_save_state / pgv_load_state (checkpoint / resume) held to the CPU oracle.

What a snapshot promises: saving is transparent — the engine that saved goes on exactly as one
that never did — and the blob resumes in ANY engine of the same configuration, whatever that engine did before: much of
what a step reads is scratch outside the blob (render pre-pass tables, chaser's base layers, the second buffers of the
random streams and their selectors, the host's generator cadence), rebuilt by Game::state_loaded and pregen().

The moments at which snapshots are taken come from the oracle alone (`snapshot_plan`): the code under test has no say in
them.  One CPU test checks that the plan is not vacuous for any case; everything else needs an MI355X.
"""
import time
from ctypes import c_void_p

import numpy as np
import pytest

from oracle_util import OracleVec, assert_same_dump, oracle, oracle_state, register_textures
from test_modes import NON_DEFAULT
from test_parity_gpu import FRAME_GAMES  # the seven games, and the four modes with a camera of their own

from procgen2_amd import lib as pglib

GAMES = ("coinrun", "maze", "bossfight", "climber", "caveflyer", "chaser", "jumper")
N, SEED_BASE, RUN_SEED = 200, 1201, 7  # n: not a multiple of 64 or 128
FOREIGN_SEED, FOREIGN_STEPS, FOREIGN_RUN_SEED = 99, 37, 3  # what a foreign engine did before it is handed the snapshot


class Case:
    def __init__(self, game, tag="", mode=0, game_flags=0, num_levels=0, start_level=0, env_offset=0, host_actions=False):
        self.game, self.mode, self.game_flags = game, mode, game_flags
        self.num_levels, self.start_level, self.env_offset, self.host_actions = num_levels, start_level, env_offset, host_actions
        self.steps = 560 if game == "maze" else 400  # maze: through its 500-step cap
        self.id = game + ("-" + tag if tag else "")

    def config(self):
        """What the engine and the oracle are both made with (seed_base aside)."""
        return dict(env_offset=self.env_offset, num_levels=self.num_levels, start_level=self.start_level, mode=self.mode,
                    game_flags=self.game_flags)


CASES = ([Case(g) for g in GAMES] +
         [Case(g, "mode%d" % m, mode=m) for g, m in NON_DEFAULT] +
         [Case("chaser", "float_abs", game_flags=pglib.CHASER_FLOAT_ABS),
          Case("jumper", "float_abs", game_flags=pglib.JUMPER_FLOAT_ABS),
          Case("coinrun", "flags15", game_flags=15),
          Case("coinrun", "levels7", num_levels=7, start_level=50),
          Case("bossfight", "levels7", num_levels=7, start_level=50),
          Case("bossfight", "offset40960", env_offset=40960),
          Case("chaser", "host_actions", host_actions=True)])


def _actions(L, run_seed, step, n, offset=0):
    return np.array([L.pgo_synthetic_action(run_seed, step, offset + e) for e in range(n)], np.int32)


def _host_threads():
    import bench
    return max(1, min(16, bench.usable_cores()))


def oracle_dones(case, n=N, seed_base=SEED_BASE, run_seed=RUN_SEED):
    """dones[steps, n] of the case's whole run, from the oracle alone (drawing off: seconds)."""
    ora = OracleVec(case.game, n, seed_base=seed_base, render=False, threads=1, **case.config())
    threads = _host_threads()
    dones = np.zeros((case.steps, n), np.uint8)
    for s in range(case.steps):
        dones[s] = ora.step(None, run_seed=run_seed, threads=threads)[2]
    ora.close()
    return dones


def snapshot_plan(case, dones):
    """{step index: names} — the steps AFTER which a snapshot is taken (-1: after reset, before any step):
    P0 after reset; P1 / P2 the first step >= 30 with an odd / even index in which an env ended (the snapshot holds pending
    auto-resets, at both parities of the step index: pg_prefetch.h reset_due_mark, chaser's State::parity); P3 the first
    step >= 150 in which an env ended (most bossfight / chaser streams have changed buffers by then); maze: P4, the step
    with the most ends (the 500-step cap).  A name is missing where no such step exists."""
    ended = dones.any(axis=1)
    named = {"P0": -1}
    for name, first, parity in (("P1", 30, 1), ("P2", 30, 0), ("P3", 150, None)):
        hits = [s for s in range(first, len(ended)) if ended[s] and (parity is None or s % 2 == parity)]
        if hits:
            named[name] = hits[0]
    if case.game == "maze":
        named["P4"] = int(dones.sum(axis=1).argmax())
    plan = {}
    for name, s in named.items():
        plan.setdefault(s, []).append(name)
    return plan


def _check_plan(case, dones, plan):
    """The conditions that keep the main test from passing vacuously."""
    names = {name for ns in plan.values() for name in ns}
    assert {"P1", "P2", "P3"} <= names, "%s: plan %r lacks a step (pick another seed_base for this case)" % (case.id, plan)
    last = max(plan)
    assert dones[last + 1:].any(), "%s: no episode ends after the last snapshot (step %d)" % (case.id, last)
    if case.game == "maze":
        assert int(dones[max(s for s, ns in plan.items() if "P4" in ns)].sum()) > N // 4, "maze: the cap ends a large share at once"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_the_snapshot_plan_holds_on_the_oracle(case):
    dones = oracle_dones(case)
    plan = snapshot_plan(case, dones)
    _check_plan(case, dones, plan)
    after = int(dones[max(plan) + 1:].sum())
    print("%s: plan %r, %d ends, %d after the last snapshot" % (case.id, plan, int(dones.sum()), after))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _same_outputs(tag, got, want):
    """Every observation byte, reward bit pattern and done flag of one step (engine, oracle)."""
    (oe, re_, de), (oo, ro, do) = got, want
    assert np.array_equal(de, do), "%s: done" % tag
    assert np.array_equal(re_.view(np.uint32), ro.view(np.uint32)), "%s: reward bits" % tag
    if not np.array_equal(oe, oo):
        bad = np.nonzero((oe != oo).any(axis=1))[0]
        raise AssertionError("%s: obs differ in %d envs (first env %d, %d bytes)" %
                             (tag, bad.size, bad[0], int((oe[bad[0]] != oo[bad[0]]).sum())))


def _foreign_engine(case, n, fresh=False):
    """An engine of the case's configuration that belongs to another rollout: another seed_base, reset and stepped with
    other actions — its scratch, stream selectors, prefetch slots, base layers and step counter are all foreign.  fresh:
    as a new process has it, never reset or stepped."""
    from engine_util import EngineVec
    eng = EngineVec(case.game, n, seed_base=FOREIGN_SEED, **case.config())
    if not fresh:
        eng.reset()
        for _ in range(FOREIGN_STEPS):
            eng.step_quiet(run_seed=FOREIGN_RUN_SEED)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_saving_and_resuming_stay_on_the_oracle(case):
    """Engine A and the oracle in lockstep for the whole run, every byte of every step.  After each plan step A saves (so
    from then on A is an engine that saved, held to the oracle: streams_home_kernel and whatever else prepare_save does
    must be harmless), and a foreign engine B loads the snapshot, must show the oracle's outputs and states at once, and
    is then stepped with A's actions and held to the oracle on every byte until the END of the run — the plan guarantees
    episode ends after the last snapshot.  The B of P2 is a freshly made engine.

    Seen to fail when streams_home_kernel copies nothing (A, the step after P3's save: bossfight, chaser), when chaser's
    state_loaded keeps base_valid_ (B's first step) and when state_loaded leaves mt_sel alone (B of P0, steps 75-150).  The
    chaser float_abs case cannot see the two stream changes: that reading of `abs` draws at every sixteenth sub-step only,
    so in 400 steps its streams hardly leave their first buffer; it is here for what else the flag touches."""
    from engine_util import EngineVec
    n = N
    dones = oracle_dones(case)
    plan = snapshot_plan(case, dones)
    _check_plan(case, dones, plan)
    threads = _host_threads()
    A = EngineVec(case.game, n, seed_base=SEED_BASE, **case.config())
    ora = OracleVec(case.game, n, seed_base=SEED_BASE, **case.config())
    L = ora.L
    followers = []  # (name, engine B)

    def snapshot(s):
        names = "+".join(plan[s])
        tag = "%s %s (after step %d)" % (case.id, names, s)
        snap = A.save_state()
        if "P1" in plan[s]:  # saving twice: the first save left nothing behind that the second one sees
            assert np.array_equal(A.save_state(), snap), tag + ": a second save at once differs from the first"
        B = _foreign_engine(case, n, fresh="P2" in plan[s])
        followers.append((names, B))
        B.load_state(snap)
        _same_outputs(tag + ", right after the load", B._fetch(), (ora.obs, ora.reward, ora.done))
        for e in range(0, n, 25):
            assert_same_dump(B.state(e), ora.state(e), "%s: state env %d after the load" % (tag, e))
            assert_same_dump(B.tiles(e), ora.tiles(e), "%s: tiles env %d after the load" % (tag, e))

    _same_outputs(case.id + " reset", (A.reset(), A.reward, A.done), (ora.reset_obs(), ora.reward, ora.done))
    if -1 in plan:
        snapshot(-1)
    for s in range(case.steps):
        a = _actions(L, RUN_SEED, s, n, case.env_offset) if case.host_actions else None
        want = ora.step(a, run_seed=RUN_SEED, threads=threads)
        assert np.array_equal(want[2], dones[s]), "the oracle's own plan run differs at step %d" % s
        _same_outputs("%s A step %d" % (case.id, s), A.step(a, run_seed=RUN_SEED), want)
        for names, B in followers:
            _same_outputs("%s B of %s step %d" % (case.id, names, s), B.step(a, run_seed=RUN_SEED), want)
        if s in plan:
            snapshot(s)
    assert len(followers) == len(plan) <= (5 if case.game == "maze" else 4)  # (and A: five engines alive at once, six for maze with its P4)
    for names, B in followers + [("A", A)]:
        for e in range(0, n, 25):
            assert_same_dump(B.state(e), ora.state(e), "%s %s: state env %d at the end" % (case.id, names, e))
            assert_same_dump(B.tiles(e), ora.tiles(e), "%s %s: tiles env %d at the end" % (case.id, names, e))
        B.close()
    ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 129])
@pytest.mark.parametrize("game", ["bossfight", "chaser"])
def test_snapshot_at_sizes_around_a_wavefront(game, n):
    """streams_home_kernel takes a wavefront per 64 envs (`e < s.n`); n = 1 is what the Appendix C trace test runs.  Saves
    after steps 61 and 150, each loaded into a foreign engine; everyone against the oracle for 260 steps."""
    from engine_util import EngineVec
    case = Case(game)
    A = EngineVec(game, n, seed_base=SEED_BASE)
    ora = OracleVec(game, n, seed_base=SEED_BASE)
    _same_outputs("reset", (A.reset(), A.reward, A.done), (ora.reset_obs(), ora.reward, ora.done))
    followers = []
    for s in range(260):
        want = ora.step(None, run_seed=RUN_SEED)
        _same_outputs("%s n=%d A step %d" % (game, n, s), A.step(None, run_seed=RUN_SEED), want)
        for at, B in followers:
            _same_outputs("%s n=%d B of step %d, step %d" % (game, n, at, s), B.step(None, run_seed=RUN_SEED), want)
        if s in (61, 150):
            snap = A.save_state()
            B = _foreign_engine(case, n)
            followers.append((s, B))
            B.load_state(snap)
            _same_outputs("%s n=%d right after the load at step %d" % (game, n, s), B._fetch(), want)
            for e in sorted({0, n // 2, n - 1}):
                assert_same_dump(B.state(e), ora.state(e), "state env %d after the load at step %d" % (e, s))
    for _, B in followers:
        B.close()
    A.close()
    ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("game,saves", [("bossfight", (60, 150)), ("chaser", (60, 150)), ("maze", (300, 450))],
                         ids=["bossfight", "chaser", "maze"])
def test_snapshot_at_full_size(game, saves, capsys):
    """65 536 envs (bossfight, chaser: prepare_save's grid is 1 024 wavefronts; maze: a generator launch every second step
    and the mass time-out at step 500).  T never saves, S saves after two steps and goes on, F is foreign and loads S's
    second snapshot; 100 steps later (maze: across step 500) the three agree on every byte of every env — rewards and
    dones of every step on the way.  T is what test_every_env_at_full_size_matches_the_oracle holds to the oracle."""
    from engine_util import EngineVec
    n = 65536
    case = Case(game)
    T, S = EngineVec(game, n, seed_base=1), EngineVec(game, n, seed_base=1)
    T.reset()
    S.reset()
    snap = None
    for s in range(saves[1] + 1):
        T.step_quiet(run_seed=RUN_SEED)
        S.step_quiet(run_seed=RUN_SEED)
        if s in saves:
            snap = None  # (one snapshot in host memory at a time)
            t0 = time.time()
            snap = S.save_state()
            took = time.time() - t0
    with capsys.disabled():
        print("\n%s: pgv_snapshot_bytes at %d envs = %d (%.1f MB), saved in %.2f s" % (game, n, snap.size, snap.size / 1e6, took))
    assert snap.size == S.L.pgv_snapshot_bytes(S.h)
    F = _foreign_engine(case, n)
    F.load_state(snap)
    del snap
    want = T._fetch()
    _same_outputs("%s S at the second save" % game, S._fetch(), want)
    _same_outputs("%s F right after the load" % game, F._fetch(), want)
    ends = 0
    for s in range(100):
        for v in (T, S, F):
            v.step_quiet(run_seed=RUN_SEED)
        rt, dt = T.fetch_scalars()
        ends += int(dt.sum())
        for name, v in (("S", S), ("F", F)):
            r, d = v.fetch_scalars()
            assert np.array_equal(d, dt) and np.array_equal(r.view(np.uint32), rt.view(np.uint32)), (game, name, s)
        if s in (49, 99):
            want = T._fetch()
            _same_outputs("%s S %d steps on" % (game, s + 1), S._fetch(), want)
            _same_outputs("%s F %d steps on" % (game, s + 1), F._fetch(), want)
    assert ends > n // 2 if game == "maze" else ends > 1000, ends
    for e in range(0, n, 4099):
        for name, v in (("S", S), ("F", F)):
            assert_same_dump(v.state(e), T.state(e), "%s %s: state env %d" % (game, name, e))
            assert_same_dump(v.tiles(e), T.tiles(e), "%s %s: tiles env %d" % (game, name, e))
    for v in (T, S, F):
        v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("game", ["maze", "chaser"])  # with prefetch slots, and without
def test_the_level_plan_lies_in_the_snapshot_where_its_listing_says(game):
    """The last 32·n bytes of a snapshot's state blob are the level plan's arrays at the offsets that
    tests/cpp/test_engine_layout.cpp pins for the listing (pg_carve.h list_plan) — the engine binds its kernels' pointers with
    that listing, so what they wrote is found there: word array 0 the seeds the envs were made with, word array 3 what
    pgv_level_numbers shows, byte array 1 what pgv_level_known shows.  And the snapshot's size is its parts'."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n, seed_base, env_offset = 65, 4242, 7
    v = ProcgenVecEnv(game, n, seed_base=seed_base, env_offset=env_offset, num_levels=5, start_level=100)
    for _ in range(20):
        v.step_synthetic(RUN_SEED)
    snap = v.save_state()
    numbers = v.level_numbers.view(torch.int32).cpu().numpy().view(np.uint32)
    known = v.level_known.cpu().numpy()
    v.close()
    state_bytes = int(snap[16:24].view(np.uint64)[0])  # the header: magic, game, n, env_offset, then the blob's length
    assert snap.size == 48 + state_bytes + n * (4 + 1 + 1 + 12288)
    plan = snap[48 + state_bytes - 32 * n:48 + state_bytes]
    assert np.array_equal(plan[12 * n:16 * n].view(np.uint32), numbers)
    assert np.array_equal(plan[28 * n + n:28 * n + 2 * n], known)
    assert np.array_equal(plan[0:4 * n].view(np.uint32), (seed_base + env_offset + np.arange(n)).astype(np.uint32))
    assert known.all() and ((numbers >= 100) & (numbers < 105)).all()  # (level-seed mode: the words compared are not blank)


# ---------------------------------------------------------------------------------------------------------------------
# human-size frames and the camera (D15)
# ---------------------------------------------------------------------------------------------------------------------
class _SingleEnvs:
    """n single oracle envs driven with the engine's auto-reset policy (the reset takes the step after the episode's last)."""

    def __init__(self, game, n, seed_base, mode=0):
        register_textures(game)
        self.L = oracle()
        self.hs = [self.L.pgo_make_mode(game.encode(), seed_base + i, 1, mode) for i in range(n)]
        for h in self.hs:
            self.L.pgo_reset(h, 0, 0)
        self.pending = [False] * n
        self.reward, self.done = np.zeros(n, np.float32), np.zeros(n, np.uint8)

    def obs(self):
        return np.stack([np.ctypeslib.as_array(self.L.pgo_obs(h), shape=(12288,)) for h in self.hs])

    def step(self, a):
        for i, h in enumerate(self.hs):
            if self.pending[i]:
                self.L.pgo_reset(h, 0, 0)
                self.pending[i] = False
                self.reward[i], self.done[i] = 0.0, 0
            else:
                self.L.pgo_step(h, int(a[i]))
                self.pending[i] = bool(self.L.pgo_terminated(h))
                self.reward[i], self.done[i] = self.L.pgo_reward(h), int(self.L.pgo_terminated(h))
        return self.obs(), self.reward, self.done

    def reset_one(self, i):
        self.L.pgo_reset(self.hs[i], 0, 0)
        self.pending[i] = False

    def frame(self, i, w, h):
        want = np.zeros((h, w, 3), np.uint8)
        self.L.pgo_render_frame(self.hs[i], w, h, want.ctypes.data_as(c_void_p))
        return want

    def close(self):
        for h in self.hs:
            self.L.pgo_close(h)


def _same_frame(tag, got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError("%s: %d pixels differ, first at (y=%d, x=%d)" % (tag, len(bad), bad[0][0], bad[0][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("game,mode", FRAME_GAMES)
def test_human_frames_of_a_loaded_snapshot_match_the_oracle(game, mode):
    """The frame kernels read what lies outside the blob too (chaser's layers, jumper's atlas extension, the pre-pass
    tables): 60 steps, save, load into a foreign engine, and its W×H frames are the oracle's — then 30 more steps of that
    engine against the oracle, human frames having been taken in between."""
    from engine_util import EngineVec
    n, seed = 6, 71
    case = Case(game, mode=mode)
    A = EngineVec(game, n, seed_base=seed, mode=mode)
    ora = _SingleEnvs(game, n, seed, mode)
    assert np.array_equal(A.reset(), ora.obs()), "reset frame"
    for s in range(60):
        a = _actions(ora.L, 4, s, n)
        _same_outputs("%s step %d" % (game, s), A.step(a), ora.step(a))
    snap = A.save_state()
    A.close()
    B = _foreign_engine(case, n)
    B.load_state(snap)
    for env in (0, 2, 5):
        for w, h in ((160, 160), (200, 120)):
            _same_frame("%s mode %d env %d %dx%d" % (game, mode, env, w, h), B.frame(env, w, h), ora.frame(env, w, h))
    for s in range(60, 90):
        a = _actions(ora.L, 4, s, n)
        _same_outputs("%s loaded engine, step %d" % (game, s), B.step(a), ora.step(a))
    B.close()
    ora.close()


@pytest.mark.gpu
@pytest.mark.parametrize("then", ["step", "masked_reset"])
def test_bossfight_snapshot_carries_a_non_square_camera(then):
    """D15: bossfight's step and reset read the camera size the LAST render left (F_CAMW / F_CAMH, in the blob).  A 200×120
    frame of envs 1 and 3, then save, load into a foreign engine, then a step — or a masked reset of env 3 — there: the
    oracle's observations, rewards, dones and state, the oracle having done the same calls."""
    from engine_util import EngineVec
    n, W, H = 8, 200, 120
    A = EngineVec("bossfight", n, seed_base=9)
    ora = _SingleEnvs("bossfight", n, 9)
    assert np.array_equal(A.reset(), ora.obs())
    for s in range(40):
        a = np.where(np.arange(n) % 2 == 0, 9, _actions(ora.L, 3, s, n)).astype(np.int32)
        _same_outputs("step %d" % s, A.step(a), ora.step(a))
    for env in (1, 3):
        _same_frame("env %d" % env, A.frame(env, W, H), ora.frame(env, W, H))
    snap = A.save_state()
    A.close()
    B = _foreign_engine(Case("bossfight"), n)
    B.load_state(snap)
    if then == "masked_reset":
        mask = np.zeros(n, np.uint8)
        mask[3] = 1
        o = B.reset(mask=mask)
        ora.reset_one(3)
        assert np.array_equal(o, ora.obs()), "observations after the masked reset"
        assert_same_dump(B.state(3), oracle_state(ora.hs[3]), "state env 3 after the masked reset")
    for s in range(40, 60):
        a = np.where(np.arange(n) % 2 == 0, 9, _actions(ora.L, 3, s, n)).astype(np.int32)
        _same_outputs("loaded engine, step %d" % s, B.step(a), ora.step(a))
        if s == 40:
            for env in (1, 3):
                assert_same_dump(B.state(env), oracle_state(ora.hs[env]), "state env %d after the first step" % env)
    assert_same_dump(B.state(3), oracle_state(ora.hs[3]), "state env 3")
    B.close()
    ora.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
_BASE = dict(game="coinrun", n=48, env_offset=0, mode=2, game_flags=0, num_levels=5, start_level=10)
_OTHERS = [("game", "maze"), ("n", 47), ("env_offset", 64), ("mode", 1), ("game_flags", 1), ("num_levels", 6),
           ("start_level", 11), ("magic", None), ("one_byte_short", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("field,value", _OTHERS, ids=[f for f, _ in _OTHERS])
def test_a_refused_snapshot_leaves_the_engine_untouched(field, value):
    """An engine that differs from the snapshot's in exactly one header field — or is offered a snapshot with a broken
    magic, or one a byte short — refuses it, and then goes on exactly as a twin that was never offered anything."""
    from engine_util import EngineVec

    def make(cfg, seed_base):
        cfg = dict(cfg)
        return EngineVec(cfg.pop("game"), cfg.pop("n"), seed_base=seed_base, **cfg)

    src = make(_BASE, 5)
    src.reset()
    for _ in range(25):
        src.step_quiet(run_seed=2)
    snap = src.save_state()
    src.close()
    cfg = dict(_BASE)
    if field == "magic":
        snap[0] ^= 0xFF
    elif field == "one_byte_short":
        snap = snap[:-1].copy()
    else:
        assert cfg[field] != value
        cfg[field] = value
    eng, twin = make(cfg, 8), make(cfg, 8)
    for v in (eng, twin):
        v.reset()
        for _ in range(10):
            v.step_quiet(run_seed=6)
    with pytest.raises(pglib.EngineError):
        eng.load_state(snap)
    _same_outputs("right after the refusal", eng._fetch(), twin._fetch())
    for s in range(20):
        _same_outputs("step %d after the refusal" % s, eng.step(None, run_seed=6), twin.step(None, run_seed=6))
    for e in range(0, eng.n, 12):
        assert_same_dump(eng.state(e), twin.state(e), "state env %d" % e)
    eng.close()
    twin.close()


@pytest.mark.gpu
def test_saving_into_a_short_buffer_fails_and_writes_nothing():
    from engine_util import EngineVec
    eng = EngineVec("chaser", 70, seed_base=3)
    eng.reset()
    size = eng.L.pgv_snapshot_bytes(eng.h)
    buf = np.full(size, 0xA5, np.uint8)
    assert eng.L.pgv_save_state(eng.h, buf.ctypes.data_as(c_void_p), size - 1) != 0
    assert b"too small" in eng.L.pgv_last_error()
    assert (buf == 0xA5).all()
    assert eng.save_state().size == size
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the torch path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vec_env_load_state_writes_through_the_bound_outputs():
    """ProcgenVecEnv.save_state / load_state with outputs bound into a shared slab (out=): pgv_load_state writes the
    snapshot's observations, rewards and dones through the bound pointers.  Two games side by side in one slab with
    sentinel blocks between and behind them; their snapshots loaded into fresh envs bound to a NEW slab land in those
    envs' blocks and nowhere else, and the 60 steps that followed the save replay byte for byte."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    games, per, gap = ("chaser", "coinrun"), 96, 8
    total = len(games) * (per + gap)
    SENT_U8, SENT_F32 = 0xA5, -12345.0

    def slab_and_envs(seed_base):
        slab = (torch.full((total, 64, 64, 3), SENT_U8, dtype=torch.uint8, device="cuda"),
                torch.full((total,), SENT_F32, dtype=torch.float32, device="cuda"),
                torch.full((total,), SENT_U8, dtype=torch.uint8, device="cuda"))
        envs = [ProcgenVecEnv(g, per, seed_base=seed_base, out=tuple(t[k * (per + gap):k * (per + gap) + per] for t in slab))
                for k, g in enumerate(games)]
        return slab, envs

    def host(slab):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().copy() for t in slab)

    def step_all(envs):
        for e in envs:
            e.step_synthetic(RUN_SEED, ordered=False)
        for e in envs:
            e.sync()

    def sentinels_intact(arrays, tag):
        for k in range(len(games)):
            lo = k * (per + gap) + per
            assert (arrays[0][lo:lo + gap] == SENT_U8).all(), "%s: obs sentinel block %d" % (tag, k)
            assert (arrays[1][lo:lo + gap] == np.float32(SENT_F32)).all(), "%s: reward sentinel block %d" % (tag, k)
            assert (arrays[2][lo:lo + gap] == SENT_U8).all(), "%s: done sentinel block %d" % (tag, k)

    slab, envs = slab_and_envs(SEED_BASE)
    for e in envs:
        e.reset()
    for _ in range(80):
        step_all(envs)
    snaps = [e.save_state() for e in envs]
    at_save = host(slab)
    sentinels_intact(at_save, "first slab at the save")
    tail = []
    for _ in range(60):
        step_all(envs)
        tail.append(host(slab))
    sentinels_intact(tail[-1], "first slab at the end")
    assert sum(int(t[2][:per].sum()) + int(t[2][per + gap:2 * per + gap].sum()) for t in tail) > 0, "no episode ended in the tail"
    for e in envs:
        e.close()

    slab2, envs2 = slab_and_envs(FOREIGN_SEED)
    for e, snap in zip(envs2, snaps):
        e.load_state(snap)
        e.sync()
    loaded = host(slab2)
    sentinels_intact(loaded, "new slab after the load")
    for got, want, what in zip(loaded, at_save, ("obs", "reward", "done")):
        assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                              want.view(np.uint32) if want.dtype == np.float32 else want), "%s after the load" % what
    for s, want in enumerate(tail):
        step_all(envs2)
        got = host(slab2)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), s
        assert np.array_equal(got[0], want[0]), "obs, step %d after the load" % s
    for e in envs2:
        e.close()
