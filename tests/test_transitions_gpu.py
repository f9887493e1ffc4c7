"""Transitions (include/procgen2_vec.h pgv_transitions_enable), the GPU half: the HIP engine against the model of
tests/transitions_util.py — the oracle's rewards and dones and EpisodeModel's terminated / truncated in a numpy record ring,
the n-step walk and the GAE recurrence in np.float32 — bit for bit after every call, floats by bit pattern: the three [T, N]
arrays whole, the gathered scalars over every held push and some that are not, the gathered rows against HistoryRing.gather,
advantages and returns.

N = 131 envs (two wavefronts and a ragged tail), also 65 and 1; T = 5 slots and 40 calls, so the ring wraps eight times; n = 6
exceeds T - 1, so every such window is cut short by what the ring holds.  tests/test_transitions.py counts, on the oracle,
what the runs reach.
"""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from episodes_util import SAME_STEP, synthetic_actions
from history_util import CALLS, N, RUN_SEED, T, HistoryEpisodes, HistoryRing
from oracle_util import OBS_BYTES
from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import ProcgenVecEnv, TransitionTensors
from transitions_util import (CUT, GAE_L, GAE_PARAMS, GAE_T, GATHER_PARAMS, RECORDED, TERMINATED, TRUNCATED, VOID, TransitionModel,
                              TransitionsEpisodes, TransitionsSequence, TransitionsVec, entries)

pytestmark = pytest.mark.gpu

SCALARS = ("action", "nstep_return", "discount", "steps", "status")
FRAME_PARAMS = [(1, "uint8"), (4, "float16"), (4, "uint8"), (1, "float16")]


def bits(t):
    """A torch tensor's bit patterns as numpy, on the host."""
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def frames_of(v):
    return v.obs.cpu().numpy().reshape(v.num_envs, OBS_BYTES)


def make(game, n, gray=False, capacity=T, **more):
    return ProcgenVecEnv(game, n, seed_base=1, history=dict(capacity=capacity, gray=gray), transitions=True, **more)


def check_rings(v, ring, tr, obs, what):
    """What a call leaves: the slab, head, the began bytes and the frames of the history; the three record arrays whole."""
    h, r = v.history, v.transitions
    assert np.array_equal(frames_of(v), obs), ("obs", what)
    assert h.head == ring.head and np.array_equal(h.began.cpu().numpy(), ring.began), ("began", what)
    assert np.array_equal(h.frames.cpu().numpy(), ring.frames), ("frames", what)
    assert np.array_equal(r.flags.cpu().numpy(), tr.flags), ("flags", what)
    assert np.array_equal(r.action.cpu().numpy(), tr.action), ("action", what)
    assert np.array_equal(bits(r.reward), raw(tr.reward)), ("reward", what)


def check_scalars(v, tr, p, i, what):
    for n, gamma in GATHER_PARAMS:
        got = v.transition_gather(p, i, n=n, gamma=gamma, frames=False)
        want = tr.walk(p, i, n, gamma)
        assert got.obs is None and got.next_obs is None
        for k in SCALARS:
            assert np.array_equal(bits(getattr(got, k)), raw(want[k])), (k, n, gamma, what)


def check_frames(v, tr, p, i, n, gamma, K, dtype, what):
    got = v.transition_gather(p, i, n=n, gamma=gamma, stack=K, dtype=dtype)
    want = tr.gather(p, i, n, gamma, K, dtype)
    assert got.obs.dtype == getattr(torch, dtype) and tuple(got.obs.shape) == want["obs"].shape == tuple(got.next_obs.shape)
    assert np.array_equal(bits(got.obs), want["obs"]), ("obs", n, gamma, K, dtype, what)
    assert np.array_equal(bits(got.next_obs), want["next_obs"]), ("next_obs", n, gamma, K, dtype, what)
    for k in SCALARS:
        assert np.array_equal(bits(getattr(got, k)), raw(want[k])), (k, n, gamma, K, dtype, what)


def check_call(v, model, t, last):
    """After call t: the rings; the scalars of every (n, gamma) over every held push, head - T - 1, head - 1, head, -1 and
    every env, -1 and N; the rows over a few envs of both wavefronts with a duplicate entry, and over all of it every eighth
    call, (K, dtype) and (n, gamma) taking turns."""
    ring, tr, n_envs = model.ring, model.tr, v.num_envs
    check_rings(v, ring, tr, model.obs, t)
    p, i = entries(ring.head, ring.T, n_envs)
    check_scalars(v, tr, p, i, t)
    K, dtype = FRAME_PARAMS[t % 4]
    n, gamma = GATHER_PARAMS[t % 6]
    few = np.isin(i, [0, 1, 63, 64, n_envs - 1, -1, n_envs])
    pf, jf = np.concatenate([p[few], p[few][:3]]), np.concatenate([i[few], i[few][:3]])  # (the same entry twice in one call)
    check_frames(v, tr, pf, jf, n, gamma, K, dtype, t)
    if t % 8 == 7 or last:
        check_frames(v, tr, p, i, n, gamma, K, dtype, (t, "all"))


RUNS = [("maze", SAME_STEP, 7, N, False), ("bossfight", "next_step", 0, N, True), ("chaser", SAME_STEP, 7, N, False),
        ("maze", SAME_STEP, 7, 65, True), ("bossfight", "next_step", 0, 1, False)]


@pytest.mark.parametrize("game,mode,limit,n,gray", RUNS)
def test_episode_runs_match_the_model(game, mode, limit, n, gray):
    """step_episodes: reward, TERMINATED and TRUNCATED from the episode outputs — the terminal step's values, which the same-step
    reset has wiped from the engine's own rows — and VOID in next-step mode."""
    v = make(game, n, gray, autoreset_mode=mode, max_episode_steps=limit)
    model = TransitionsEpisodes(game, n, mode, T, gray, max_episode_steps=limit)
    r = v.transitions
    assert tuple(r.action.shape) == tuple(r.reward.shape) == tuple(r.flags.shape) == (T, n) and not bool(r.flags.any())
    assert r.action.dtype == torch.int32 and r.reward.dtype == torch.float32 and r.flags.dtype == torch.uint8
    assert v.L.pgv_transitions_flags(v._h) == r.flags.data_ptr()
    v.reset(), model.first_reset()
    check_rings(v, model.ring, model.tr, model.obs, "reset")
    seen = 0
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step_episodes(torch.as_tensor(a)), model.step(a)
        check_call(v, model, t, t == CALLS - 1)
        seen |= int(np.bitwise_or.reduce(model.tr.flags[(model.ring.head - 2) % T]))
    if n == N:  # (chaser's run is there for its rewards: 0.04 a pellet; nobody dies within seven steps)
        assert (seen & TERMINATED or game == "chaser") and seen & (TRUNCATED if limit else VOID), seen
    v.close(), model.close()


@pytest.mark.parametrize("game", ["bossfight", "maze"])
def test_plain_and_synthetic_steps(game):
    """pgv_step and pgv_step_synthetic taking turns, on rows 1000 .. of a larger engine: the action as given, the device-made
    action equal to pgo_synthetic_action of (run seed, step index, env_offset + i), TERMINATED from the done row, VOID on the
    step behind it, never TRUNCATED."""
    off = 1000
    v = make(game, N, True, env_offset=off)
    model = TransitionsVec(game, N, T, True, env_offset=off)
    v.reset(), model.first_reset()
    void = 0
    for t in range(CALLS):
        if t % 2:
            a = synthetic_actions(RUN_SEED, t, N, off)  # (what the engine makes for its step t)
            v.step_synthetic(RUN_SEED)
        else:
            a = synthetic_actions(RUN_SEED + 1, t, N, off)
            v.step(torch.as_tensor(a))
        model.step(a)
        check_call(v, model, t, t == CALLS - 1)
        slot = (model.ring.head - 2) % T
        assert np.array_equal(v.transitions.action[slot].cpu().numpy(), a)
        void += int(((model.tr.flags[slot] & VOID) != 0).sum())
    assert not (model.tr.flags & TRUNCATED).any() and (void >= 10 or game == "maze"), void
    v.close(), model.close()


def test_sequences_and_pushes_by_hand_are_not_recorded():
    """A drawn sequence and a push by hand open slots whose rows are flags = 0, so a window stops in front of them and a stale
    row of push q - T is never taken for row q; a sequence without frames leaves no VOID behind for the next step."""
    v, model = make("bossfight", N, True), TransitionsSequence("bossfight", N, T, True)
    v.reset(), model.first_reset()
    check_rings(v, model.ring, model.tr, model.obs, "reset")
    t = unrecorded = void = 0
    for call in range(18):
        kind = call % 6
        if kind in (0, 1, 3, 5):
            a = synthetic_actions(RUN_SEED, t, N)
            v.step(torch.as_tensor(a)), model.step(a)
            t += 1
            void += int(((model.tr.flags[(model.ring.head - 2) % T] & VOID) != 0).sum())
        else:
            length = 3 if kind == 2 else 5
            a = np.stack([synthetic_actions(RUN_SEED, t + k, N) for k in range(length)])
            t += length
            if kind == 2:
                v.step_sequence(torch.as_tensor(a), frames="last")
                model.sequence(a, frames_last=True)
            else:
                v.step_sequence(torch.as_tensor(a), frames="none")
                assert v.history.head == model.ring.head  # (no slot, no row)
                v.render_obs()
                v.history_push()
                model.sequence(a, frames_last=False, draw=True)
                model.push()
            unrecorded += 1
            assert not model.tr.flags[(model.ring.head - 2) % T].any()
        check_call(v, model, call, call == 17)
    assert unrecorded == 6 and void >= 3, void
    v.close(), model.close()


def test_resets_and_loads_cut_rows():
    """A masked pgv_reset mid-run and a fork write no row: the began byte they leave on the next frame is how they show, and
    the rows in front of it are CUT exactly where the model has them.  The model is fed the engine's own rows here (what a
    load leaves in obs, reward and done is tests/test_env_records_gpu.py's subject)."""
    n = 96
    v, ring = make("maze", n, True), HistoryRing(n, T, True)
    tr = TransitionModel(ring)

    class Fed:
        pass
    model = Fed()
    model.ring, model.tr = ring, tr
    v.reset()
    ring.reset(frames_of(v))
    cut = 0
    for t in range(30):
        found = v.done.cpu().numpy().copy()
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a))
        ring.flag(found)
        ring.push(frames_of(v))
        tr.record(a, v.reward.cpu().numpy(), v.done.cpu().numpy(), 0, found)
        if t in (9, 22):
            mask = ((np.arange(n) + t) % 4 == 0).astype(np.uint8)
            v.reset(mask=mask)
            ring.reset(frames_of(v), mask)
        if t == 14:
            v.fork([5, 5], [40, 77])
            where = np.zeros(n, np.uint8)
            where[[40, 77]] = 1
            ring.flag(where)
        model.obs = frames_of(v)
        check_call(v, model, t, t == 29)
        if t in (10, 15, 23):
            w = tr.walk(*entries(ring.head, T, n), 3, 0.99)
            cut += int(((w["status"] & CUT) != 0).sum())
            if t == 15:
                newest = tr.walk(np.full(2, ring.head - 2, np.int64), np.array([40, 77]), 3, 0.99)  # the step behind the fork
                ended = (tr.flags[(ring.head - 2) % T][[40, 77]] & (TERMINATED | VOID)) != 0
                assert (((newest["status"] & CUT) != 0) | ended).all() and (newest["steps"][~ended] == 1).all()
    assert cut >= 40, cut
    v.close()


@pytest.mark.parametrize("game,mode,limit", [("maze", SAME_STEP, 7), ("bossfight", "next_step", 0)])
def test_gae_over_a_stretch(game, mode, limit):
    """A ring of 17 slots, a stretch of 16 rows, values from a seeded draw: (0.99, 0.95) and (1, 1), with and without
    trunc_values, half way through the run (the ring not yet wrapped twice) and at its end."""
    v = make(game, N, True, capacity=GAE_T, autoreset_mode=mode, max_episode_steps=limit)
    model = TransitionsEpisodes(game, N, mode, GAE_T, True, max_episode_steps=limit)
    v.reset(), model.first_reset()
    rng = np.random.default_rng(11)
    V = rng.standard_normal((GAE_L + 1, N)).astype(np.float32)
    tv = rng.standard_normal((GAE_L, N)).astype(np.float32)
    dV, dtv = torch.as_tensor(V, device="cuda"), torch.as_tensor(tv, device="cuda")
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, N)
        v.step_episodes(torch.as_tensor(a)), model.step(a)
        if t not in (19, CALLS - 1):
            continue
        check_rings(v, model.ring, model.tr, model.obs, t)
        first = model.ring.head - 1 - GAE_L
        for gamma, lam in GAE_PARAMS:
            for trunc, dtrunc in ((None, None), (tv, dtv)):
                adv, ret = v.transition_gae(first, GAE_L, dV, gamma=gamma, lam=lam, trunc_values=dtrunc)
                want_adv, want_ret = model.tr.gae(first, GAE_L, V, gamma, lam, trunc)
                assert np.array_equal(bits(adv), raw(want_adv)), ("advantages", gamma, lam, trunc is None, t)
                assert np.array_equal(bits(ret), raw(want_ret)), ("returns", gamma, lam, trunc is None, t)
        # a shorter stretch somewhere inside, without the optional arrays
        g = pglib.gae(0.99, 0.95, dV.data_ptr(), None)
        adv = torch.full((3, N), 7.0, device="cuda")
        g.advantages = adv.data_ptr()
        v._before()
        pglib.check(v.L, v.L.pgv_transitions_gae(v._h, first + 5, 3, ctypes.byref(g)), "pgv_transitions_gae")
        v._after()
        want_adv, _ = model.tr.gae(first + 5, 3, V[:4], 0.99, 0.95)
        assert np.array_equal(bits(adv), raw(want_adv))
    v.close(), model.close()


def test_the_refusals():
    """Each refusal leaves a message and the engine as it was: it goes on equal to a twin that never saw any of it."""
    n = 70
    plain = ProcgenVecEnv("maze", n, seed_base=1)
    L = plain.L

    def refused(rc, who, word):
        assert rc != 0, "not refused"
        msg = L.pgv_last_error().decode()
        assert who in msg and word in msg, msg

    def enable(h, size=None, cfg=True, reserved=0):
        c = pglib.TransitionsConfig(ctypes.sizeof(pglib.TransitionsConfig) if size is None else size, reserved)
        return L.pgv_transitions_enable(h, ctypes.byref(c) if cfg else None)

    E = "pgv_transitions_enable"
    refused(enable(plain._h), E, "pgv_history_enable")  # without the history
    assert L.pgv_transitions_flags(plain._h) is None and plain.transitions is None
    plain.close()
    one = ProcgenVecEnv("maze", n, seed_base=1, history=dict(capacity=1))
    refused(enable(one._h), E, "capacity")  # T = 1
    assert L.pgv_transitions_action(one._h) is None
    one.close()
    for bad in (dict(transitions=True), dict(transitions=True, history=dict(capacity=1)), dict(transitions="yes", history=dict(capacity=4))):
        with pytest.raises(ValueError):
            ProcgenVecEnv("maze", 4, **bad)

    v, twin = ProcgenVecEnv("maze", n, seed_base=1, history=dict(capacity=T)), make("maze", n)
    h = v._h
    refused(enable(h, size=4), E, "struct_size"), refused(enable(h, cfg=False), E, "struct_size"), refused(enable(h, reserved=1), E, "reserved")
    assert L.pgv_transitions_flags(h) is None
    with pytest.raises(pglib.EngineError):
        v.transition_gather([0], [0])
    with pytest.raises(pglib.EngineError):
        v.transition_gae(0, 1, torch.zeros((2, n)))
    v._before()
    assert enable(h) == 0
    refused(enable(h), E, "already")  # twice
    v._after()
    v.transitions = TransitionTensors(v)
    v.reset(), twin.reset()
    for t in range(8):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, n))
        v.step(a), twin.step(a)

    def same(what):
        assert bool((v.obs == twin.obs).all()) and bool((v.reward == twin.reward).all()) and bool((v.done == twin.done).all()), what
        assert v.history.head == twin.history.head and bool((v.history.frames == twin.history.frames).all()), what
        assert bool((v.history.began == twin.history.began).all()) and bool((v.history.pending == twin.history.pending).all()), what
        for k in ("action", "flags"):
            assert bool((getattr(v.transitions, k) == getattr(twin.transitions, k)).all()), (k, what)
        assert np.array_equal(bits(v.transitions.reward), bits(twin.transitions.reward)), what

    same("before")
    head = v.history.head
    B = 4
    p = torch.full((B,), head - 2, dtype=torch.int64, device="cuda")
    i = torch.arange(B, dtype=torch.int32, device="cuda")
    rows = torch.full((B * 4 * 3 * 4096 * 2 + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    words = torch.full((B + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    P, I = c_void_p(p.data_ptr()), c_void_p(i.data_ptr())
    torch.cuda.synchronize()
    G = "pgv_transitions_gather"

    def gather(count=B, pushes=P, envs=I, size=None, query=True, **fields):
        q = pglib.transition_query(**{**dict(n=3, gamma=0.99, stack=4, dtype="float16", obs=rows.data_ptr(), action=words.data_ptr()), **fields})
        if size is not None:
            q.struct_size = size
        return L.pgv_transitions_gather(h, pushes, envs, count, ctypes.byref(q) if query else None)

    refused(gather(n=0), G, "n must"), refused(gather(n=65), G, "n must"), refused(gather(n=-1), G, "n must")
    refused(gather(stack=0), G, "stack"), refused(gather(stack=9), G, "stack"), refused(gather(dtype=4), G, "dtype")
    refused(gather(count=-1), G, "count"), refused(gather(size=8), G, "struct_size"), refused(gather(query=False), G, "struct_size")
    refused(gather(obs=rows.data_ptr() + 8), G, "aligned"), refused(gather(next_obs=rows.data_ptr() + 4), G, "aligned")
    refused(gather(action=words.data_ptr() + 2), G, "aligned"), refused(gather(nstep_return=words.data_ptr() + 1), G, "aligned")
    refused(gather(discount=words.data_ptr() + 3), G, "aligned"), refused(gather(steps=words.data_ptr() + 2), G, "aligned")
    refused(gather(pushes=None), G, "NULL"), refused(gather(envs=None), G, "NULL")
    assert gather(count=0, pushes=None, envs=None) == 0  # nothing to do
    # a stretch that is not complete; misaligned arrays
    A = "pgv_transitions_gae"
    vals = torch.zeros((T + 2) * n + 2, dtype=torch.float32, device="cuda")
    out = torch.full(((T + 1) * n + 2,), 3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def gae(first, length, size=None, **fields):
        g = pglib.gae(**{**dict(gamma=0.99, lam=0.95, values=vals.data_ptr(), advantages=out.data_ptr()), **fields})
        if size is not None:
            g.struct_size = size
        return L.pgv_transitions_gae(h, first, length, ctypes.byref(g))

    oldest = head - T
    refused(gae(oldest, T), A, "held")            # the last row's successor is not pushed yet
    refused(gae(oldest - 1, 2), A, "held")        # the first row is no longer held
    refused(gae(head - 1, 1), A, "held"), refused(gae(head, 1), A, "held"), refused(gae(-1, 1), A, "held"), refused(gae(2**62, 1), A, "held")
    refused(gae(oldest, 2**31 - 1), A, "held")
    refused(gae(oldest, 0), A, "length"), refused(gae(oldest, -1), A, "length"), refused(gae(oldest, 1, size=8), A, "struct_size")
    refused(gae(oldest, 1, values=None), A, "NULL"), refused(gae(oldest, 1, advantages=None), A, "NULL")
    refused(gae(oldest, 1, values=vals.data_ptr() + 2), A, "aligned"), refused(gae(oldest, 1, advantages=out.data_ptr() + 1), A, "aligned")
    refused(gae(oldest, 1, returns=out.data_ptr() + 2), A, "aligned"), refused(gae(oldest, 1, trunc_values=vals.data_ptr() + 3), A, "aligned")
    torch.cuda.synchronize()
    assert bool((rows == 0x5A).all()) and bool((words == 0x5A5A5A5A).all()) and bool((out == 3.0).all())
    assert gae(oldest, T - 1) == 0  # the longest stretch the ring holds
    torch.cuda.synchronize()
    assert bool((out[(T - 1) * n:] == 3.0).all())
    same("after the refusals")
    # a misaligned obs slab: the step is refused before anything is enqueued — no row, no pending byte, no push
    odd = torch.zeros(n * OBS_BYTES + 16, dtype=torch.uint8, device="cuda")
    acts = torch.as_tensor(synthetic_actions(RUN_SEED, 8, n), device="cuda")
    torch.cuda.synchronize()
    pglib.check(L, L.pgv_bind_outputs(h, c_void_p(odd.data_ptr() + 8), None, None), "pgv_bind_outputs")
    assert L.pgv_step(h, c_void_p(acts.data_ptr())) != 0 and L.pgv_step_synthetic(h, RUN_SEED) != 0 and L.pgv_history_push(h) != 0
    pglib.check(L, L.pgv_bind_outputs(h, c_void_p(v.obs.data_ptr()), None, None), "pgv_bind_outputs")
    same("after the misaligned slab")
    for t in range(8, 20):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, n))
        v.step(a), twin.step(a)
        same(t)
    v.close(), twin.close()


def test_an_engine_without_the_feature():
    """Made without transitions=: the same 40 calls give the same obs, reward, done, history frames and began bytes as the model —
    and as a twin with the feature —, every getter is NULL, the calls are refused, and the sizes of snapshots and records
    are what they were."""
    game, mode, limit = "maze", SAME_STEP, 7
    plain = ProcgenVecEnv(game, N, seed_base=1, history=dict(capacity=T), autoreset_mode=mode, max_episode_steps=limit)
    twin = make(game, N, autoreset_mode=mode, max_episode_steps=limit)
    model = HistoryEpisodes(game, N, mode, T, False, max_episode_steps=limit)
    L, h = plain.L, plain._h
    assert plain.transitions is None
    assert L.pgv_transitions_action(h) is None and L.pgv_transitions_reward(h) is None and L.pgv_transitions_flags(h) is None
    q = pglib.transition_query(3, 0.99, 4, "float16")
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.pgv_transitions_gather(h, c_void_p(idx.data_ptr()), c_void_p(idx.data_ptr()), 1, ctypes.byref(q)) != 0
    assert b"pgv_transitions_enable" in L.pgv_last_error()
    plain.reset(), twin.reset(), model.first_reset()
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, N)
        plain.step_episodes(torch.as_tensor(a)), twin.step_episodes(torch.as_tensor(a)), model.step(a)
        assert np.array_equal(frames_of(plain), model.obs) and np.array_equal(frames_of(twin), model.obs), t
        assert np.array_equal(bits(plain.reward), raw(model.m.engine_reward)) and np.array_equal(plain.done.cpu().numpy(), model.m.engine_done), t
        assert np.array_equal(bits(plain.episode.reward), raw(model.m.reward)) and np.array_equal(plain.episode.ended.cpu().numpy(), model.m.ended), t
        assert plain.history.head == model.ring.head and np.array_equal(plain.history.began.cpu().numpy(), model.ring.began), t
        assert np.array_equal(plain.history.frames.cpu().numpy(), model.ring.frames), t
        assert np.array_equal(plain.history.pending.cpu().numpy(), model.ring.pending), t
        assert bool((plain.history.frames == twin.history.frames).all()) and bool((plain.reward == twin.reward).all()), t
    assert L.pgv_snapshot_bytes(plain._h) == L.pgv_snapshot_bytes(twin._h) and plain.env_record_bytes == twin.env_record_bytes
    plain.close(), twin.close(), model.close()
