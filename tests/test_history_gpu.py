"""Frame history (include/procgen2_vec.h pgv_history_enable), the GPU half: the HIP engine against the model of
tests/history_util.py — the oracle's frames in a numpy ring with began bytes and pending flags, and a plain-Python gather —
bit for bit after every call: the obs slab, the whole ring, the began bytes, the pending flags, head, and gathered rows.

n = 131 envs (two wavefronts of envs plus a ragged tail; the push and gather kernels have a workgroup per env / per entry) and
n = 1; T = 5 slots and about 40 calls, so the ring wraps eight times.  tests/test_history.py counts, on the oracle, the stacks
the episode runs cut and carry across the wrap.
"""
import ctypes
import functools
from ctypes import c_float, c_void_p

import numpy as np
import pytest
import torch

from engine_util import _dump
from episodes_util import synthetic_actions
from history_util import CALLS, EPISODE_RUNS, N, RUN_SEED, T, Frames, HistoryEpisodes, HistoryRing, HistorySequence, HistoryVec, cut_and_wrapped
from oracle_util import OBS_BYTES, OracleVec
from policy_obs_util import DTYPES
from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import HistoryTensors, ProcgenVecEnv, _device_view
from sequence_util import GAMES, protocol_calls

pytestmark = pytest.mark.gpu


def bits(t):
    """A torch tensor's bit patterns as numpy, on the host."""
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def frames_of(v):
    return v.obs.cpu().numpy().reshape(v.num_envs, OBS_BYTES)


def make(game, n, gray, capacity=T, **more):
    return ProcgenVecEnv(game, n, seed_base=1, history=dict(capacity=capacity, gray=gray), **more)


def check(v, ring, obs, what):
    """What a call leaves, against the model: the slab, the ring whole, the began bytes whole, the pending flags, head."""
    h = v.history
    assert np.array_equal(frames_of(v), obs), "obs, %s" % (what,)
    assert h.head == ring.head and h.capacity == ring.T, "head, %s" % (what,)
    got = h.frames.cpu().numpy()
    assert got.shape == ring.frames.shape and np.array_equal(got, ring.frames), "frames, %s" % (what,)
    assert np.array_equal(h.began.cpu().numpy(), ring.began), "began, %s" % (what,)
    assert np.array_equal(h.pending.cpu().numpy(), ring.pending), "pending, %s" % (what,)


def check_gather(v, ring, pushes, envs, K, dtype, what):
    got = v.history_gather(torch.as_tensor(pushes, dtype=torch.int64), torch.as_tensor(envs, dtype=torch.int32), stack=K, dtype=dtype)
    want = ring.gather(pushes, envs, K, dtype)
    assert got.dtype == getattr(torch, dtype) and tuple(got.shape) == want.shape and got.is_contiguous(), what
    assert np.array_equal(bits(got), want), "gather K=%d %s, %s" % (K, dtype, what)


def check_newest(v, ring, K, dtype, what):
    n = v.num_envs
    check_gather(v, ring, [ring.head - 1] * n, list(range(n)), K, dtype, what)


def check_every_held_push(v, ring, dtype, what):
    """Every held push of every env, K = 1, 4 and 8 (8 > T: the walk runs off the ring)."""
    n = v.num_envs
    held = range(max(0, ring.head - ring.T), ring.head)
    pushes = [p for p in held for _ in range(n)]
    envs = list(range(n)) * len(held)
    for K in (1, 4, 8):
        check_gather(v, ring, pushes, envs, K, dtype, what)


def state_of(v, env):
    return _dump(lambda buf, m: v.L.pgv_dump_state(v._h, env, buf, m), c_float, np.float32)


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("game", GAMES)
def test_single_steps_match_the_model(game, gray):
    """All seven games: reset and 40 single steps; the ring whole and gather(head - 1) after every call, every held push
    with K = 1, 4, 8 every eighth call and at the end."""
    v, model = make(game, N, gray), HistoryVec(game, N, T, gray)
    h = v.history
    assert tuple(h.frames.shape) == (T, N, 1 if gray else 3, 64, 64) and tuple(h.began.shape) == (T, N) and h.head == 0 and h.capacity == T
    assert bool((h.pending == 1).all()) and not bool(h.frames.any())  # enable pushes nothing
    assert v.L.pgv_history_frames(v._h) == h.frames.data_ptr()
    v.reset(), model.first_reset()
    check(v, model.ring, model.obs, "reset")
    check_newest(v, model.ring, 4, "float16", "reset")
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, N)
        v.step(torch.as_tensor(a)), model.step(a)
        check(v, model.ring, model.obs, (game, t))
        check_newest(v, model.ring, 4, "float16", (game, t))
        if t % 8 == 7 or t == CALLS - 1:
            check_every_held_push(v, model.ring, "uint8", (game, t))
    assert model.ring.head == CALLS + 1
    v.close(), model.close()


@functools.lru_cache(maxsize=None)
def maze_reference(n=N, steps=CALLS):
    """One oracle run of maze shared by the dtype tests: the reset frame, then per step (frame, the done row the step found)."""
    o = OracleVec("maze", n)
    rows = [(o.reset_obs().copy(), np.zeros(n, np.uint8))]
    for t in range(steps):
        found = o.done.copy()
        o.step(synthetic_actions(RUN_SEED, t, n))
        rows.append((o.obs.copy(), found))
    o.close()
    for obs, found in rows:
        obs.setflags(write=False), found.setflags(write=False)
    return rows


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_every_dtype_on_maze(dtype, gray):
    rows = maze_reference()
    v, ring = make("maze", N, gray), HistoryRing(N, T, gray)
    v.reset()
    ring.reset(rows[0][0])
    check(v, ring, rows[0][0], "reset")
    for t in range(CALLS):
        obs, found = rows[t + 1]
        v.step(torch.as_tensor(synthetic_actions(RUN_SEED, t, N)))
        ring.flag(found)
        ring.push(obs)
        check(v, ring, obs, t)
        check_newest(v, ring, 4, dtype, t)
        if t in (3, 21, CALLS - 1):  # (3: fewer pushes than slots)
            check_every_held_push(v, ring, dtype, t)
    assert ring.began.sum() >= 1
    if dtype != "uint8":  # the values a network sees: 0 .. 1
        got = v.history_gather([ring.head - 1] * N, list(range(N)), stack=2, dtype=dtype).float()
        assert float(got.max()) <= 1.0 and float(got.min()) >= 0.0
    v.close()


def test_a_single_env():
    v, model = make("maze", 1, True), HistoryVec("maze", 1, T, True)
    v.reset(), model.first_reset()
    check(v, model.ring, model.obs, "reset")
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, 1)
        v.step(torch.as_tensor(a)), model.step(a)
        check(v, model.ring, model.obs, t)
        check_every_held_push(v, model.ring, "float32", t)
    v.close(), model.close()


def test_indices_that_give_zero_rows():
    """p = head, p = head - T - 1, head - T (the oldest held), negative p, env = -1, env = N, huge values, a duplicate entry;
    count = 0; an `out` of the caller's with guards on both sides."""
    v, model = make("maze", N, False), HistoryVec("maze", N, T, False)
    v.reset(), model.first_reset()
    for t in range(12):
        a = synthetic_actions(RUN_SEED, t, N)
        v.step(torch.as_tensor(a)), model.step(a)
    head = model.ring.head
    pushes = [head, head - T - 1, head - T, -1, -2**40, 2**40, head - 1, head - 1, head - 1, head - 2, head - 1, head - 1]
    envs = [0, 0, 5, 0, 0, 0, -1, N, 2**31 - 1, -2**31, 7, 7]
    want = model.ring.gather(pushes, envs, 4, "float16")
    zero = [0, 1, 3, 4, 5, 6, 7, 8, 9]
    assert not want[zero].any() and want[2].any() and want[10].any() and np.array_equal(want[10], want[11])
    for K, dtype in ((4, "float16"), (8, "float32"), (1, "uint8")):
        check_gather(v, model.ring, pushes, envs, K, dtype, "odd indices")
    # the caller's rows, with guards
    B, K, guard = len(pushes), 4, 4096
    body = B * K * 3 * 4096 * 2
    slab = torch.full((guard + body + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = slab[guard:guard + body].view(torch.float16).view(B, K * 3, 64, 64)
    got = v.history_gather(pushes, envs, stack=K, dtype="float16", out=out)
    assert got is out and np.array_equal(bits(out), want)
    assert bool((slab[:guard] == 0xA5).all()) and bool((slab[guard + body:] == 0xA5).all())
    # nothing to do
    empty = v.history_gather([], [], stack=4, dtype="float16")
    assert tuple(empty.shape) == (0, 12, 64, 64)
    assert v.L.pgv_history_gather(v._h, None, None, 0, 4, 1, None) == 0
    check(v, model.ring, model.obs, "after the gathers")
    v.close(), model.close()


def enable_raw(v, capacity, gray, frames=None):
    """pgv_history_enable on an env made without the feature; `frames`: a tensor of the caller's, or None for the engine's own."""
    v._before()
    pglib.history_enable(v.L, v._h, capacity, gray, None if frames is None else c_void_p(frames.data_ptr()))
    v._after()
    v.history = HistoryTensors(v, frames, gray)


def test_a_callers_ring_and_its_guards():
    """`frames` carved from a larger tensor with 4 096 guard bytes of a pattern on each side: untouched after the run."""
    n, guard = 67, 4096
    body = T * n * 3 * 4096
    slab = torch.full((guard + body + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    slab[guard:guard + body] = 0
    frames = slab[guard:guard + body].view(T, n, 3, 64, 64)
    v, model = ProcgenVecEnv("maze", n, seed_base=1), HistoryVec("maze", n, T, False)
    enable_raw(v, T, False, frames)
    assert v.L.pgv_history_frames(v._h) == frames.data_ptr()
    v.reset(), model.first_reset()
    for t in range(23):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a)), model.step(a)
    check(v, model.ring, model.obs, "the end")
    check_every_held_push(v, model.ring, "bfloat16", "the end")
    assert bool((slab[:guard] == 0xA5).all()) and bool((slab[guard + body:] == 0xA5).all())
    v.close(), model.close()


def test_reset_under_a_mask_at_head_zero_and_mid_rollout():
    """pgv_reset opens no slot — except slot 0 at head == 0 — and rewrites the named envs' rows of the newest one with
    began = 1; the others keep every byte and their flags.  (The feature is enabled behind the engine's first full reset, so
    that the slab holds a frame of every env when the masked reset finds head == 0.)"""
    v, model = ProcgenVecEnv("maze", N, seed_base=1), HistoryVec("maze", N, T, False, ring=False)
    v.reset(), model.first_reset()
    enable_raw(v, T, False)
    model.f.enable_ring()
    first = (np.arange(N) % 3 != 0).astype(np.uint8)
    v.reset(mask=first), model.reset(first)
    assert model.ring.head == 1 and not model.ring.frames[0][first == 0].any() and np.array_equal(model.ring.pending, 1 - first)
    check(v, model.ring, model.obs, "reset at head 0")
    check_newest(v, model.ring, 4, "float16", "reset at head 0")
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, N)
        v.step(torch.as_tensor(a)), model.step(a)
        check(v, model.ring, model.obs, t)
        if t in (9, 22, 23):
            mask = ((np.arange(N) + t) % 4 == 0).astype(np.uint8)
            before = v.history.frames.cpu().numpy().copy()
            head = v.history.head
            v.reset(mask=mask), model.reset(mask)
            assert v.history.head == head
            check(v, model.ring, model.obs, ("masked reset", t))
            after = v.history.frames.cpu().numpy()
            slot = (head - 1) % T
            assert np.array_equal(after[slot][mask == 0], before[slot][mask == 0])
            assert all(np.array_equal(after[s], before[s]) for s in range(T) if s != slot)
            assert bool((v.history.began[slot].cpu().numpy()[mask != 0] == 1).all())
            check_every_held_push(v, model.ring, "float16", ("masked reset", t))
        if t == 30:
            v.reset(), model.reset(None)
            check(v, model.ring, model.obs, "full reset")
            check_newest(v, model.ring, 8, "uint8", "full reset")
    v.close(), model.close()


@pytest.mark.parametrize("game,mode,limit", EPISODE_RUNS)
def test_episodes_on_the_device(game, mode, limit):
    """step_episodes held to EpisodeModel plus the ring: same-step with a 3-step limit puts began bytes all over the ring;
    next-step.  At least one gathered stack was cut by a began byte and at least one crossed the slot wrap."""
    v = make(game, N, False, autoreset_mode=mode, max_episode_steps=limit)
    model = HistoryEpisodes(game, N, mode, T, False, max_episode_steps=limit)
    v.reset(), model.first_reset()
    cut = wrapped = 0
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, N)
        v.step_episodes(torch.as_tensor(a)), model.step(a)
        check(v, model.ring, model.obs, (mode, t))
        assert np.array_equal(v.episode.ended.cpu().numpy(), model.m.ended)
        check_newest(v, model.ring, 4, "uint8", (mode, t))
        if t % 6 == 5 or t == CALLS - 1:
            check_every_held_push(v, model.ring, "float16", (mode, t))
            c, w = cut_and_wrapped(model.ring, 4)
            cut, wrapped = cut + c, wrapped + w
    assert cut >= 1 and wrapped >= 1, (cut, wrapped)
    v.close(), model.close()


@pytest.mark.parametrize("game", ["maze", "bossfight"])
def test_sequences_push_once(game):
    """Calls of 1, 2, 3, 5, 8, 13 sub-steps with frames="last" against the model; a twin under frames="none" → render_obs() →
    history_push() ends with the same slab, ring and flags; after the frames="none" call alone the flags are the model's
    and nothing was pushed."""
    v, twin, model = make(game, N, True), make(game, N, True), HistorySequence(game, N, T, True)
    v.reset(), twin.reset(), model.first_reset()
    check(v, model.ring, model.obs, "reset")
    inside = 0
    for k, (t, actions) in enumerate(protocol_calls(N, lengths=(1, 2, 3, 5, 8, 13) * 2, run_seed=RUN_SEED)):
        a = torch.as_tensor(actions)
        before_flags, before_done = model.ring.pending.copy(), model.m.engine_done.copy()
        v.step_sequence(a, frames="last")
        model.sequence(actions, frames_last=True)
        check(v, model.ring, model.obs, ("last", t))
        check_newest(v, model.ring, 4, "float16", ("last", t))
        inside += int((model.m.dones[:-1] != 0).any(axis=0).sum())
        kept, head = twin.history.frames.clone(), twin.history.head
        twin.step_sequence(a, frames="none")
        found = (np.vstack([before_done[None], model.m.dones[:-1]]) != 0).any(axis=0)
        assert np.array_equal(twin.history.pending.cpu().numpy(), before_flags | found), ("flags after none", t)
        twin.render_obs()
        assert twin.history.head == head and bool((twin.history.frames == kept).all()), ("none or render_obs pushed", t)
        assert twin.history_push() == head
        check(twin, model.ring, model.obs, ("none, render, push", t))
    check_every_held_push(v, model.ring, "float16", "the end")
    assert inside >= 3, inside
    v.close(), twin.close(), model.close()


def test_loads_flag_the_slots_they_wrote():
    """fork into two slots mid-rollout: the loaded slots begin afresh at their next push and the others move on; load_state
    flags all; an index outside the batch and a zero-filled record change nothing.  The ring model is fed the engine's own
    rows (what a load leaves in obs and done is tests/test_env_records_gpu.py's subject)."""
    n = 96
    v, ring = make("maze", n, True), HistoryRing(n, T, True)
    v.reset()
    ring.reset(frames_of(v))

    def step(t):
        ring.flag(v.done.cpu().numpy())
        v.step(torch.as_tensor(synthetic_actions(RUN_SEED, t, n)))
        ring.push(frames_of(v))
        check(v, ring, frames_of(v), t)
        check_newest(v, ring, 4, "float16", t)

    for t in range(12):
        step(t)
    kept, head = v.history.frames.clone(), v.history.head
    v.fork([5, 5], [40, 77])
    where = np.zeros(n, np.uint8)
    where[[40, 77]] = 1
    ring.flag(where)
    assert np.array_equal(v.history.pending.cpu().numpy(), ring.pending) and ring.pending.sum() >= 2
    assert v.history.head == head and bool((v.history.frames == kept).all())  # a load pushes nothing
    step(12)
    assert ring.began[(ring.head - 1) % T][[40, 77]].tolist() == [1, 1]
    for t in range(13, 20):
        step(t)
    records = v.save_envs([3, 4])
    flags = v.history.pending.clone()
    v.load_envs(records, [n + 7, -1])
    empty = records.clone()
    empty.data.zero_()
    v.load_envs(empty, [10, 11])
    assert bool((v.history.pending == flags).all())
    step(20)
    snap = v.save_state()
    step(21)
    v.load_state(snap)
    ring.flag(None)
    assert bool((v.history.pending == 1).all()) and v.history.head == ring.head
    step(22)
    assert bool(ring.began[(ring.head - 1) % T].all())
    step(23)
    check_every_held_push(v, ring, "uint8", "the end")
    v.close()


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_the_law_against_the_policy_observations(dtype, gray):
    """Both features on one engine, the same gray, T >= K: gather(head - 1, every env, K, dtype) equals pgv_policy_obs bit
    for bit after every step and every reset — on the device, and both against the model."""
    K = 4
    v, model = ProcgenVecEnv("maze", N, seed_base=1), HistoryVec("maze", N, T, gray, ring=False)
    v.reset(), model.first_reset()
    # both enabled at the same moment, behind the first full reset: the masked reset below finds head == 0 and a whole slab
    v.policy_obs = torch.zeros((N, K * (1 if gray else 3), 64, 64), dtype=getattr(torch, dtype), device="cuda")
    v._before()
    pglib.policy_obs_enable(v.L, v._h, K, gray, dtype, c_void_p(v.policy_obs.data_ptr()))
    v.policy_restart = _device_view(v.L.pgv_policy_obs_restart(v._h), N, "|u1", v.device)
    enable_raw(v, T, gray)
    model.f = Frames(N, T, gray, policy=(K, dtype))
    envs = torch.arange(N, dtype=torch.int32, device="cuda")

    def law(what):
        got = v.history_gather(torch.full((N,), v.history.head - 1, dtype=torch.int64, device="cuda"), envs, stack=K, dtype=dtype)
        assert bool((got.view(torch.uint8) == v.policy_obs.view(torch.uint8)).all()), what
        assert np.array_equal(bits(got), model.stack.out), what
        assert np.array_equal(v.history.pending.cpu().numpy(), v.policy_restart.cpu().numpy()), what

    first = (np.arange(N) % 3 != 0).astype(np.uint8)
    v.reset(mask=first), model.reset(first)
    law("reset at head 0")
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, N)
        v.step(torch.as_tensor(a)), model.step(a)
        law(t)
        if t in (9, 22, 23):
            mask = ((np.arange(N) + t) % 4 == 0).astype(np.uint8)
            v.reset(mask=mask), model.reset(mask)
            law(("reset", t))
    check(v, model.ring, model.obs, "the end")
    v.close(), model.close()


def test_both_features_from_the_constructor():
    """policy_obs= and history= together, the ordinary way: the law from the first full reset on."""
    n, K = 50, 3
    v = ProcgenVecEnv("maze", n, seed_base=1, policy_obs=dict(stack=K, gray=True, dtype="bfloat16"), history=dict(capacity=T, gray=True))
    model = HistoryVec("maze", n, T, True, policy=(K, "bfloat16"))
    v.reset(), model.first_reset()
    for t in range(-1, 14):
        if t >= 0:
            a = synthetic_actions(RUN_SEED, t, n)
            v.step(torch.as_tensor(a)), model.step(a)
        check(v, model.ring, model.obs, t)
        got = v.history_gather([v.history.head - 1] * n, list(range(n)), stack=K, dtype="bfloat16")
        assert np.array_equal(bits(got), bits(v.policy_obs)) and np.array_equal(bits(got), model.stack.out), t
    v.close(), model.close()


def test_enabling_mid_rollout():
    n = 80
    v, model = ProcgenVecEnv("maze", n, seed_base=1), HistoryVec("maze", n, T, True, ring=False)
    v.reset(), model.first_reset()
    for t in range(15):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a)), model.step(a)
    enable_raw(v, T, True)  # the engine's own ring
    model.f.enable_ring()
    assert v.history.head == 0 and bool((v.history.pending == 1).all()) and not bool(v.history.frames.any()) and not bool(v.history.began.any())
    for t in range(15, 30):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a)), model.step(a)
        check(v, model.ring, model.obs, t)
        check_every_held_push(v, model.ring, "float16", t)
        if t == 15:  # the first push began every env's history
            assert bool(model.ring.began[0].all())
    v.close(), model.close()


def test_an_engine_without_the_feature():
    """Outputs byte-equal to a twin with the feature over steps and sequences, every getter NULL / 0, push and gather refused."""
    n = 120
    plain, v = ProcgenVecEnv("bossfight", n, seed_base=1), make("bossfight", n, False)
    L, h = plain.L, plain._h
    assert plain.history is None
    assert L.pgv_history_frames(h) is None and L.pgv_history_began(h) is None and L.pgv_history_pending(h) is None
    assert L.pgv_history_head(h) == 0 and L.pgv_history_capacity(h) == 0
    out = torch.zeros(16, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.pgv_history_push(h) != 0 and b"pgv_history_enable" in L.pgv_last_error()
    assert L.pgv_history_gather(h, c_void_p(idx.data_ptr()), c_void_p(idx.data_ptr()), 1, 4, 1, c_void_p(out.data_ptr())) != 0
    assert b"pgv_history_enable" in L.pgv_last_error()
    with pytest.raises(pglib.EngineError):
        plain.history_push()
    with pytest.raises(pglib.EngineError):
        plain.history_gather([0], [0])
    plain.reset(), v.reset()
    assert np.array_equal(frames_of(plain), frames_of(v))
    for t, actions in protocol_calls(n, lengths=(1, 2, 3, 5, 8, 13) * 2):
        a = torch.as_tensor(actions)
        if len(actions) in (3, 8):
            plain.step_sequence(a), v.step_sequence(a)
        else:
            for row in a:
                plain.step(row), v.step(row)
        assert np.array_equal(frames_of(plain), frames_of(v)), t
        assert np.array_equal(bits(plain.reward), bits(v.reward)) and bool((plain.done == v.done).all()), t
    for i in (0, 1, 63, 64, n - 1):
        assert np.array_equal(state_of(plain, i).view(np.uint32), state_of(v, i).view(np.uint32)), i
    assert L.pgv_snapshot_bytes(plain._h) == L.pgv_snapshot_bytes(v._h) and plain.env_record_bytes == v.env_record_bytes
    assert L.pgv_history_head(h) == 0 and v.history.head > 0
    plain.close(), v.close()
    for bad in (dict(capacity=0), dict(capacity=4, gray=2), dict(capacity=4, colour=True), dict(gray=True), 5):
        with pytest.raises(ValueError):
            ProcgenVecEnv("maze", 4, history=bad)


def test_the_refusals():
    """The refusals of pgv_history_enable, of gather's host checks and of a misaligned obs slab: each leaves a message, and the
    engine's outputs, ring and head as they were — it goes on equal to a twin that never saw any of it."""
    n = 70
    v, twin = ProcgenVecEnv("maze", n, seed_base=1), make("maze", n, False)
    L, h = v.L, v._h

    def ask(capacity=T, gray=0, frames=None, size=None, cfg=True):
        c = pglib.HistoryConfig(ctypes.sizeof(pglib.HistoryConfig) if size is None else size, capacity, gray, frames)
        return L.pgv_history_enable(h, ctypes.byref(c) if cfg else None)

    def refused(rc, who, word):
        assert rc != 0, "not refused"
        msg = L.pgv_last_error().decode()
        assert who in msg and word in msg, msg

    buf = torch.zeros(T * n * 3 * 4096 + 64, dtype=torch.uint8, device="cuda")
    v._before()
    E = "pgv_history_enable"
    refused(ask(capacity=0), E, "capacity"), refused(ask(capacity=-3), E, "capacity")
    refused(ask(gray=2), E, "gray"), refused(ask(gray=-1), E, "gray")
    refused(ask(frames=c_void_p(buf.data_ptr() + 8)), E, "aligned")
    refused(ask(size=16), E, "struct_size"), refused(ask(size=0), E, "struct_size"), refused(ask(cfg=False), E, "struct_size")
    refused(ask(capacity=2**31 - 1), E, "memory")  # a failed allocation: 2^31 slots of the engine's own
    assert L.pgv_history_frames(h) is None and L.pgv_history_capacity(h) == 0 and L.pgv_history_head(h) == 0  # still off
    assert ask(frames=c_void_p(buf.data_ptr())) == 0
    refused(ask(), E, "already")
    v._after()
    v.history = HistoryTensors(v, buf[:T * n * 3 * 4096].view(T, n, 3, 64, 64))
    assert L.pgv_history_frames(h) == buf.data_ptr() and L.pgv_history_capacity(h) == T
    v.reset(), twin.reset()
    for t in range(8):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, n))
        v.step(a), twin.step(a)

    def same(what):
        assert bool((v.obs == twin.obs).all()) and bool((v.reward == twin.reward).all()) and bool((v.done == twin.done).all()), what
        assert v.history.head == twin.history.head and bool((v.history.frames == twin.history.frames).all()), what
        assert bool((v.history.began == twin.history.began).all()) and bool((v.history.pending == twin.history.pending).all()), what

    same("before")
    # gather's host checks
    G = "pgv_history_gather"
    p = torch.full((4,), v.history.head - 1, dtype=torch.int64, device="cuda")
    i = torch.arange(4, dtype=torch.int32, device="cuda")
    rows = torch.full((4 * 8 * 3 * 4096 * 4 + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    P, I, O = c_void_p(p.data_ptr()), c_void_p(i.data_ptr()), c_void_p(rows.data_ptr())
    torch.cuda.synchronize()
    refused(L.pgv_history_gather(h, P, I, 4, 0, 1, O), G, "stack"), refused(L.pgv_history_gather(h, P, I, 4, 9, 1, O), G, "stack")
    refused(L.pgv_history_gather(h, P, I, 4, 4, 4, O), G, "dtype"), refused(L.pgv_history_gather(h, P, I, 4, 4, -1, O), G, "dtype")
    refused(L.pgv_history_gather(h, P, I, -1, 4, 1, O), G, "count")
    refused(L.pgv_history_gather(h, P, I, 4, 4, 1, c_void_p(rows.data_ptr() + 8)), G, "aligned")
    refused(L.pgv_history_gather(h, None, I, 4, 4, 1, O), G, "NULL"), refused(L.pgv_history_gather(h, P, None, 4, 4, 1, O), G, "NULL")
    refused(L.pgv_history_gather(h, P, I, 4, 4, 1, None), G, "NULL")
    torch.cuda.synchronize()
    assert bool((rows == 0x5A).all())
    same("after gather's refusals")
    # a misaligned obs slab: every call that ends with a push, pgv_reset and the push by hand fail and take no step
    odd = torch.zeros(n * OBS_BYTES + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pglib.check(L, L.pgv_bind_outputs(h, c_void_p(odd.data_ptr() + 8), None, None), "pgv_bind_outputs")
    acts = torch.as_tensor(synthetic_actions(RUN_SEED, 8, n), device="cuda")
    mask = torch.ones(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    q = pglib.sequence(2, None, 0, RUN_SEED, "last")
    head = v.history.head
    host_acts = synthetic_actions(RUN_SEED, 8, n)
    for name, call in (("pgv_step", lambda: L.pgv_step(h, c_void_p(acts.data_ptr()))), ("pgv_step_synthetic", lambda: L.pgv_step_synthetic(h, RUN_SEED)),
                       ("pgv_step_host", lambda: L.pgv_step_host(h, host_acts.ctypes.data_as(c_void_p))),
                       ("pgv_reset", lambda: L.pgv_reset(h, c_void_p(mask.data_ptr()), None)),
                       ("pgv_step_sequence", lambda: L.pgv_step_sequence(h, ctypes.byref(q))), ("pgv_history_push", lambda: L.pgv_history_push(h))):
        rc = call()
        msg = L.pgv_last_error().decode()
        assert rc != 0 and "16-byte aligned" in msg and name in msg, (name, rc, msg)
    assert v.history.head == head
    q0 = pglib.sequence(0, None, 0, RUN_SEED, "last")  # (no steps: nothing to push, nothing to check)
    assert L.pgv_step_sequence(h, ctypes.byref(q0)) == 0 and v.history.head == head
    pglib.check(L, L.pgv_bind_outputs(h, c_void_p(v.obs.data_ptr()), None, None), "pgv_bind_outputs")  # (copies the slab back)
    same("after the misaligned slab")
    for t in range(8, 30):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, n))
        v.step(a), twin.step(a)
        same(t)
    for i in (0, n - 1):
        assert np.array_equal(state_of(v, i).view(np.uint32), state_of(twin, i).view(np.uint32))
    assert not bool(buf[T * n * 3 * 4096:].any())
    v.close(), twin.close()


def test_the_gymnasium_adapter_passes_it_through():
    """history= reaches the engine, `.history` is the engine's, and the return values are what a twin without it returns."""
    from procgen2_amd.gym_vector import ProcgenGymVectorEnv
    n = 40
    env = ProcgenGymVectorEnv("maze", n, history=dict(capacity=T, gray=True))
    plain = ProcgenGymVectorEnv("maze", n)
    model = HistoryVec("maze", n, T, True)
    assert env.history is env.engine.history and plain.history is None and tuple(env.history.frames.shape) == (T, n, 1, 64, 64)
    a_, _ = env.reset()
    b_, _ = plain.reset()
    model.first_reset()
    assert bool((a_ == b_).all()) and a_.shape == b_.shape
    for t in range(12):
        a = synthetic_actions(RUN_SEED, t, n)
        got, want = env.step(torch.as_tensor(a)), plain.step(torch.as_tensor(a))
        model.step(a)
        assert all(bool((x == y).all()) for x, y in zip(got[:4], want[:4])), t
        check(env.engine, model.ring, model.obs, t)
    check_every_held_push(env.engine, model.ring, "float16", "the end")
    env.close(), plain.close(), model.close()
