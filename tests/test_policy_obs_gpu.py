"""Policy-ready observations (include/procgen2_vec.h pgv_policy_obs_enable), the GPU half: the HIP engine against the model
of tests/policy_obs_util.py — the oracle's frames through the numpy value / gray rules and the stack with its restart flags
— bit for bit after every call: the obs slab, the policy tensor, the pending flags.

n = 300 envs in the protocol tests: two 256-lane workgroups of the flag kernels, the last wave partial; the push kernel has
a workgroup per env.  The protocol is tests/sequence_util.py's (160 steps of pgo_synthetic_action(7, t, env));
tests/test_policy_obs.py counts, on the oracle, the restarts it reaches through auto-resets.
"""
import ctypes
import functools
from ctypes import c_float, c_void_p

import numpy as np
import pytest
import torch

from engine_util import _dump
from episodes_util import NEXT_STEP, SAME_STEP, synthetic_actions
from oracle_util import OBS_BYTES, OracleVec
from policy_obs_util import DTYPES, PolicyEpisodes, PolicySequence, PolicyStack, PolicyVec, transform
from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import ProcgenVecEnv, _device_view
from sequence_util import GAMES, PROTOCOL_N as N, PROTOCOL_SEED as RUN_SEED, PROTOCOL_STEPS, protocol_calls

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


def make(game, n, K, gray, dtype, **more):
    return ProcgenVecEnv(game, n, seed_base=1, policy_obs=dict(stack=K, gray=gray, dtype=dtype), **more)


def check(v, stack, obs, what):
    """What a call leaves, against the model: the slab, the policy tensor, the pending flags."""
    assert np.array_equal(frames_of(v), obs), "obs, %s" % (what,)
    got = bits(v.policy_obs)
    assert got.shape == stack.out.shape and got.dtype == stack.out.dtype, what
    assert np.array_equal(got, stack.out), "policy tensor, %s" % (what,)
    assert np.array_equal(v.policy_restart.cpu().numpy(), stack.restart), "restart flags, %s" % (what,)


def state_of(v, env):
    return _dump(lambda buf, m: v.L.pgv_dump_state(v._h, env, buf, m), c_float, np.float32)


@pytest.mark.parametrize("game", GAMES)
def test_single_steps_match_the_model(game):
    """All seven games, the 160-step protocol as single step calls, (K = 4, gray, f16) and (K = 3, RGB, u8) side by side
    against one oracle run."""
    configs = ((4, True, "float16"), (3, False, "uint8"))
    envs = [make(game, N, *c) for c in configs]
    model = PolicyVec(game, N, *configs[0])
    other = PolicyStack(N, *configs[1])
    for v in envs:
        assert tuple(v.policy_obs.shape) == (N, v.policy_obs.shape[1], 64, 64) and v.policy_obs.is_contiguous()
        assert bool((v.policy_restart == 1).all()) and not bool(v.policy_obs.any())  # enable pushes nothing
        v.reset()
    model.first_reset()
    other.push(model.obs)
    restarts = 0
    for t in range(PROTOCOL_STEPS):
        a = synthetic_actions(RUN_SEED, t, N)
        found = model.o.done.copy()
        model.step(a)
        other.flag(found)
        other.push(model.obs)
        restarts += int((found != 0).sum())
        for v, stack in zip(envs, (model.stack, other)):
            v.step(torch.as_tensor(a))
            check(v, stack, model.obs, (game, t))
    assert restarts >= 30, restarts  # (coinrun, the smallest: 40 on the oracle — tests/test_policy_obs.py)
    for v in envs:
        v.close()
    model.close()


MATRIX_N, MATRIX_STEPS = 130, 40


@functools.lru_cache(maxsize=None)
def maze_reference(n=MATRIX_N, steps=MATRIX_STEPS):
    """One oracle run of maze shared by the matrix: the reset frame, then per step (frame, the done row the step found)."""
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


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("gray", [True, False])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_every_configuration_on_maze(dtype, gray, K):
    run_configuration(dtype, gray, K)


@pytest.mark.parametrize("gray", [True, False])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_the_strided_store_form(dtype, gray):
    """pgv_set_debug bit 26: every lane stores its own units as they lie, no exchange inside the wave (the form
    docs/OPTLOG.md measures the default against) — the same bytes, for the element sizes where the two forms differ."""
    run_configuration(dtype, gray, 4, debug=1 << 26)


def run_configuration(dtype, gray, K, debug=0):
    rows = maze_reference()
    v = make("maze", MATRIX_N, K, gray, dtype)
    if debug:
        pglib.check(v.L, v.L.pgv_set_debug(v._h, debug), "pgv_set_debug")
    stack = PolicyStack(MATRIX_N, K, gray, dtype)
    assert v.policy_obs.dtype == getattr(torch, dtype) and tuple(v.policy_obs.shape) == (MATRIX_N, K * (1 if gray else 3), 64, 64)
    assert v.L.pgv_policy_obs_bytes_per_env(v._h) == K * (1 if gray else 3) * 4096 * pglib.POLICY_DTYPES[dtype][1]
    assert v.L.pgv_policy_obs(v._h) == v.policy_obs.data_ptr()
    v.reset()
    stack.push(rows[0][0])
    check(v, stack, rows[0][0], "reset")
    restarts = 0
    for t in range(MATRIX_STEPS):
        obs, found = rows[t + 1]
        v.step(torch.as_tensor(synthetic_actions(RUN_SEED, t, MATRIX_N)))
        stack.flag(found)
        stack.push(obs)
        restarts += int((found != 0).sum())
        check(v, stack, obs, t)
    assert restarts >= 3, restarts
    if dtype != "uint8":  # the values a network sees: 0 .. 1
        assert float(v.policy_obs.float().max()) <= 1.0 and float(v.policy_obs.float().min()) >= 0.0
    v.close()


def test_a_single_env():
    v, model = make("maze", 1, 4, True, "float16"), PolicyVec("maze", 1, 4, True, "float16")
    v.reset(), model.first_reset()
    check(v, model.stack, model.obs, "reset")
    for t in range(40):
        a = synthetic_actions(RUN_SEED, t, 1)
        v.step(torch.as_tensor(a)), model.step(a)
        check(v, model.stack, model.obs, t)
    v.close(), model.close()


def enable_raw(v, K, gray, dtype, out=None):
    """pgv_policy_obs_enable on an env made without the feature; `out`: a tensor of the caller's, or None for the engine's own."""
    v._before()  # (the engine's stream behind whatever filled `out`, and the caller's behind the enable: as ProcgenVecEnv does it)
    pglib.policy_obs_enable(v.L, v._h, K, gray, dtype, None if out is None else c_void_p(out.data_ptr()))
    v._after()
    shape = (v.num_envs, K * (1 if gray else 3), 64, 64)
    if out is None:
        count = v.num_envs * v.L.pgv_policy_obs_bytes_per_env(v._h)
        out = _device_view(v.L.pgv_policy_obs(v._h), count, "|u1", v.device).view(getattr(torch, dtype))
    v.policy_obs = out.view(shape)
    v.policy_restart = _device_view(v.L.pgv_policy_obs_restart(v._h), v.num_envs, "|u1", v.device)


def test_a_callers_tensor_and_its_guards():
    """`out` carved from a larger tensor with 4 096 guard bytes of a pattern on each side: untouched after the run."""
    n, K, guard = 67, 4, 4096
    body = n * K * 3 * 4096 * 2
    slab = torch.full((guard + body + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    slab[guard:guard + body] = 0
    out = slab[guard:guard + body].view(torch.float16)
    v, model = ProcgenVecEnv("maze", n, seed_base=1), PolicyVec("maze", n, K, False, "float16")
    enable_raw(v, K, False, "float16", out)
    assert v.L.pgv_policy_obs(v._h) == out.data_ptr()
    v.reset(), model.first_reset()
    for t in range(30):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a)), model.step(a)
    check(v, model.stack, model.obs, "the end")
    assert bool((slab[:guard] == 0xA5).all()) and bool((slab[guard + body:] == 0xA5).all())
    v.close(), model.close()


def test_reset_under_a_mask_mid_rollout():
    """pgv_reset under a mask: the named envs restart with the frame it drew, the others keep every byte and their flags."""
    n = 150
    v, model = make("maze", n, 3, False, "bfloat16"), PolicyVec("maze", n, 3, False, "bfloat16")
    v.reset(), model.first_reset()
    for t in range(45):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a)), model.step(a)
        if t in (9, 30):
            mask = ((np.arange(n) + t) % 3 == 0).astype(np.uint8)
            before = bits(v.policy_obs).copy()
            v.reset(mask=mask), model.reset(mask)
            check(v, model.stack, model.obs, ("masked reset", t))
            after = bits(v.policy_obs)
            assert np.array_equal(after[mask == 0], before[mask == 0])
            named = after[mask != 0]
            assert all(np.array_equal(named[:, 3 * s:3 * s + 3], named[:, -3:]) for s in range(3))
        check(v, model.stack, model.obs, t)
    v.close(), model.close()


@pytest.mark.parametrize("game", ["maze", "bossfight"])
def test_sequences_restart_what_reset_inside(game):
    """The protocol's calls with frames="last" against the model; a twin under frames="none" → render_obs() →
    push_policy_obs() ends with the same obs, tensor and flags (point 5); after the frames="none" call alone the flags are
    the model's and the tensor's bytes are as they were."""
    K, gray, dtype = 4, True, "float16"
    v, twin, model = make(game, N, K, gray, dtype), make(game, N, K, gray, dtype), PolicySequence(game, N, K, gray, dtype)
    v.reset(), twin.reset(), model.first_reset()
    check(v, model.stack, model.obs, "reset")
    inside = 0
    for k, (t, actions) in enumerate(protocol_calls()):
        a = torch.as_tensor(actions)
        before_flags = model.stack.restart.copy()
        before_done = model.m.engine_done.copy()
        res = v.step_sequence(a, frames="last")
        model.sequence(actions, frames_last=True)
        assert res.obs is v.obs
        check(v, model.stack, model.obs, ("last", t))
        inside += int((model.m.dones[:-1] != 0).any(axis=0).sum())
        # the twin, in three calls
        kept = bits(twin.policy_obs).copy()
        twin.step_sequence(a, frames="none")
        found = (np.vstack([before_done[None], model.m.dones[:-1]]) != 0).any(axis=0)
        assert np.array_equal(twin.policy_restart.cpu().numpy(), before_flags | found), ("flags after none", t)
        assert np.array_equal(bits(twin.policy_obs), kept), ("none pushed", t)
        twin.render_obs()
        assert np.array_equal(bits(twin.policy_obs), kept), ("render_obs pushed", t)
        twin.push_policy_obs()
        check(twin, model.stack, model.obs, ("none, render, push", t))
    assert inside >= 30, inside
    v.close(), twin.close(), model.close()


@pytest.mark.parametrize("game", ["maze", "bossfight"])
@pytest.mark.parametrize("mode,limit", [(SAME_STEP, 20), (NEXT_STEP, 0)])
def test_episodes_on_the_device(game, mode, limit):
    """step_episodes held to EpisodeModel plus the stack: same-step with a 20-step limit — an ended env, terminated or
    truncated, holds K copies of its new episode's first frame — and next-step."""
    n, K, gray, dtype = 200, 3, False, "uint8"
    v = make(game, n, K, gray, dtype, autoreset_mode=mode, max_episode_steps=limit, final_obs_capacity=16)
    model = PolicyEpisodes(game, n, mode, K, gray, dtype, max_episode_steps=limit, final_capacity=16)
    v.reset(), model.first_reset()
    ended = truncated = 0
    for t in range(70):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step_episodes(torch.as_tensor(a)), model.step(a)
        check(v, model.stack, model.obs, (mode, t))
        assert np.array_equal(v.episode.ended.cpu().numpy(), model.m.ended)
        c = int(model.m.counts[1])
        assert np.array_equal(v.episode.final_obs[:c].cpu().numpy().reshape(c, OBS_BYTES), model.m.final_obs)  # the HWC terminal frames, as before
        if mode == SAME_STEP:
            where = model.m.ended != 0
            got = bits(v.policy_obs)[where]
            first = transform(model.obs[where], gray, dtype)
            assert np.array_equal(got, np.tile(first, (1, K, 1, 1))), t
        ended += int(model.m.ended.sum())
        truncated += int(model.m.truncated.sum())
    assert ended >= 10 and (mode != SAME_STEP or truncated >= 100), (ended, truncated)  # (200 envs, a limit of 20, 70 steps: three rounds of truncations)
    v.close(), model.close()


def test_loads_restart_the_slots_they_wrote():
    """fork into two slots mid-rollout: the loaded slots restart at their next push and the others move on; load_state
    restarts all; an index outside the batch and a zero-filled record change nothing.  The stack model is fed the engine's
    own rows (what a load leaves in obs and done is tests/test_env_records_gpu.py's subject)."""
    n, K, gray, dtype = 96, 4, True, "float16"
    v = make("maze", n, K, gray, dtype)
    stack = PolicyStack(n, K, gray, dtype)
    v.reset()
    stack.push(frames_of(v))

    def step(t):
        stack.flag(v.done.cpu().numpy())
        v.step(torch.as_tensor(synthetic_actions(RUN_SEED, t, n)))
        stack.push(frames_of(v))
        check(v, stack, frames_of(v), t)

    for t in range(12):
        step(t)
    kept = bits(v.policy_obs).copy()
    v.fork([5, 5], [40, 77])
    where = np.zeros(n, np.uint8)
    where[[40, 77]] = 1
    stack.flag(where)
    assert np.array_equal(v.policy_restart.cpu().numpy(), stack.restart) and stack.restart.sum() >= 2
    assert np.array_equal(bits(v.policy_obs), kept)  # a load pushes nothing
    step(12)
    got = bits(v.policy_obs)
    for slot in (40, 77):
        assert all(np.array_equal(got[slot, s], got[slot, -1]) for s in range(K))
    for t in range(13, 20):
        step(t)
    # nothing written, nothing flagged: an index outside the batch, an empty record
    records = v.save_envs([3, 4])
    flags = v.policy_restart.clone()
    v.load_envs(records, [n + 7, -1])
    empty = records.clone()
    empty.data.zero_()
    v.load_envs(empty, [10, 11])
    assert bool((v.policy_restart == flags).all())
    step(20)
    # a snapshot restarts every env
    snap = v.save_state()
    step(21)
    v.load_state(snap)
    stack.flag(None)
    assert bool((v.policy_restart == 1).all())
    step(22)
    got = bits(v.policy_obs)
    assert all(np.array_equal(got[:, s], got[:, -1]) for s in range(K))
    step(23)
    v.close()


def test_enabling_mid_rollout():
    n, K = 80, 3
    v, model = ProcgenVecEnv("maze", n, seed_base=1), PolicyVec("maze", n, K, True, "float32", enabled=False)
    assert v.L.pgv_policy_obs(v._h) is None and v.L.pgv_policy_obs_restart(v._h) is None and v.L.pgv_policy_obs_bytes_per_env(v._h) == 0
    assert v.L.pgv_policy_obs_push(v._h, None) != 0 and b"pgv_policy_obs_enable" in v.L.pgv_last_error()
    v.reset(), model.first_reset()
    for t in range(15):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a)), model.step(a)
    enable_raw(v, K, True, "float32")  # the engine's own tensor
    model.enable()
    assert bool((v.policy_restart == 1).all()) and not bool(v.policy_obs.any())  # flags all 1, the tensor still zero
    for t in range(15, 30):
        a = synthetic_actions(RUN_SEED, t, n)
        v.step(torch.as_tensor(a)), model.step(a)
        check(v, model.stack, model.obs, t)
        if t == 15:  # the first push filled every stack
            got = bits(v.policy_obs)
            assert all(np.array_equal(got[:, s], got[:, -1]) for s in range(K)) and got.any()
    # a push by hand under a mask, host form: the others keep stack and flag
    mask = (np.arange(n) % 2).astype(np.uint8)
    pglib.check(v.L, v.L.pgv_policy_obs_push_host(v._h, mask.ctypes.data_as(c_void_p)), "pgv_policy_obs_push_host")
    model.stack.push(model.obs, mask)
    check(v, model.stack, model.obs, "masked push")
    v.close(), model.close()


def test_a_misaligned_slab_is_refused_before_anything_is_enqueued():
    """pgv_bind_outputs moves the obs slab to an address that is not 16-byte aligned: every call that ends with a push, and the
    push itself, fails with a message and takes no step; bound to an aligned slab again the engine goes on as its twin,
    which never saw any of it."""
    n, K = 70, 3
    v, twin = make("maze", n, K, True, "float16"), make("maze", n, K, True, "float16")
    L, h = v.L, v._h
    v.reset(), twin.reset()
    for t in range(8):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, n))
        v.step(a), twin.step(a)
    torch.cuda.synchronize()
    odd = torch.zeros(n * OBS_BYTES + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pglib.check(L, L.pgv_bind_outputs(h, c_void_p(odd.data_ptr() + 8), None, None), "pgv_bind_outputs")
    acts = torch.as_tensor(synthetic_actions(RUN_SEED, 8, n), device="cuda")
    mask = torch.ones(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    q = pglib.sequence(2, None, 0, RUN_SEED, "last")
    for name, rc in (("pgv_step", L.pgv_step(h, c_void_p(acts.data_ptr()))), ("pgv_step_synthetic", L.pgv_step_synthetic(h, RUN_SEED)),
                     ("pgv_step_host", L.pgv_step_host(h, synthetic_actions(RUN_SEED, 8, n).ctypes.data_as(c_void_p))),
                     ("pgv_reset", L.pgv_reset(h, c_void_p(mask.data_ptr()), None)), ("pgv_step_sequence", L.pgv_step_sequence(h, ctypes.byref(q))),
                     ("pgv_policy_obs_push", L.pgv_policy_obs_push(h, None)), ("pgv_policy_obs_push_host", L.pgv_policy_obs_push_host(h, None))):
        msg = L.pgv_last_error().decode()
        assert rc != 0 and "16-byte aligned" in msg and "pgv_" in msg, (name, rc, msg)
    # what does not push goes on: a frameless sequence of no steps, the flags as they were
    q0 = pglib.sequence(0, None, 0, RUN_SEED, "none")
    assert L.pgv_step_sequence(h, ctypes.byref(q0)) == 0
    pglib.check(L, L.pgv_bind_outputs(h, c_void_p(v.obs.data_ptr()), None, None), "pgv_bind_outputs")  # (copies the slab back)
    assert bool((v.obs == twin.obs).all()) and bool((v.policy_restart == twin.policy_restart).all())
    for t in range(8, 30):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, n))
        v.step(a), twin.step(a)
        assert bool((v.obs == twin.obs).all()) and bool((v.reward == twin.reward).all()) and bool((v.done == twin.done).all()), t
        assert np.array_equal(bits(v.policy_obs), bits(twin.policy_obs)) and bool((v.policy_restart == twin.policy_restart).all()), t
    for i in (0, n - 1):
        assert np.array_equal(state_of(v, i).view(np.uint32), state_of(twin, i).view(np.uint32))
    v.close(), twin.close()


def test_the_off_path_and_the_refusals():
    """An engine without the feature and one with it produce equal obs / reward / done / state dumps over the protocol;
    every refusal of point 1 leaves a message and an engine that goes on equal to its twin."""
    n = 120
    plain, v = ProcgenVecEnv("bossfight", n, seed_base=1), ProcgenVecEnv("bossfight", n, seed_base=1)
    L, h = v.L, v._h

    def ask(stack=4, gray=1, dtype=1, out=None, size=None, cfg=True):
        c = pglib.PolicyObsConfig(ctypes.sizeof(pglib.PolicyObsConfig) if size is None else size, stack, gray, dtype, out)
        return L.pgv_policy_obs_enable(h, ctypes.byref(c) if cfg else None)

    def refused(rc, word):
        assert rc != 0, "not refused"
        msg = L.pgv_last_error().decode()
        assert "pgv_policy_obs_enable" in msg and word in msg, msg

    buf = torch.zeros(n * 4 * 4096 * 2 + 64, dtype=torch.uint8, device="cuda")
    v._before()
    refused(ask(stack=0), "stack"), refused(ask(stack=9), "stack"), refused(ask(stack=-1), "stack")
    refused(ask(gray=2), "gray"), refused(ask(gray=-1), "gray")
    refused(ask(dtype=4), "dtype"), refused(ask(dtype=-1), "dtype")
    refused(ask(out=c_void_p(buf.data_ptr() + 8)), "aligned")
    refused(ask(size=16), "struct_size"), refused(ask(size=0), "struct_size"), refused(ask(cfg=False), "struct_size")
    assert L.pgv_policy_obs(h) is None and L.pgv_policy_obs_bytes_per_env(h) == 0  # still off
    assert ask(out=c_void_p(buf.data_ptr())) == 0
    refused(ask(), "already")
    assert L.pgv_policy_obs(h) == buf.data_ptr() and L.pgv_policy_obs_bytes_per_env(h) == 4 * 4096 * 2
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
    assert L.pgv_snapshot_bytes(plain._h) == L.pgv_snapshot_bytes(h) and plain.env_record_bytes == v.env_record_bytes
    assert bool(buf[:n * 4 * 4096 * 2].any()) and not bool(buf[n * 4 * 4096 * 2:].any())
    plain.close(), v.close()
    with pytest.raises(ValueError):
        ProcgenVecEnv("maze", 4, policy_obs=dict(stack=9))
    with pytest.raises(ValueError):
        ProcgenVecEnv("maze", 4, policy_obs=dict(stack=2, dtype="int8"))
    with pytest.raises(ValueError):
        ProcgenVecEnv("maze", 4, policy_obs=dict(stack=2, colour=True))


@pytest.mark.parametrize("path", ["next_step", "same_step_host", "same_step_device"])
def test_the_gymnasium_adapter(path):
    """Policy observations from reset and step in the three step paths against the model; info["final_obs*"] stays the HWC
    terminal frame; without policy_obs= the adapter returns what a twin without the engine feature returns."""
    from procgen2_amd.gym_vector import ProcgenGymVectorEnv
    n, K, gray, dtype = 90, 4, True, "float16"
    mode = "next_step" if path == "next_step" else "same_step"
    more = dict(episodes="device", final_obs_capacity=n) if path == "same_step_device" else {}
    env = ProcgenGymVectorEnv("maze", n, autoreset_mode=mode, policy_obs=dict(stack=K, gray=gray, dtype=dtype), **more)
    plain = ProcgenGymVectorEnv("maze", n, autoreset_mode=mode, **more)
    assert env.single_observation_space.shape == (K, 64, 64) and env.single_observation_space.dtype == np.float16
    assert float(env.single_observation_space.high.flat[0]) == 1.0 and env.observation_space.shape == (n, K, 64, 64)
    assert plain.single_observation_space.shape == (64, 64, 3) and plain.single_observation_space.dtype == np.uint8
    if mode == "next_step":
        model = PolicyVec("maze", n, K, gray, dtype)
        model.first_reset()
        stack = model.stack
    else:
        model = PolicyEpisodes("maze", n, SAME_STEP, K, gray, dtype, final_capacity=n)
        model.first_reset()
        stack = model.stack
    obs, _ = env.reset()
    hwc, _ = plain.reset()
    assert obs is env.engine.policy_obs and np.array_equal(bits(obs), stack.out)
    assert np.array_equal(hwc.cpu().numpy().reshape(n, OBS_BYTES), model.obs)
    ended = 0
    for t in range(60):
        a = synthetic_actions(RUN_SEED, t, n)
        model.step(a)
        obs, reward, terminated, truncated, info = env.step(torch.as_tensor(a))
        hwc, reward2, terminated2, _, info2 = plain.step(torch.as_tensor(a))
        assert tuple(obs.shape) == (n, K, 64, 64) and obs.dtype == torch.float16
        assert np.array_equal(bits(obs), stack.out), (path, t)
        assert np.array_equal(env.engine.policy_restart.cpu().numpy(), stack.restart), (path, t)
        assert np.array_equal(hwc.cpu().numpy().reshape(n, OBS_BYTES), model.obs), (path, t)
        assert np.array_equal(bits(reward), bits(reward2)) and bool((terminated == terminated2).all())
        if mode == "same_step" and bool(terminated.any()):
            a_, b_ = info["final_obs_compact"], info2["final_obs_compact"]
            k = int(terminated.sum())
            assert tuple(a_.shape[1:]) == (64, 64, 3) and a_.dtype == torch.uint8 and bool((a_[:k] == b_[:k]).all())
            ended += k
    assert mode == "next_step" or ended >= 3, ended
    env.close(), plain.close(), model.close()
