"""The feature layers at the batch sizes they are made for, the GPU half: step_episodes across 274 workgroups, policy
observations, the frame history and its plain and augmented gathers across byte offsets 2^31 and 2^32 — the HIP engine
against the models of tests/*_util.py, bit for bit; no tolerance anywhere.

tests/feature_scale_util.py has the plans and says how a reference is had at these sizes: a whole-batch model without
drawing for everything folded from rewards and dones (every env, every call), drawn 64-env slices at the ends of the batch
and around every boundary for the pixels, single drawn envs for ring rows only the whole-batch run can name, and laws that tie
a large tensor to another engine output, checked over the whole tensor with torch on the device.  tests/test_feature_scale.py
establishes on the oracle alone that the plans reach what they are meant to; the tests here assert it again on their own run.

Results are read as a training loop reads them: through torch on the caller's current stream, with no synchronize() and no
env.sync() between an engine call and the read — a missing stream dependency is a failing comparison here.
"""
import gc
from ctypes import c_float, c_uint8

import numpy as np
import pytest
import torch

import feature_scale_util as fs
import custom_levels_util
import history_aug_util
import path_util
from engine_util import _dump
from episodes_util import NEXT_STEP
from history_util import HistoryVec
from policy_obs_util import PolicyVec, value_table
from state_obs_util import assert_rows
from procgen2_amd import lib as pglib

pytestmark = pytest.mark.gpu

CHUNK = 2048  # rows of a whole-tensor check made at once


def make(game, n, **kw):
    from procgen2_amd.vec_env import ProcgenVecEnv
    return ProcgenVecEnv(game, n, seed_base=fs.SEED_BASE, **kw)


def host(t):
    """A device tensor on the host, floats and uint32 as their bit patterns."""
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def bits(x):
    x = np.asarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same(got, want, what):
    """Equal bit for bit: a device tensor or host array against the model's array of the same shape and type."""
    got, want = host(got) if isinstance(got, torch.Tensor) else bits(got), bits(want)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), what


def rows_of(t, a, k):
    """Rows [a, a + k) of an [N, ...] device tensor on the host, one row flat."""
    return host(t[a:a + k].reshape(k, -1))


def free(*envs):
    for v in envs:
        v.close()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def nothing_left_on_the_device():
    """A test's tensors are gone before the next test allocates its own (an env and its HistoryTensors refer to each other)."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


# ---- 1. episodes across many workgroups ---------------------------------------------------------------------------------
def terminal_frame(case, env, t):
    """The frame env `env` ended call `t` on: a drawn one-env model of the case, replayed from the reset."""
    game, mode, limit, _ = case
    m = fs.episode_model(game, mode, limit, 1, n=1, env_offset=env, render=True, threads=1)
    for s in range(t + 1):
        m.step(fs.actions_of(fs.RUN_SEED, s, 1, env))
    assert int(m.counts[0]) == 1, "env %d does not end in call %d of its replay" % (env, t)
    frame = m.final_obs[0].copy()
    m.close()
    return frame


@pytest.mark.parametrize("case", fs.EP_CASES, ids=["%s-%s" % c[:2] for c in fs.EP_CASES])
def test_episodes_across_many_workgroups(case):
    """70 001 envs, 274 workgroups of pg_episodes.h's kernels, 27 calls of step_episodes.  Every call, over all envs against
    the whole-batch EpisodeModel: reward, terminated, truncated, ended, counts, the ended lists up to counts[0], the running
    counters.  Pixels: obs and the ring rows of the envs of five drawn slices against the slices' models; up to 8 ring rows a
    call — the last written, the rows beside workgroup boundaries — against one-env replays; in next_step mode the whole
    ring against obs[ended_env] on the device.  What the case reaches is feature_scale_util.EP_MEETS; the settings that
    differ from the first wish (no limit in next_step, bossfight's ring of 496) are explained at EP_CASES."""
    game, mode, limit, capacity = case
    n, slices = fs.EP_N, fs.EP_SLICES
    v = make(game, n, autoreset_mode=mode, max_episode_steps=limit, final_obs_capacity=capacity)
    whole = fs.episode_model(game, mode, limit, capacity)
    parts = [fs.episode_model(game, mode, limit, k, n=k, env_offset=a, render=True, threads=1) for a, k in slices]
    v.reset()
    for (a, k), p in zip(slices, parts):
        same(rows_of(v.obs, a, k), p.first_reset(), "reset frames of rows %d.." % a)
    ground, spots, ring_rows_in_slices = fs.EpisodeGround(n, capacity), 0, 0
    for t in range(fs.EP_CALLS):
        acts = fs.actions_of(fs.RUN_SEED, t, n)
        obs, ep = v.step_episodes(torch.as_tensor(acts))
        whole.step(acts)
        for name in ("reward", "terminated", "truncated", "ended", "counts", "running_return", "running_length"):
            same(getattr(ep, name), getattr(whole, name), "%s, call %d" % (name, t))
        c, kept = int(whole.counts[0]), int(whole.counts[1])
        for name in ("ended_env", "ended_return", "ended_length", "ended_level_known"):
            same(getattr(ep, name)[:c], getattr(whole, name), "%s, call %d" % (name, t))
        same(ep.ended_level.view(torch.int32)[:c], whole.ended_level.view(np.int32), "ended_level, call %d" % t)
        same(v.reward, whole.engine_reward, "the engine's reward row, call %d" % t)
        same(v.done, whole.engine_done, "the engine's done row, call %d" % t)
        ground.add(whole.ended_env)
        ring_env = whole.ended_env[:kept]
        for (a, k), p in zip(slices, parts):
            p.step(acts[a:a + k])
            same(rows_of(obs, a, k), p.obs, "obs of rows %d.., call %d" % (a, t))
            rows = np.nonzero((ring_env >= a) & (ring_env < a + k))[0]
            if rows.size:
                at = np.searchsorted(p.ended_env, ring_env[rows] - a)
                assert np.array_equal(p.ended_env[at], ring_env[rows] - a)
                got = host(ep.final_obs[torch.as_tensor(rows, device=v.device)].reshape(rows.size, -1))
                same(got, p.final_obs[at], "ring rows of envs %d.., call %d" % (a, t))
                ring_rows_in_slices += rows.size
        for r in fs.ring_spots(whole.ended_env, kept):
            same(ep.final_obs[r].reshape(-1), terminal_frame(case, int(ring_env[r]), t), "ring row %d (env %d), call %d" % (r, ring_env[r], t))
            spots += 1
        if mode == NEXT_STEP and kept:  # the terminal frame is the obs row
            assert torch.equal(ep.final_obs[:kept], obs[ep.ended_env[:kept].long()]), "the ring against obs[ended_env], call %d" % t
    assert ground.met == fs.EP_MEETS[game, mode], ground.met
    assert spots >= 8 and ring_rows_in_slices >= 1, (spots, ring_rows_in_slices)
    whole.close()
    for p in parts:
        p.close()
    del obs, ep
    free(v)


# ---- 3. policy observations beyond 2^32 bytes ---------------------------------------------------------------------------
def device_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def table_on(device, dtype):
    t = value_table(dtype)
    return torch.as_tensor(t.view(np.int32) if t.dtype == np.uint32 else t, device=device)


def assert_policy_law(v, table, prev, fresh, touched, K, what):
    """Over the whole tensor, on the device: an env the push touched holds the new frame — the value table indexed by its
    planar obs row — in its newest slot and, where its stack restarted, in every slot, else its earlier slots moved up by
    one; an env it did not touch holds what it held."""
    n, C = v.num_envs, 3
    fresh, touched = torch.as_tensor(fresh, device=v.device), torch.as_tensor(touched, device=v.device)
    for a in range(0, n, CHUNK):
        b = min(n, a + CHUNK)
        new = table[v.obs[a:b].permute(0, 3, 1, 2).long()]
        want = new.repeat(1, K, 1, 1)
        if prev is not None:
            old = device_bits(prev[a:b])
            want = torch.where(fresh[a:b, None, None, None], want, torch.cat([old[:, C:], new], 1))
            want = torch.where(touched[a:b, None, None, None], want, old)
        assert torch.equal(device_bits(v.policy_obs[a:b]), want), "%s: rows %d..%d of the policy tensor" % (what, a, b)


@pytest.mark.parametrize("game,dtype,K,n,debug", fs.PO_CASES, ids=["%s-%s-K%d-%d%s" % (c[:4] + ("-strided" if c[4] else "",)) for c in fs.PO_CASES])
def test_policy_observations_beyond_4_gib(game, dtype, K, n, debug):
    """A policy tensor of 4.33 GB (rows of 196 608 or 98 304 bytes: env 10 922 / 21 845 holds byte 2^31, env 21 845 / 43 690
    byte 2^32): reset, 9 steps, a masked reset of every third env, 2 more steps.  After every call the rows of four drawn
    slices — the ends of the batch, 64 envs around each of the two — against PolicyVec; policy_restart over all envs against
    the whole-batch flags; the whole tensor against the law of assert_policy_law, whose `fresh` is the whole-batch model's.
    coinrun (whose generator launches run on the side stream) is not asked for episode ends inside the slices: it has 100
    in 40 steps of 65 536 envs."""
    slices = fs.policy_slices(dtype, K, n)
    v = make(game, n, policy_obs=dict(stack=K, gray=False, dtype=dtype))
    if debug:
        pglib.check(v.L, v.L.pgv_set_debug(v._h, debug), "pgv_set_debug")
    assert v.policy_obs.numel() * v.policy_obs.element_size() > 1 << 32
    assert v.L.pgv_policy_obs_bytes_per_env(v._h) * (slices[3][0] + 32) < 1 << 32 < v.L.pgv_policy_obs_bytes_per_env(v._h) * (slices[3][0] + 33)
    parts = [PolicyVec(game, k, K, False, dtype, seed_base=fs.SEED_BASE, env_offset=a) for a, k in slices]
    table, prev, fresh_on_steps = table_on(v.device, dtype), None, 0
    for (kind, arg), m, fresh, touched in fs.run_logic(game, n, fs.policy_calls(n)):
        what = "%s %s" % (kind, "of a third" if kind == "reset" and arg is not None else arg)
        if kind == "reset":
            v.reset(mask=arg)
        else:
            acts = fs.actions_of(fs.RUN_SEED, arg, n)
            v.step(torch.as_tensor(acts))
            fresh_on_steps += int(fresh.sum())
        for (a, k), p in zip(slices, parts):
            if kind == "step":
                p.step(acts[a:a + k])
            elif arg is None:
                p.first_reset()
            else:
                p.reset(arg[a:a + k])
            same(rows_of(v.obs, a, k), p.obs, "%s: obs of rows %d.." % (what, a))
            same(rows_of(v.policy_obs, a, k), p.out.reshape(k, -1), "%s: policy rows %d.." % (what, a))
        same(v.policy_restart, m.f.flags, what + ": policy_restart")
        same(v.done, m.done, what + ": done")
        assert_policy_law(v, table, prev, fresh, touched, K, what)
        prev = v.policy_obs.clone() if prev is None else prev.copy_(v.policy_obs)
        restarted = m.restarted.copy()
    if game == "maze":
        assert fs.slices_restart_and_not(restarted, slices) and fresh_on_steps >= n // 50, fresh_on_steps
    for p in parts:
        p.close()
    del prev, table
    free(v)


# ---- 4. frame history and gathers beyond 2^32 bytes ---------------------------------------------------------------------
def planes_on_device(obs, gray):
    """history_util.planes with torch: the stored planes u8 [N, C, 64, 64] of an obs slab."""
    if not gray:
        return obs.permute(0, 3, 1, 2)
    o = obs.to(torch.int32)
    return ((77 * o[..., 0] + 150 * o[..., 1] + 29 * o[..., 2] + 128) >> 8).to(torch.uint8)[:, None]


def named_rows(parts, slices, pushes, envs, named, rows_of_ring):
    """The model's rows of the named entries: each from the ring of the drawn slice that holds its env."""
    where = [fs.slice_of(slices, int(envs[b])) for b in named]
    out = None
    for s, p in enumerate(parts):
        sel = [j for j, w in enumerate(where) if w[0] == s]
        if not sel:
            continue
        got = rows_of_ring(p.ring, pushes[named[sel]], [where[j][1] for j in sel], named[sel])
        out = np.zeros((len(named),) + got.shape[1:], got.dtype) if out is None else out
        out[sel] = got
    return out


def assert_rows_zero_where_not_held(out, held, what, exactly=True):
    """On the device, over the whole output: a row is all zeros where its entry is not held (and, `exactly`, only there)."""
    flat = device_bits(out).reshape(out.shape[0], -1)
    held = torch.as_tensor(held, device=out.device)
    for a in range(0, out.shape[0], CHUNK):
        some = (flat[a:a + CHUNK] != 0).any(1)
        assert not bool((some & ~held[a:a + CHUNK]).any()), "%s: a row that is not held is not zeros, entries %d.." % (what, a)
        assert not exactly or bool((some | ~held[a:a + CHUNK]).all()), "%s: a held row is zeros, entries %d.." % (what, a)


@pytest.mark.parametrize("gray,n,T,slices", fs.HI_CASES, ids=["rgb-22000x16", "gray-65536x17"])
def test_frame_history_and_gathers_beyond_4_gib(gray, n, T, slices):
    """A ring of 4.33 GB (RGB: frame (slot 7, env 20 762) holds byte 2^31, (slot 15, env 19 525) byte 2^32) or 4.56 GB (gray:
    slot 8 begins at byte 2^31, slot 16 at 2^32), reset plus 19 steps of maze, so that the ring wraps.  Every call: began, pending
    and head over all envs against the whole-batch model; the newest slot's frames of every drawn slice against HistoryVec and,
    on the device, of every env against the obs slab; every slot of the slices after the reset, after the wrap and at the end.
    On the RGB ring then the gathers of feature_scale_util.gather_entries, 22 000 entries of K = 4 float32 — an output of
    4.33 GB whose rows 10 922 and 21 845 hold bytes 2^31 and 2^32: the 256 named entries against the plain-Python gather, zeros
    exactly where an entry is not held over the whole output, gather(head - 1, every env) against the engine's own policy
    tensor over the whole output, and the augmented gather at sizes 64 and 56: the draws of all entries, the named rows."""
    rgb = not gray
    v = make("maze", n, history=dict(capacity=T, gray=gray),
             policy_obs=dict(stack=fs.GATHER_K, gray=False, dtype=fs.GATHER_DTYPE) if rgb else None)
    assert v.history.frames.numel() > 1 << 32
    parts = [HistoryVec("maze", k, T, gray, seed_base=fs.SEED_BASE, env_offset=a) for a, k in slices]
    rows, calls = fs.BeganRows(n, T), fs.history_calls()
    for at, ((kind, arg), m, fresh, touched) in enumerate(fs.run_logic("maze", n, calls)):
        what = "%s %s" % (kind, arg)
        if kind == "reset":
            v.reset()
        else:
            acts = fs.actions_of(fs.RUN_SEED, arg, n)
            v.step(torch.as_tensor(acts))
        rows.add(kind, fresh, touched)
        assert v.history.head == rows.head, what
        same(v.history.began, rows.began, what + ": began")
        same(v.history.pending, m.f.flags, what + ": pending")
        slot = (rows.head - 1) % T
        for (a, k), p in zip(slices, parts):
            p.first_reset() if kind == "reset" else p.step(acts[a:a + k])
            assert p.ring.head == rows.head
            same(rows_of(v.history.frames[slot], a, k), p.ring.frames[slot].reshape(k, -1), "%s: slot %d, rows %d.." % (what, slot, a))
            if at in (0, T + 1, len(calls) - 1):
                same(host(v.history.frames[:, a:a + k].reshape(T, -1)), p.ring.frames.reshape(T, -1), "%s: every slot, rows %d.." % (what, a))
        for a in range(0, n, 4 * CHUNK):
            assert torch.equal(v.history.frames[slot, a:a + 4 * CHUNK], planes_on_device(v.obs[a:a + 4 * CHUNK], gray)), "%s: slot %d against obs" % (what, slot)
        restarted = m.restarted.copy()
    head = rows.head
    assert head == 1 + fs.HI_STEPS > T and fs.slices_restart_and_not(restarted, slices)
    if rgb:
        K, dtype = fs.GATHER_K, fs.GATHER_DTYPE
        pushes, envs, named = fs.gather_entries(n, T, head, slices)
        held = fs.held(pushes, envs, n, T, head)
        assert 0.01 * n <= (~held).sum() <= 0.5 * n
        named_on_device = torch.as_tensor(named, device=v.device)
        room = torch.empty((n, K * 3, 64, 64), dtype=getattr(torch, dtype), device=v.device)  # every gather's output: 4.33 GB once
        out = v.history_gather(pushes, envs, stack=K, dtype=dtype, out=room)
        assert out.numel() * out.element_size() > 1 << 32
        want = named_rows(parts, slices, pushes, envs, named, lambda ring, p, i, e: ring.gather(p, i, K, dtype))
        same(host(out[named_on_device]), want, "the gather's named rows")
        assert_rows_zero_where_not_held(out, held, "gather")
        out = v.history_gather(torch.full((n,), head - 1, dtype=torch.int64), torch.arange(n, dtype=torch.int32), stack=K, dtype=dtype, out=room)
        for a in range(0, n, CHUNK):
            assert torch.equal(device_bits(out[a:a + CHUNK]), device_bits(v.policy_obs[a:a + CHUNK])), "gather(head - 1) against policy_obs, rows %d.." % a
        for size in (64, 56):
            cfg = fs.augment_config(size)
            out, params = v.history_gather(pushes, envs, stack=K, dtype=dtype, augment=dict(fs.AUGMENT, size=size), return_params=True,
                                           out=room.flatten()[:n * K * 3 * size * size].view(n, K * 3, size, size))
            same(params, history_aug_util.aug_params_many(cfg, np.arange(n)), "the draws, size %d" % size)
            want = named_rows(parts, slices, pushes, envs, named,
                              lambda ring, p, i, e: history_aug_util.augment(ring, p, i, K, dtype, cfg, entries=e)[0])
            same(host(out[named_on_device]), want, "the augmented gather's named rows, size %d" % size)
            assert_rows_zero_where_not_held(out, held, "augmented gather, size %d" % size, exactly=False)
        del out, params, room
    for p in parts:
        p.close()
    free(v)


# ---- 2. frameless sequences at batch size -------------------------------------------------------------------------------
def dump(v, what, env):
    """An env's whole state or tile dump through the C ABI, as engine_util.EngineVec has it."""
    if what == "state":
        return _dump(lambda buf, m: v.L.pgv_dump_state(v._h, env, buf, m), c_float, np.float32)
    return _dump(lambda buf, m: v.L.pgv_dump_tiles(v._h, env, buf, m), c_uint8, np.uint8)


@pytest.mark.parametrize("game", list(fs.SEQ_GAMES))
def test_frameless_sequences_at_batch_size(game):
    """65 536 envs, two calls of step_sequence of T sub-steps (feature_scale_util.SEQ_GAMES: chaser's T is 40), the first with
    frames="none", the second with frames="last".  rewards and dones [T, N] and the three summary rows over all envs against
    the whole-batch SequenceModel; the drawn last frame against the models of four drawn slices; against a twin engine that
    made the same 2 T steps with step(), on the device: the reward and done rows of every sub-step, the whole obs slab after the
    second call; the state and tile dumps of every 4 099th env against the twin's and the oracle's."""
    n, T, slices = fs.SEQ_N, fs.SEQ_GAMES[game], fs.SEQ_SLICES
    v, twin = make(game, n), make(game, n)
    whole = fs.sequence_model(game)
    parts = [fs.sequence_model(game, k, env_offset=a, render=True, threads=1) for a, k in slices]
    v.reset(), twin.reset()
    assert torch.equal(v.obs, twin.obs)
    for (a, k), p in zip(slices, parts):
        same(rows_of(v.obs, a, k), p.first_reset(), "reset frames of rows %d.." % a)
    ground = fs.SequenceGround()
    twin_rewards = torch.zeros((T, n), dtype=torch.float32, device=v.device)
    twin_dones = torch.zeros((T, n), dtype=torch.uint8, device=v.device)
    for call, frames in enumerate(("none", "last")):
        acts = fs.sequence_actions(call, T, n)
        on_device = torch.as_tensor(acts, device=v.device)
        res = v.step_sequence(on_device, frames=frames)
        for t in range(T):
            _, reward, done = twin.step(on_device[t])
            twin_rewards[t], twin_dones[t] = reward, done
        whole.sequence(acts)
        ground.add(whole, T)
        what = "call %d (frames=%s)" % (call, frames)
        for name in ("rewards", "dones", "seq_return", "seq_length", "seq_done"):
            same(getattr(res, name), getattr(whole, name), "%s: %s" % (what, name))
        same(v.reward, whole.engine_reward, what + ": the engine's reward row")
        same(v.done, whole.engine_done, what + ": the engine's done row")
        assert torch.equal(res.rewards.view(torch.int32), twin_rewards.view(torch.int32)) and torch.equal(res.dones, twin_dones), what + ": the twin's rows"
        for (a, k), p in zip(slices, parts):
            p.sequence(acts[:, a:a + k], draw_last=frames == "last")
            if frames == "last":
                same(rows_of(res.obs, a, k), p.obs, "%s: the last frame of rows %d.." % (what, a))
    assert torch.equal(v.obs, twin.obs), "the obs slab against the twin's"
    for env in list(range(0, n, fs.SEQ_STRIDE)) + [n - 1]:
        for kind in ("state", "tiles"):
            want = (whole.o.state if kind == "state" else whole.o.tiles)(env)
            same(dump(v, kind, env), want, "%s of env %d against the oracle's" % (kind, env))
            same(dump(twin, kind, env), want, "%s of env %d, the twin's" % (kind, env))
    assert ground.holds(game), (ground.early, ground.late, ground.inside)
    whole.close()
    for p in parts:
        p.close()
    del res, twin_rewards, twin_dones, on_device
    free(v, twin)


# ---- 5. the symbolic layer and caller-made levels at batch size ---------------------------------------------------------
def same_rows_on_device(permuted, ordered, idx, inside, what):
    """On the device: the permuted call's rows of the indices inside the batch are the ordered call's rows of those envs."""
    for p, o in zip(permuted, ordered):
        assert torch.equal(device_bits(p)[inside], device_bits(o)[idx[inside].long()]), what


@pytest.mark.parametrize("game", list(fs.SY_GAMES))
def test_symbolic_observations_at_batch_size(game):
    """65 536 envs after 12 steps.  state_obs and tile_obs (coinrun, chaser), tile_paths with its distance fields (maze,
    caveflyer) and get_levels (maze), each called once for all envs in order and once for 100 003 indices — draws with repeats
    and -1, n, 2^31 - 1, -2^31 at fixed places: the ordered call's rows of 512 sampled envs (the ends of workgroups and of the
    batch among them) against the oracle's state and tile dumps, path_util's queue BFS and custom_levels_util's cell rule; on
    the device, every permuted row against the ordered row of its env, and the rows of the outside indices."""
    n, features = fs.SY_N, fs.SY_GAMES[game]
    v = make(game, n)
    o = fs.OracleVec(game, n, seed_base=fs.SEED_BASE, render=False, threads=fs.host_threads())
    v.reset()
    for t in range(fs.SY_STEPS):
        acts = fs.actions_of(fs.RUN_SEED, t, n)
        v.step(torch.as_tensor(acts))
        o.step(acts)
    same(v.done, o.done, "done after %d steps" % fs.SY_STEPS)
    sample = fs.symbolic_sample()
    states, tiles = [o.state(int(e)) for e in sample], [o.tiles(int(e)) for e in sample]
    on_device = torch.as_tensor(sample, device=v.device)
    idx = torch.as_tensor(fs.symbolic_indices(), device=v.device)
    inside = (idx >= 0) & (idx < n)
    outside = torch.as_tensor([place for place, _ in fs.SY_OUTSIDE], device=v.device)
    assert int((~inside).sum()) == len(fs.SY_OUTSIDE)
    if "state" in features:
        rows, lengths = v.state_obs()
        cells = v.tile_obs()
        assert_rows(host(rows[on_device]).view(np.float32), host(lengths[on_device]), host(cells[on_device]), states, tiles, game)
        p_rows, p_lengths = v.state_obs(idx)
        p_cells = v.tile_obs(idx)
        same_rows_on_device((p_rows, p_lengths, p_cells), (rows, lengths, cells), idx, inside, "state_obs / tile_obs of the index list")
        assert not device_bits(p_rows)[outside].any() and not p_lengths[outside].any() and not p_cells[outside].any()
    if "paths" in features:
        lay = v.path_layout
        want = path_util.model_rows(game, states, tiles, lay.tile_w, lay.tile_h, path_util.GOAL, path_util.AGENT, (0,))
        got = v.tile_paths(dist=True)
        fields = lambda r: (r.dist, r.probe_dist, r.probe_step, r.cells)
        for name, g, w in zip(path_util.Model._fields, fields(got), want):
            same(g[on_device], w, "tile_paths %s of the sampled envs" % name)
        assert int((want.probe_dist > 0).sum()) >= fs.SY_SAMPLE // 2  # (the fields are not trivial: the goal is reached from afar)
        permuted = v.tile_paths(dist=True, envs=idx)
        same_rows_on_device(fields(permuted), fields(got), idx, inside, "tile_paths of the index list")
        assert bool((permuted.dist[outside] == -1).all()) and bool((permuted.probe_dist[outside] == -1).all())
        assert bool((permuted.cells[outside] == -1).all()) and not permuted.probe_step[outside].any()
    if "levels" in features:
        side = custom_levels_util.SIDE[custom_levels_util.HARD]
        want = custom_levels_util.levels_of_dumps(np.stack(states), np.stack(tiles), side)
        got = v.get_levels()
        for name, g, w in zip(want._fields, got, want):
            same(g[on_device], w, "get_levels %s of the sampled envs" % name)
        permuted = v.get_levels(idx)
        same_rows_on_device(permuted, got, idx, inside, "get_levels of the index list")
        assert not permuted.tiles[outside].any() and bool((permuted.agent_cell[outside] == -1).all()) and bool((permuted.goal_cell[outside] == -1).all())
        assert not permuted.background[outside].any() and not device_bits(permuted.background_shift)[outside].any()
    o.close()
    free(v)


def test_levels_of_one_engine_installed_into_another_at_batch_size():
    """Engine A (seed 1) steps 5 times; its get_levels() of all 65 536 envs, every 97th row spoiled so that every refusal
    occurs, goes into engine B (seed 2).  status over all rows against custom_levels_util.status_of; B and a twin that was
    offered nothing agree on every refused env (state and tile rows, obs, reward, done); then 20 steps with the same actions:
    B's reward and done are A's for every installed env up to and including its first done, and its obs too wherever the
    mouse faces the same way — an installed mouse looks right, A's looks where it last moved, and the two agree from the env's
    first horizontal move on.  All of it on the device, under masks kept there."""
    n, side = fs.LV_N, custom_levels_util.SIDE[custom_levels_util.HARD]
    from procgen2_amd.vec_env import ProcgenVecEnv
    A, B, twin = (ProcgenVecEnv("maze", n, seed_base=seed) for seed in (fs.LV_SEEDS[0], fs.LV_SEEDS[1], fs.LV_SEEDS[1]))
    A.reset(), B.reset(), twin.reset()
    for t in range(fs.LV_A_STEPS):
        A.step(torch.as_tensor(fs.actions_of(fs.RUN_SEED, t, n)))
    read = A.get_levels()
    levels, indices = fs.spoil_levels(custom_levels_util.Levels(*(x.cpu().numpy() for x in read)), n, side)
    want = custom_levels_util.status_of(levels, indices, n, side)
    assert fs.levels_plan_holds(want), np.bincount(want, minlength=6)
    status = B.set_levels(type(read)(*(torch.as_tensor(x, device=B.device) for x in levels)), indices=torch.as_tensor(indices, device=B.device))
    same(status, want, "status")
    installed = torch.as_tensor(want == 0, device=B.device)  # (row k is env k wherever a row is installed)
    everything = lambda e: (device_bits(e.state_obs()[0]), e.tile_obs(), e.obs, device_bits(e.reward), e.done)
    for name, b, t in zip(("state", "tiles", "obs", "reward", "done"), everything(B), everything(twin)):
        assert torch.equal(b[~installed], t[~installed]), "a refused env's %s" % name
    assert torch.equal(B.tile_obs()[installed], A.tile_obs()[installed]) and not torch.equal(twin.tile_obs()[installed], A.tile_obs()[installed])
    alive = installed.clone()
    faces = alive & (A.state_obs()[0][:, custom_levels_util.FORWARD] == 1.0)
    # (no claim about the frame the install leaves: an episode's first frame does not show the cheese, A's sixth does)
    compared = 0
    for t in range(fs.LV_A_STEPS, fs.LV_A_STEPS + fs.LV_STEPS):
        acts = fs.actions_of(fs.RUN_SEED, t, n)
        on_device = torch.as_tensor(acts, device=A.device)
        A.step(on_device), B.step(on_device)
        faces |= torch.as_tensor(acts // 3 != 1, device=A.device)  # (a horizontal move turns both mice the same way)
        assert torch.equal(device_bits(B.reward)[alive], device_bits(A.reward)[alive]) and torch.equal(B.done[alive], A.done[alive]), "step %d" % t
        assert torch.equal(B.obs[alive & faces], A.obs[alive & faces]), "obs, step %d" % t
        compared += int((alive & faces).sum())
        alive &= A.done == 0
    assert compared >= 10 * n and int(alive.sum()) >= n // 2
    free(A, B, twin)
