"""Steps without frames (include/procgen2_vec.h pgv_step_sequence, pgv_render_obs), the GPU half: the HIP engine against
the model of tests/sequence_util.py — an OracleVec that draws only what the call draws, plus the numpy fold — bit for bit
after every call on all seven games, and against a twin engine driven by pgv_step.

n = 300 envs: two 256-lane workgroups, the last wave partial, not a multiple of 64.  The protocol (sequence_util.py): 160
steps of pgo_synthetic_action(7, t, env) cut into sequences of (1, 2, 3, 5, 8, 13) x 5; tests/test_sequence.py counts, on the
oracle, the resets that fall inside a sequence, on its last sub-step and on its second-to-last, for every game.
"""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from engine_util import EngineVec
from episodes_util import synthetic_actions
from oracle_util import OBS_BYTES
from procgen2_amd import lib as pglib
from sequence_util import (GAMES, PROTOCOL_N as N, PROTOCOL_SEED as RUN_SEED, PROTOCOL_STEPS, SequenceModel, chaser_late_rows, fold,
                           protocol_calls)
from test_modes import NON_DEFAULT

pytestmark = pytest.mark.gpu

LAST, NONE = 0, 1
OUTPUTS = {"rewards": np.float32, "dones": np.uint8, "seq_return": np.float32, "seq_length": np.int32, "seq_done": np.uint8}


class SeqEngine(EngineVec):
    """EngineVec plus the host-pointer forms of the new calls."""

    def sequence(self, actions=None, steps=None, frames=LAST, run_seed=0, outputs=tuple(OUTPUTS)):
        """actions [T, N] (stride N), [N] with steps (stride 0) or None with steps (synthetic).  Returns the outputs asked
        for as numpy arrays, pre-filled with a pattern no result has."""
        a, stride, T = None, 0, steps
        if actions is not None:
            a = np.ascontiguousarray(actions, np.int32)
            if a.ndim == 2:
                T, stride = a.shape[0], self.n
        out = {}
        for name in outputs:
            shape = (T, self.n) if name in ("rewards", "dones") else (self.n,)
            out[name] = np.full(shape, -77 if OUTPUTS[name] != np.uint8 else 177, OUTPUTS[name])
        q = pglib.sequence(T, None if a is None else a.ctypes.data, stride, run_seed, frames, **{k: v.ctypes.data for k, v in out.items()})
        pglib.check(self.L, self.L.pgv_step_sequence_host(self.h, ctypes.byref(q)), "pgv_step_sequence_host")
        return out

    def render_obs(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        pglib.check(self.L, self.L.pgv_render_obs_host(self.h, None if m is None else m.ctypes.data_as(c_void_p)), "pgv_render_obs_host")
        return self._fetch()[0]

    def launches(self):
        return self.L.pgv_generator_launches(self.h)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def check_rows(eng, model, got, t):
    """What one call leaves beside the frame, against the model: the [T][N] rows, the engine's own rows, the summary."""
    assert same_bits(got["rewards"], model.rewards) and same_bits(got["dones"], model.dones), "rows, call at step %d" % t
    reward, done = eng.fetch_scalars()
    assert same_bits(reward, model.engine_reward) and same_bits(done, model.engine_done), "the engine's own rows, call at step %d" % t
    for name in ("seq_return", "seq_length", "seq_done"):
        assert same_bits(got[name], getattr(model, name)), "%s, call at step %d" % (name, t)


def run_frames_last(game, debug=0, mode=0):
    eng, twin, model = SeqEngine(game, N, mode=mode), SeqEngine(game, N, mode=mode), SequenceModel(game, N, mode=mode)
    assert eng.L.pgv_mode(eng.h) == mode or mode == 0
    if debug:
        eng.set_debug(debug), twin.set_debug(debug)
    assert np.array_equal(eng.reset(), model.first_reset()) and np.array_equal(twin.reset(), model.obs)
    assert np.array_equal(eng.reset(), model.reset()) and np.array_equal(twin.reset(), model.obs)
    steps = inside = 0
    for t, actions in protocol_calls():
        got = eng.sequence(actions, frames=LAST)
        model.sequence(actions)
        check_rows(eng, model, got, t)
        inside += int((model.dones[:-1] != 0).sum())
        assert np.array_equal(eng._fetch()[0], model.obs), "obs, call at step %d" % t
        for a in actions:
            obs, reward, done = twin.step(a)
        assert np.array_equal(eng.obs, obs) and same_bits(eng.reward, reward) and same_bits(eng.done, done), "pgv_step, call at step %d" % t
        assert eng.launches() == twin.launches(), "generator launches, call at step %d" % t
        steps += len(actions)
    assert steps == PROTOCOL_STEPS  # (bossfight and chaser have no level prefetch: their launch count is 0 on both sides)
    eng.close(), twin.close(), model.close()
    return inside


@pytest.mark.parametrize("game", GAMES)
def test_frames_last_matches_the_model_and_plain_steps(game):
    """Test 1: PGV_FRAMES_LAST, explicit actions: rows, own rows, summary and the whole slab against the model after every
    call; a twin under pgv_step has equal rows, obs and generator launches."""
    run_frames_last(game)


@pytest.mark.parametrize("game,debug", [("coinrun", 1 << 8), ("chaser", 1 << 8), ("jumper", 1 << 23)])
def test_frames_last_with_debug_paths(game, debug):
    """Test 3: the same without level prefetch (bit 8: every level is generated inside the step, as more of them are when no
    render kernel gives the generator time) and, for jumper, with the pre-pass's hand-back path (bit 23)."""
    run_frames_last(game, debug)


def run_frames_none(game, mode=0):
    """The body of test_frames_none_then_render_obs (see there), in any distribution mode.  Returns the resets that fell
    inside a sequence.  chaser: the late-pass rows are looked at after every third call, or after every call in a mode where
    every third gives fewer than six (sequence_util.chaser_late_rows); the model then draws every call's last sub-step,
    which changes nothing it computes, and the engine is asked for no frame it would not be asked for otherwise."""
    eng, model = SeqEngine(game, N, mode=mode), SequenceModel(game, N, mode=mode)
    assert eng.L.pgv_mode(eng.h) == mode or mode == 0
    assert np.array_equal(eng.reset(), model.first_reset()) and np.array_equal(eng.reset(), model.reset())
    every_call, late_floor = chaser_late_rows(mode)[1:] if game == "chaser" else (False, 0)
    masked, late_rows, inside = False, 0, 0
    due = np.zeros(N, bool)  # envs whose reset the next sub-step serves
    for k, (t, actions) in enumerate(protocol_calls()):
        draw = k % 3 == 2
        got = eng.sequence(actions, frames=NONE)
        model.sequence(actions, draw_last=draw or every_call)
        check_rows(eng, model, got, t)
        inside += int((model.dones[:-1] != 0).sum())
        reset_last = model.dones[-2] != 0 if len(actions) >= 2 else due
        due = model.dones[-1] != 0
        if game == "chaser" and (draw or every_call):
            assert np.array_equal(eng._fetch()[0][reset_last], model.obs[reset_last]), "the late pass's frames, call at step %d" % t
            late_rows += int(reset_last.sum())
        if not draw:
            continue
        if not masked:
            masked = True
            before = eng._fetch()[0].copy()
            mask = (np.arange(N) % 2 == 0).astype(np.uint8)
            after = eng.render_obs(mask)
            assert np.array_equal(after[1::2], before[1::2]), "a masked pgv_render_obs touched rows it does not name"
            assert np.array_equal(after[0::2], model.obs[0::2]), "the rows a masked pgv_render_obs names"
        assert np.array_equal(eng.render_obs(), model.obs), "pgv_render_obs, call at step %d" % t
        assert np.array_equal(eng.render_obs(), model.obs), "pgv_render_obs twice"
    assert masked and (game != "chaser" or late_rows >= late_floor), late_rows  # (mode 0, on the oracle: 8 such rows in the calls looked at)
    for t in range(PROTOCOL_STEPS, PROTOCOL_STEPS + 20):
        a = synthetic_actions(RUN_SEED, t, N)
        obs, reward, done = eng.step(a)
        want = model.plain_step(a)
        assert np.array_equal(obs, want[0]) and same_bits(reward, want[1]) and same_bits(done, want[2]), "plain step %d" % t
    eng.close(), model.close()
    return inside


@pytest.mark.parametrize("game", GAMES)
def test_frames_none_then_render_obs(game):
    """Test 2: PGV_FRAMES_NONE: rows and summary after every call; after every third, pgv_render_obs(NULL) is the frame
    PGV_FRAMES_LAST would have left — the first time behind a masked pgv_render_obs of every other env, which leaves the
    other rows' bytes alone.  Then 20 plain steps: nothing was left stale.  chaser: "unspecified" still means the late
    pass has drawn the envs reset in the call's last sub-step (their base layers come from that) — those rows are the
    model's before any pgv_render_obs."""
    run_frames_none(game)


@pytest.mark.parametrize("game,mode", NON_DEFAULT)
def test_frames_last_in_every_variant(game, mode):
    """Test 1 in every non-default distribution mode: launch_no_frame and the late pass a frameless step keeps are game
    code, compiled per mode.  At least 10 resets fall inside a sequence (tests/test_variant_paths.py has each pair's count)."""
    inside = run_frames_last(game, mode=mode)
    assert inside >= 10, inside


@pytest.mark.parametrize("game,mode", NON_DEFAULT)
def test_frames_none_then_render_obs_in_every_variant(game, mode):
    """Test 2 in every non-default distribution mode, pgv_render_obs and chaser's late-pass rows included."""
    inside = run_frames_none(game, mode=mode)
    assert inside >= 10, inside


def test_synthetic_sequences_share_the_action_hash_and_the_step_counter():
    """Test 4: actions = NULL with run_seed, mixed with pgv_step_synthetic, against explicit pgo_synthetic_action on a twin."""
    n = 130
    a, b = SeqEngine("bossfight", n), SeqEngine("bossfight", n)
    assert np.array_equal(a.reset(), b.reset())
    t = ended = 0
    for k, T in enumerate((3, 1, 5, 2, 8, 1, 13, 4)):
        if k % 3 == 1:
            a.step_quiet(RUN_SEED)
            b.step(synthetic_actions(RUN_SEED, t, n))
            t += 1
        got = a.sequence(None, steps=T, frames=LAST if k % 2 == 0 else NONE, run_seed=RUN_SEED)
        rewards, dones = np.zeros((T, n), np.float32), np.zeros((T, n), np.uint8)
        for s in range(T):
            obs, rewards[s], dones[s] = b.step(synthetic_actions(RUN_SEED, t, n))
            t += 1
        assert same_bits(got["rewards"], rewards) and same_bits(got["dones"], dones), "call %d" % k
        for name, want in zip(("seq_return", "seq_length", "seq_done"), fold(rewards, dones)):
            assert same_bits(got[name], want), "%s, call %d" % (name, k)
        assert np.array_equal(a.render_obs() if k % 2 else a._fetch()[0], obs), "obs, call %d" % k
        ended += int(dones.sum())
    assert ended >= 5, ended  # (resets inside the synthetic sequences too)
    a.close(), b.close()


def test_action_repeat_is_stride_zero():
    """Test 5: [N] actions with stride 0 against the same row given T times with stride N."""
    a, b = SeqEngine("maze", N), SeqEngine("maze", N)
    assert np.array_equal(a.reset(), b.reset())
    ended = 0
    for k, T in enumerate((4, 1, 7, 16, 3, 9)):
        row = synthetic_actions(RUN_SEED, k, N)
        x = a.sequence(row, steps=T)
        y = b.sequence(np.tile(row, (T, 1)))
        for name in OUTPUTS:
            assert same_bits(x[name], y[name]), "%s, call %d" % (name, k)
        p, q = a._fetch(), b._fetch()
        assert np.array_equal(p[0], q[0]) and same_bits(p[1], q[1]) and same_bits(p[2], q[2]), "call %d" % k
        ended += int(x["seq_done"].sum())
    assert ended >= 5, ended
    a.close(), b.close()


def test_null_outputs_change_nothing_else():
    """Test 6: rows without summary, summary without rows, one of each, neither: what is asked for equals the full call's,
    and the engines agree in everything else."""
    asks = (tuple(OUTPUTS), ("rewards", "dones"), ("seq_return", "seq_length", "seq_done"), ("dones", "seq_return"), ("seq_length",), ())
    engines = [SeqEngine("maze", N) for _ in asks]
    first = engines[0].reset()
    for e in engines[1:]:
        assert np.array_equal(e.reset(), first)
    ended = 0
    for k, (t, actions) in enumerate(protocol_calls(lengths=(1, 2, 3, 5, 8, 13) * 2)):
        frames = NONE if k % 4 == 3 else LAST
        full = engines[0].sequence(actions, frames=frames)
        want = engines[0]._fetch() if frames == LAST else (engines[0].render_obs(),) + engines[0].fetch_scalars()
        want = [x.copy() for x in want]
        for e, ask in zip(engines[1:], asks[1:]):
            got = e.sequence(actions, frames=frames, outputs=ask)
            assert set(got) == set(ask)
            for name in ask:
                assert same_bits(got[name], full[name]), "%s of %r, call %d" % (name, ask, k)
            have = e._fetch() if frames == LAST else (e.render_obs(),) + e.fetch_scalars()
            assert np.array_equal(have[0], want[0]) and same_bits(have[1], want[1]) and same_bits(have[2], want[2]), "%r, call %d" % (ask, k)
            assert e.launches() == engines[0].launches()
        ended += int(full["seq_done"].sum())
    assert ended >= 10, ended
    for e in engines:
        e.close()


def test_look_ahead_over_forked_envs():
    """Test 7: env 3 forked into slots 16 .. 30, fifteen constant actions for 24 frameless sub-steps: the summary equals
    what a second engine gets that forks the same way, takes 24 pgv_steps and is folded in numpy.  Then a slot saved and
    loaded after the frameless steps goes on bit for bit for 20 steps."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n, T = 64, 24
    v, w = ProcgenVecEnv("caveflyer", n, seed_base=1), ProcgenVecEnv("caveflyer", n, seed_base=1)
    v.reset(), w.reset()
    for t in range(10):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, n))
        v.step(a), w.step(a)
    slots = list(range(16, 31))
    v.fork([3] * 15, slots), w.fork([3] * 15, slots)
    acts = np.zeros(n, np.int32)
    acts[16:31] = np.arange(15)
    res = v.step_sequence(torch.as_tensor(acts), steps=T, frames="none")
    assert res.obs is None
    rewards, dones = np.zeros((T, n), np.float32), np.zeros((T, n), np.uint8)
    for t in range(T):
        _, r, d = w.step(torch.as_tensor(acts))
        rewards[t], dones[t] = r.cpu().numpy(), d.cpu().numpy()
    assert same_bits(res.rewards.cpu().numpy(), rewards) and same_bits(res.dones.cpu().numpy(), dones)
    ret, length, done = fold(rewards, dones)
    assert same_bits(res.seq_return.cpu().numpy(), ret) and same_bits(res.seq_length.cpu().numpy(), length) and same_bits(res.seq_done.cpu().numpy(), done)
    assert np.array_equal(v.render_obs().cpu().numpy(), w.obs.cpu().numpy())
    # a record taken after frameless steps
    v.load_envs(v.save_envs([20]), [40]), w.load_envs(w.save_envs([20]), [40])
    for t in range(20):
        a = synthetic_actions(RUN_SEED, 100 + t, n)
        a[40] = a[20]
        a = torch.as_tensor(a)
        v.step(a), w.step(a)
        assert bool((v.obs == w.obs).all()) and same_bits(v.reward.cpu().numpy(), w.reward.cpu().numpy()) and bool((v.done == w.done).all()), "step %d" % t
        assert bool((v.obs[40] == v.obs[20]).all()) and float(v.reward[40]) == float(v.reward[20]) and int(v.done[40]) == int(v.done[20]), "the loaded slot, step %d" % t
    v.close(), w.close()


def test_refusals_leave_the_engine_as_it_was():
    """Test 8: every refusal of contract 6 leaves a message and an engine that steps as one nobody asked anything of;
    steps = 0 succeeds and writes nothing; an engine with episodes enabled does not count a sequence's steps."""
    n = 70
    eng, twin = SeqEngine("maze", n), SeqEngine("maze", n)
    L, h = eng.L, eng.h
    assert np.array_equal(eng.reset(), twin.reset())
    acts = np.zeros((4, n), np.int32)
    rows = np.full((4, n), -77, np.float32)

    def ask(steps=4, frames=LAST, stride=n, size=None, host=True, actions=acts):
        q = pglib.sequence(steps, None if actions is None else actions.ctypes.data, stride, 0, frames, rewards=rows.ctypes.data)
        if size is not None:
            q.struct_size = size
        return (L.pgv_step_sequence_host if host else L.pgv_step_sequence)(h, ctypes.byref(q))

    def refused(rc):
        assert rc != 0 and L.pgv_last_error(), "not refused"
        msg = L.pgv_last_error().decode()
        assert len(msg) > 10
        return msg

    for host in (True, False):  # (the device form is refused before it looks at a pointer)
        assert "steps" in refused(ask(steps=-1, host=host))
        assert "frames" in refused(ask(frames=2, host=host))
        assert "frames" in refused(ask(frames=-1, host=host))
        assert "struct_size" in refused(ask(size=ctypes.sizeof(pglib.Sequence) - 8, host=host))
        assert "struct_size" in refused(ask(size=0, host=host))
        assert "stride" in refused(ask(stride=n - 1, host=host))
        assert "stride" in refused(ask(stride=1, host=host))
        assert "stride" in refused(ask(stride=-n, host=host))
        refused((L.pgv_step_sequence_host if host else L.pgv_step_sequence)(h, None))
        refused((L.pgv_step_sequence_host if host else L.pgv_step_sequence)(None, ctypes.byref(pglib.sequence(1))))
    refused(L.pgv_render_obs(None, None))
    refused(L.pgv_render_obs_host(None, None))
    assert ask(steps=0) == 0 and ask(steps=0, host=False) == 0 and ask(steps=0, actions=None) == 0
    assert (rows == -77).all()  # nothing was written, by any of them
    for t in range(12):
        a = synthetic_actions(RUN_SEED, t, n)
        x, y = eng.step(a), twin.step(a)
        assert np.array_equal(x[0], y[0]) and same_bits(x[1], y[1]) and same_bits(x[2], y[2]), "step %d" % t
    assert eng.launches() == twin.launches()
    eng.close(), twin.close()

    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    v = ProcgenVecEnv("maze", n, seed_base=1, autoreset_mode="next_step")
    v.reset()
    for t in range(6):
        v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, n)))
    length, ret = v.episode.running_length.clone(), v.episode.running_return.clone()
    assert int(length.max()) > 0
    res = v.step_sequence(steps=9, run_seed=RUN_SEED)
    assert tuple(res.rewards.shape) == (9, n)
    assert bool((v.episode.running_length == length).all()) and bool((v.episode.running_return == ret).all())
    v.close()


def test_python_step_sequence_and_render_obs():
    """Test 9: ProcgenVecEnv.step_sequence / render_obs: shapes and dtypes, tensors reused per T, [N] actions with steps=
    against [T, N], everything against the ctypes path."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv, SequenceResult
    v, w, ref = ProcgenVecEnv("maze", N, seed_base=1), ProcgenVecEnv("maze", N, seed_base=1), SeqEngine("maze", N)
    first = ref.reset()
    assert np.array_equal(v.reset().reshape(N, OBS_BYTES).cpu().numpy(), first) and np.array_equal(w.reset().reshape(N, OBS_BYTES).cpu().numpy(), first)
    seen = {}
    for k, T in enumerate((5, 3, 5, 1, 3, 8)):
        row = synthetic_actions(RUN_SEED, k, N)
        frames = "none" if k % 2 else "last"
        res = v.step_sequence(torch.as_tensor(row), steps=T, frames=frames)
        other = w.step_sequence(np.tile(row, (T, 1)), frames=frames)
        want = ref.sequence(row, steps=T, frames=NONE if k % 2 else LAST)
        assert isinstance(res, SequenceResult) and res.rewards.device == v.device
        for name, (shape, dtype) in SequenceResult.layout(T, N).items():
            t = getattr(res, name)
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
            assert same_bits(t.cpu().numpy(), want[name]), "%s, call %d" % (name, k)
            assert bool((t == getattr(other, name)).all()), "%s of [T, N] actions, call %d" % (name, k)
        assert (res.obs is None) == (frames == "none")
        if frames == "last":
            assert res.obs is v.obs and tuple(res.obs.shape) == (N, 64, 64, 3) and res.obs.dtype == torch.uint8
        obs = v.render_obs() if frames == "none" else res.obs
        assert obs is v.obs and np.array_equal(obs.reshape(N, OBS_BYTES).cpu().numpy(), ref.render_obs() if frames == "none" else ref._fetch()[0])
        assert bool((w.render_obs(torch.ones(N, dtype=torch.uint8)) == obs).all())
        assert same_bits(v.reward.cpu().numpy(), ref.fetch_scalars()[0]) and same_bits(v.done.cpu().numpy(), ref.done)
        ptrs = tuple(getattr(res, name).data_ptr() for name in SequenceResult.layout(T, N))
        assert seen.setdefault(T, ptrs) == ptrs, "the tensors of T = %d were not reused" % T
    assert len(set(seen.values())) == len(seen) == 4
    # parts left out; caller-owned tensors
    res = v.step_sequence(steps=4, run_seed=3, rewards=False, summary=False)
    assert res.rewards is None and res.seq_return is None and res.seq_length is None and res.seq_done is None and tuple(res.dones.shape) == (4, N)
    mine = SequenceResult(**{name: torch.zeros(shape, dtype=dtype, device=v.device) for name, (shape, dtype) in SequenceResult.layout(4, N).items()})
    w.step_sequence(steps=4, run_seed=3, rewards=False, summary=False)
    res = v.step_sequence(steps=4, run_seed=3, out=mine)
    other = w.step_sequence(steps=4, run_seed=3)
    assert res.rewards is mine.rewards and res.seq_length is mine.seq_length
    assert bool((mine.rewards == other.rewards).all()) and bool((mine.seq_length == other.seq_length).all()) and int(mine.seq_length.min()) >= 1
    with pytest.raises(ValueError):
        v.step_sequence(torch.zeros(N, dtype=torch.int32))  # [N] actions without steps
    with pytest.raises(ValueError):
        v.step_sequence(steps=4, frames="first")
    with pytest.raises(ValueError):
        v.step_sequence(steps=3, out=mine)  # tensors of another T
    v.close(), w.close(), ref.close()
