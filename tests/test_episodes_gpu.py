"""Episodes on the device (include/procgen2_vec.h pgv_step_episodes), the GPU half: the HIP engine against the model of
tests/episodes_util.py — an OracleVec plus numpy counters — bit for bit, every step, on all seven games; the refusals; the
engine that never enabled anything; the Gym adapter's episodes="device" path over the real engine.

n = 300 envs: two 256-lane workgroups, the last wave partial, not a multiple of 64.  Actions are pgo_synthetic_action,
computed on the host and fed to both sides as explicit actions.
"""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from engine_util import EngineVec
from episodes_util import NEXT_STEP, SAME_STEP, EpisodeModel, synthetic_actions
from oracle_util import OBS_BYTES
from procgen2_amd import lib as pglib
from test_modes import NON_DEFAULT
from variant_paths_util import (EPISODE_LIMIT, EPISODE_N, EPISODE_RING, assert_limit_case_covers, run_limit_case)

pytestmark = pytest.mark.gpu

GAMES = ("coinrun", "maze", "bossfight", "climber", "caveflyer", "chaser", "jumper")
N, RUN_SEED, STEPS = 300, 7, 160
# Case 3 (a limit of 23 steps, a ring of 4).  On the CPU oracle, terminated / truncated / steps that overflow the ring in the
# 160 steps: coinrun 1 / 1799 / 6, maze 316 / 1774 / 89, bossfight 61 / 1781 / 16, climber 134 / 1775 / 41, caveflyer
# 157 / 1790 / 47, chaser 0 / 1800 / 6, jumper 125 / 1784 / 44.  The oracle's chaser never terminates inside 23 steps under
# these actions (not once in 3 200 steps of 300 envs, 41 700 episodes; none at a limit of 40 either), so chaser — the game
# whose reset generates its levels inside the masked reset — also runs with a limit of 60, where the oracle gives
# 82 / 518 / 12 and 9 steps with both kinds of ending at once; the model is asked for both kinds wherever it can give them.
LIMIT_CASES = [(g, 23) for g in GAMES] + [("chaser", 60)]


class Engine:
    """ProcgenVecEnv with episodes, driven with host arrays and read back as numpy, as the model is."""

    def __init__(self, game, n, mode, max_episode_steps=0, final_capacity=0, distribution_mode=0):
        import torch
        from procgen2_amd.vec_env import ProcgenVecEnv
        self.torch = torch
        self.v = ProcgenVecEnv(game, n, seed_base=1, autoreset_mode=mode, max_episode_steps=max_episode_steps,
                               final_obs_capacity=final_capacity, distribution_mode=distribution_mode)
        self.n = n

    def rows(self):
        v = self.v
        return v.obs.reshape(self.n, OBS_BYTES).cpu().numpy(), v.reward.cpu().numpy(), v.done.cpu().numpy()

    def reset(self, mask=None):
        self.v.reset(mask=mask)
        return self.rows()[0]

    def plain_step(self, actions):
        self.v.step(self.torch.as_tensor(np.asarray(actions, np.int32)))
        return self.rows()

    def step(self, actions):
        obs, ep = self.v.step_episodes(self.torch.as_tensor(np.asarray(actions, np.int32)))
        assert ep is self.v.episode and ep.counts.dtype == self.torch.int32 and tuple(ep.counts.shape) == (2,)
        assert ep.final_obs.dtype == self.torch.uint8 and tuple(ep.final_obs.shape) == (ep.capacity, 64, 64, 3)
        out = {k: getattr(ep, k).cpu().numpy() for k in ("reward", "terminated", "truncated", "ended", "counts", "ended_env", "ended_return",
                                                        "ended_length", "ended_level_known", "running_return", "running_length")}
        out["ended_level"] = ep.ended_level.view(self.torch.int32).cpu().numpy().view(np.uint32)
        out["final_obs"] = ep.final_obs.reshape(ep.capacity, OBS_BYTES).cpu().numpy()
        return out

    def close(self):
        self.v.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.shape == b.shape and np.array_equal(a, b)


def check_step(eng, model, got, t):
    """Everything one pgv_step_episodes leaves, against the model's step."""
    obs, reward, done = eng.rows()
    assert np.array_equal(obs, model.obs), "obs, step %d" % t
    assert same_bits(reward, model.engine_reward) and np.array_equal(done, model.engine_done), "the engine's own rows, step %d" % t
    for name in ("reward", "terminated", "truncated", "ended", "counts", "running_return", "running_length"):
        assert same_bits(got[name], getattr(model, name)), "%s, step %d" % (name, t)
    c, k = int(got["counts"][0]), int(got["counts"][1])
    for name in ("ended_env", "ended_return", "ended_length", "ended_level", "ended_level_known"):
        assert same_bits(got[name][:c], getattr(model, name)), "%s, step %d" % (name, t)
    assert np.array_equal(got["final_obs"][:k], model.final_obs), "final_obs, step %d" % t


@pytest.mark.parametrize("game", GAMES)
def test_next_step_matches_the_model_and_plain_steps(game):
    """Case 1: NEXT_STEP, no limit.  The engine's own obs / reward / done also equal a second engine's under pgv_step."""
    eng, model, plain = Engine(game, N, NEXT_STEP, 0, 8), EpisodeModel(game, N, NEXT_STEP, 0, 8), EngineVec(game, N)
    assert np.array_equal(eng.reset(), model.first_reset()) and np.array_equal(plain.reset(), model.obs)
    assert np.array_equal(eng.reset(), model.reset()) and np.array_equal(plain.reset(), model.obs)  # (an explicit reset of every env)
    terminations = several = none = 0
    for t in range(STEPS):
        a = synthetic_actions(RUN_SEED, t, N)
        got = eng.step(a)
        model.step(a)
        check_step(eng, model, got, t)
        obs, reward, done = plain.step(a)
        rows = eng.rows()
        assert np.array_equal(rows[0], obs) and same_bits(rows[1], reward) and np.array_equal(rows[2], done), "pgv_step, step %d" % t
        k = int(model.counts[1])
        assert np.array_equal(got["final_obs"][:k], obs[model.ended_env[:k]])  # next-step: the terminal frame is the obs row
        terminations += int(model.counts[0])
        several += model.counts[0] >= 2
        none += model.counts[0] == 0
    assert not model.truncated.any()
    # the oracle's own run covers the ground (the issue's figures: at least 40 / 8 / 19 for every game)
    assert terminations >= 20 and several >= 5 and none >= 5, (terminations, several, none)
    eng.close(), model.close(), plain.close()


@pytest.mark.parametrize("game", GAMES)
def test_same_step_matches_the_model_and_leaves_the_callers_state(game):
    """Case 2: SAME_STEP, no limit, a ring of 8; then 20 plain steps on both: the state is what the caller's loop leaves."""
    eng, model = Engine(game, N, SAME_STEP, 0, 8), EpisodeModel(game, N, SAME_STEP, 0, 8)
    assert np.array_equal(eng.reset(), model.first_reset()) and np.array_equal(eng.reset(), model.reset())
    terminations = 0
    for t in range(STEPS):
        a = synthetic_actions(RUN_SEED, t, N)
        got = eng.step(a)
        model.step(a)
        check_step(eng, model, got, t)
        terminations += int(model.counts[0])
        assert not model.engine_done.any()  # (same-step: no reset is ever left pending)
    assert terminations >= 20, terminations  # (on the CPU oracle: 41 for coinrun, the fewest)
    for t in range(STEPS, STEPS + 20):
        a = synthetic_actions(RUN_SEED, t, N)
        obs, reward, done = eng.plain_step(a)
        want = model.plain_step(a)
        assert np.array_equal(obs, want[0]) and same_bits(reward, want[1]) and np.array_equal(done, want[2]), "plain step %d" % t
    eng.close(), model.close()


@pytest.mark.parametrize("game,T", LIMIT_CASES)
def test_same_step_with_a_limit_and_staggered_episodes(game, T):
    """Case 3: SAME_STEP, max_episode_steps = 23 (chaser: also 60), a ring of 4.  Three plain steps first, each followed by an
    explicit reset of another third of the envs (which zeroes the counters it names), so the limit falls on different steps."""
    cap = 4
    eng, model = Engine(game, N, SAME_STEP, T, cap), EpisodeModel(game, N, SAME_STEP, T, cap)
    assert np.array_equal(eng.reset(), model.first_reset()) and np.array_equal(eng.reset(), model.reset())
    t = 0
    for third in range(3):
        a = synthetic_actions(RUN_SEED, t, N)
        mask = (np.arange(N) % 3 == third).astype(np.uint8)
        obs, reward, done = eng.plain_step(a)
        want = model.plain_step(a)
        assert np.array_equal(obs, want[0]) and np.array_equal(done, want[2])
        assert np.array_equal(eng.reset(mask), model.reset(mask))
        t += 1
    terminated = truncated = overflows = mixed = 0
    for _ in range(STEPS):
        a = synthetic_actions(RUN_SEED, t, N)
        got = eng.step(a)
        model.step(a)
        check_step(eng, model, got, t)
        mixed += bool(model.terminated.any() and model.truncated.any())
        c = int(got["counts"][0])
        assert int(got["counts"][1]) == min(c, cap)
        assert c == 0 or got["ended_length"][:c].max() <= T
        terminated += int(model.terminated.sum())
        truncated += int(model.truncated.sum())
        overflows += model.counts[0] > cap
        t += 1
    assert model.longest <= T
    assert truncated > 0 and overflows >= 1, (terminated, truncated, overflows)
    if (game, T) != ("chaser", 23):  # (see LIMIT_CASES: the oracle's chaser cannot end a game in 23 steps; it does in 60)
        assert terminated > 0 and mixed >= 1, (terminated, truncated, overflows, mixed)
    eng.close(), model.close()


@pytest.mark.parametrize("game,mode", NON_DEFAULT)
def test_same_step_with_a_limit_in_every_variant(game, mode):
    """Case 3 in every non-default distribution mode, 131 envs, 70 steps, everything checked after every step: the
    masked-reset level install that same-step episodes make (pg_prefetch.h level_serve mode 1) runs on the mode's own Level
    and GenLds.  With a limit of 23 every env ends at least twice, so every env's level comes from that install at least
    twice, in jumper-memory and caveflyer-memory too (variant_paths_util.py; tests/test_variant_paths.py asserts the same on
    the oracle alone)."""
    eng = Engine(game, EPISODE_N, SAME_STEP, EPISODE_LIMIT, EPISODE_RING, distribution_mode=mode)
    model = EpisodeModel(game, EPISODE_N, SAME_STEP, EPISODE_LIMIT, EPISODE_RING, distribution_mode=mode)
    assert pglib.MODES[eng.v.distribution_mode] == mode
    assert np.array_equal(eng.reset(), model.first_reset()) and np.array_equal(eng.reset(), model.reset())
    assert_limit_case_covers(*run_limit_case(model, eng, check_step))
    eng.close(), model.close()


@pytest.mark.parametrize("game", ["bossfight", "maze"])
def test_same_step_lists_the_level_that_ended_and_installs_the_assigned_one(game):
    """SAME_STEP in level-seed mode (num_levels = 50) with a level assigned to every odd env before every step:
    ended_level / ended_level_known are the level words the ended envs carried BEFORE the call (snapshots of
    pgv_level_numbers / pgv_level_known), and after it the reset envs are in their new levels — the odd ones in the level
    assigned to them (the same-step reset consumes the pending assignment), the even ones in a level of the set — while
    the envs that go on keep their words."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n, levels = N, 50
    v = ProcgenVecEnv(game, n, seed_base=1, num_levels=levels, autoreset_mode="same_step", final_obs_capacity=8)
    v.reset()
    words = lambda: (v.level_numbers.view(torch.int32).cpu().numpy().view(np.uint32).astype(np.int64), v.level_known.cpu().numpy().copy())
    odd = np.arange(1, n, 2)
    assert words()[1].all() and words()[0].max() < levels and words()[0].any()  # (level-seed mode: every env's level has a number)
    ended_total = assigned_ended = changed = 0
    for t in range(120):
        assigned = 1000 + t * n + np.arange(n)
        v.assign_levels(assigned[odd], odd)
        before_number, before_known = words()
        v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, n)))
        ep = v.episode
        c = int(ep.counts[0])
        env = ep.ended_env[:c].cpu().numpy()
        assert np.array_equal(env, np.nonzero(ep.ended.cpu().numpy())[0])
        got_number = ep.ended_level.view(torch.int32)[:c].cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(got_number, before_number[env]), "ended_level, step %d" % t
        assert np.array_equal(ep.ended_level_known[:c].cpu().numpy(), before_known[env]), "ended_level_known, step %d" % t
        after_number, after_known = words()
        goes_on = np.ones(n, bool)
        goes_on[env] = False
        assert np.array_equal(after_number[goes_on], before_number[goes_on]) and after_known.all()
        was_odd = env % 2 == 1
        assert np.array_equal(after_number[env[was_odd]], assigned[env[was_odd]]), "the assigned level, step %d" % t
        assert (after_number[env[was_odd]] != before_number[env[was_odd]]).all()
        assert (after_number[env[~was_odd]] < levels).all()
        ended_total += c
        assigned_ended += int((before_number[env] >= 1000).sum())
        changed += int((after_number[env] != before_number[env]).sum())
    # the run covers the ground: endings, endings of an assigned level (a number no level of the set has), new levels
    assert ended_total >= 40 and assigned_ended >= 3 and changed >= 20, (ended_total, assigned_ended, changed)
    v.close()


def _twin_steps(a, b, steps, first=0):
    for t in range(first, first + steps):
        acts = synthetic_actions(RUN_SEED, t, a.n)
        x, y = a.step(acts), b.step(acts)
        assert np.array_equal(x[0], y[0]) and same_bits(x[1], y[1]) and np.array_equal(x[2], y[2]), "step %d" % t


def test_refusals_leave_the_engine_as_it_was():
    """Case 5: every refusal leaves a message and an engine that steps as one nobody asked anything of."""
    n = 70
    eng, twin = EngineVec("maze", n), EngineVec("maze", n)
    L, h = eng.L, eng.h
    assert np.array_equal(eng.reset(), twin.reset())
    acts = np.zeros(n, np.int32)

    def refused(rc):
        assert rc != 0 and L.pgv_last_error(), "not refused"
        msg = L.pgv_last_error().decode()
        assert len(msg) > 10
        return msg

    # not enabled: the step calls and the outputs
    assert "pgv_episodes_enable" in refused(L.pgv_step_episodes_host(h, acts.ctypes.data_as(c_void_p)))
    assert "pgv_episodes_enable" in refused(L.pgv_step_episodes_synthetic(h, 1))
    assert "pgv_episodes_enable" in refused(L.pgv_step_episodes(h, c_void_p(L.pgv_done(h))))
    out = pglib.EpisodeOutputs(ctypes.sizeof(pglib.EpisodeOutputs))
    refused(L.pgv_episode_outputs_get(h, ctypes.byref(out)))

    def enable(mode, limit, capacity, size=None):
        cfg = pglib.EpisodeConfig(ctypes.sizeof(pglib.EpisodeConfig) if size is None else size, mode, limit, capacity)
        return L.pgv_episodes_enable(h, ctypes.byref(cfg))
    refused(enable(0, -1, 0))       # max_episode_steps < 0
    refused(enable(1, 0, -1))       # final_capacity outside 0 .. N
    refused(enable(1, 0, n + 1))
    refused(enable(2, 0, 0))        # an unknown mode
    refused(enable(-1, 0, 0))
    refused(enable(0, 10, 0))       # a limit with NEXT_STEP
    refused(enable(1, 0, 0, size=8))  # a struct of another size
    refused(L.pgv_episodes_enable(h, None))
    assert "pgv_episodes_enable" in refused(L.pgv_step_episodes_synthetic(h, 1))  # (still not enabled)
    _twin_steps(eng, twin, 12)
    assert L.pgv_generator_launches(h) == L.pgv_generator_launches(twin.h)
    assert enable(1, 10, n) == 0    # the limits themselves are fine
    assert "already" in refused(enable(1, 10, n))  # once per env
    assert L.pgv_episode_outputs_get(h, ctypes.byref(out)) == 0 and out.reward and out.final_obs and out.running_length
    _twin_steps(eng, twin, 12, first=12)  # enabled, stepped through pgv_step: nothing changes
    eng.close(), twin.close()


def test_never_enabled_engine_and_next_step_engine_agree():
    """Case 6: 60 steps of an engine that never enabled anything beside one enabled in NEXT_STEP and driven through
    pgv_step_episodes: the same obs, reward and done, and the same number of generator launches."""
    plain, eng = EngineVec("coinrun", N), EngineVec("coinrun", N)
    pglib.episodes_enable(eng.L, eng.h, NEXT_STEP, 0, 16)
    assert np.array_equal(plain.reset(), eng.reset())
    for t in range(60):
        a = synthetic_actions(RUN_SEED, t, N)
        want = plain.step(a)
        pglib.check(eng.L, eng.L.pgv_step_episodes_host(eng.h, a.ctypes.data_as(c_void_p)), "pgv_step_episodes_host")
        got = eng._fetch()
        assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]), "step %d" % t
    assert eng.L.pgv_generator_launches(eng.h) == plain.L.pgv_generator_launches(plain.h) > 0
    plain.close(), eng.close()


def test_synthetic_steps_share_the_action_hash_and_the_step_counter():
    """pgv_step_episodes_synthetic against explicit pgo_synthetic_action actions, mixed with pgv_step_synthetic."""
    n = 130
    a, b = EngineVec("bossfight", n), EngineVec("bossfight", n)
    pglib.episodes_enable(a.L, a.h, NEXT_STEP, 0, 0)
    assert np.array_equal(a.reset(), b.reset())
    for t in range(40):
        if t % 5 == 4:
            a.step_quiet(RUN_SEED)
        else:
            pglib.check(a.L, a.L.pgv_step_episodes_synthetic(a.h, RUN_SEED), "pgv_step_episodes_synthetic")
        want = b.step(synthetic_actions(RUN_SEED, t, n))
        got = a._fetch()
        assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]), "step %d" % t
    a.close(), b.close()


def test_loaded_slot_with_a_pending_reset_takes_its_reset_step():
    """NEXT_STEP after pgv_load_envs: a slot whose source had a reset pending is on its reset step (the done row travels)
    and the step is not counted; the running counters stay the slot's own."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n = 64
    v = ProcgenVecEnv("bossfight", n, seed_base=1, autoreset_mode="next_step")
    v.reset()
    t = 0
    while True:  # until some env reports done and some other does not
        v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, n)))
        t += 1
        done = v.done.cpu().numpy()
        if done.any() and not done.all():
            break
        assert t < 400
    playing = (done == 0) & (v.episode.running_length.cpu().numpy() > 0)
    assert playing.any()
    src, dst = int(np.nonzero(done)[0][0]), int(np.nonzero(playing)[0][0])
    before = (float(v.episode.running_return[dst]), int(v.episode.running_length[dst]))
    assert before[1] > 0
    v.fork([src], [dst])
    v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, n)))
    ep = v.episode
    assert int(v.done[dst]) == 0 and int(ep.ended[dst]) == 0 and float(ep.reward[dst]) == 0.0
    assert (float(ep.running_return[dst]), int(ep.running_length[dst])) == before  # the reset step: not counted
    assert int(ep.running_length[src]) == 0  # the source's own reset step
    ep.running_length[dst] = 0  # the caller's to write
    ep.running_return[dst] = 0.0
    v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t + 1, n)))
    assert int(ep.running_length[dst]) == 1 - int(ep.ended[dst]) and int(ep.running_length[src]) == 1 - int(ep.ended[src])
    v.close()


def test_gym_adapter_device_episodes_on_the_real_engine():
    """Case 7: maze, 300 envs, same-step with a limit of 23 and a full-size ring, 60 steps: against the default same-step
    adapter over the real engine until the first truncation, against the model all the way."""
    from procgen2_amd.gym_vector import ProcgenGymVectorEnv
    T = 23
    dev = ProcgenGymVectorEnv("maze", N, episodes="device", autoreset_mode="same_step", max_episode_steps=T, final_obs_capacity=N)
    ref = ProcgenGymVectorEnv("maze", N, autoreset_mode="same_step")
    model = EpisodeModel("maze", N, SAME_STEP, T, N)
    obs, _ = dev.reset()
    ref.reset()
    assert np.array_equal(obs.reshape(N, -1).cpu().numpy(), model.first_reset())
    seen_truncation, compared = False, 0
    for t in range(60):
        a = synthetic_actions(RUN_SEED, t, N)
        obs, reward, terminated, truncated, info = dev.step(a)
        model.step(a)
        assert np.array_equal(obs.reshape(N, -1).cpu().numpy(), model.obs), "obs, step %d" % t
        assert same_bits(reward.cpu().numpy(), model.reward)
        assert np.array_equal(terminated.cpu().numpy(), model.terminated != 0)
        assert np.array_equal(truncated.cpu().numpy(), model.truncated != 0)
        assert np.array_equal(info["_final_obs"].cpu().numpy(), model.ended != 0)
        c, k = (int(x) for x in info["final_count"].cpu().numpy())
        assert [c, k] == list(model.counts) and c == k
        assert np.array_equal(info["final_obs_env"][:c].cpu().numpy(), model.ended_env)
        assert np.array_equal(info["final_obs_compact"][:k].reshape(k, OBS_BYTES).cpu().numpy(), model.final_obs)
        assert same_bits(info["episode"]["r"][:c].cpu().numpy(), model.ended_return)
        assert np.array_equal(info["episode"]["l"][:c].cpu().numpy(), model.ended_length)
        assert not info["episode"]["level_known"][:c].any()
        if not seen_truncation and not model.truncated.any():
            o2, r2, t2, u2, i2 = ref.step(a)
            assert bool((obs == o2).all()) and bool((reward == r2).all()) and bool((terminated == t2).all()) and not bool(u2.any())
            if c:
                compared += 1
                assert bool((info["final_obs_compact"][:k] == i2["final_obs_compact"]).all())
                assert bool((info["final_obs_env"][:c] == i2["final_obs_env"]).all())
        seen_truncation = seen_truncation or bool(model.truncated.any())
    assert seen_truncation and compared >= 1
    dev.close(), ref.close(), model.close()
