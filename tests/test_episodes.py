"""Episodes on the device (include/procgen2_vec.h pgv_step_episodes) without a GPU: the per-env rule of
procgen2_amd/csrc/pg_episodes.h compiled for the CPU and the compaction's arithmetic restated on the host
(tests/cpp/test_episodes.cpp), the new symbols in the built libraries, and the Gym adapter's episodes="device" path over an
oracle-backed stand-in engine whose step_episodes is the model of tests/episodes_util.py."""
import os
import subprocess

import numpy as np
import pytest

from episodes_util import NEXT_STEP, SAME_STEP, EpisodeModel, OracleEpisodeEngine, synthetic_actions
from procgen2_amd import lib as pglib
from procgen2_amd.gym_vector import GymVectorAdapter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("pgv_episodes_enable", "pgv_episode_outputs_get", "pgv_step_episodes", "pgv_step_episodes_synthetic",
           "pgv_step_episodes_host", "pgv_step_episodes_times")


def test_rule_and_compaction_on_the_host(tmp_path):
    exe = str(tmp_path / "test_episodes")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_episodes.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK truncation boundary", "OK reset step", "OK accumulation", "OK compaction", "ALL OK"):
        assert section in out.stdout, section


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libCoinRun.so"])
def test_episode_symbols_exported(engine_lib, libname):
    path = os.path.join(pglib.LIB_DIR, libname)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names


def test_episode_calls_bound(engine_lib):
    for name in SYMBOLS:
        assert getattr(engine_lib, name).restype is pglib.c_int32
        assert name in pglib.EXPORTED_VEC_SYMBOLS
    # the structs as the header lays them out (LP64): four 32-bit words; a word, padding, thirteen pointers
    assert pglib.ctypes.sizeof(pglib.EpisodeConfig) == 16
    assert pglib.ctypes.sizeof(pglib.EpisodeOutputs) == 8 + 13 * 8
    assert pglib.AUTORESET_MODES == {"next_step": 0, "same_step": 1}


def test_model_counts_episodes_as_the_callers_loop_does():
    """The model against a loop written out by hand over a second oracle: same-step with a limit, 60 steps of maze."""
    n, T = 12, 9
    m = EpisodeModel("maze", n, SAME_STEP, max_episode_steps=T, final_capacity=3)
    from oracle_util import OracleVec
    o = OracleVec("maze", n)
    m.first_reset(), o.reset_obs()
    length, ret = np.zeros(n, np.int64), np.zeros(n, np.float32)
    kinds = set()
    for t in range(60):
        a = synthetic_actions(7, t, n)
        m.step(a)
        obs, reward, done = o.step(a)
        length += 1
        ret = (ret + reward).astype(np.float32)
        ended = (done != 0) | (length == T)
        assert np.array_equal(m.ended != 0, ended) and np.array_equal(m.truncated != 0, ended & (done == 0))
        where = np.nonzero(ended)[0]
        assert np.array_equal(m.ended_env, where) and np.array_equal(m.ended_length, length[where])
        assert np.array_equal(m.ended_return.view(np.uint32), ret[where].view(np.uint32))
        assert np.array_equal(m.final_obs, obs[where[:3]]) and list(m.counts) == [where.size, min(where.size, 3)]
        kinds |= {"terminated"} if (done != 0).any() else set()
        kinds |= {"truncated"} if (ended & (done == 0)).any() else set()
        if ended.any():
            o.reset(mask=ended.astype(np.uint8))
            length[ended], ret[ended] = 0, 0
        assert np.array_equal(m.obs, o.obs)
    assert kinds == {"terminated", "truncated"} and m.longest <= T
    m.close(), o.close()


def test_adapter_device_episodes_over_the_model(output="numpy"):
    """episodes="device": one step_episodes call a step and nothing else, real terminated / truncated, the info keys; held
    to the default same-step adapter over a plain engine until the first truncation, to a second model all the way."""
    from test_gym_vector import OracleEngine
    n, T, cap = 10, 17, 4
    dev = GymVectorAdapter(OracleEpisodeEngine("maze", n, SAME_STEP, T, cap), output=output, autoreset_mode="same_step", episodes="device")
    ref = GymVectorAdapter(OracleEngine("maze", n), output=output, autoreset_mode="same_step")
    model = EpisodeModel("maze", n, SAME_STEP, T, cap)
    obs0, info0 = dev.reset()
    ref.reset(), model.first_reset()
    assert info0 == {} and obs0.shape == (n, 64, 64, 3)
    dev.engine.calls.clear()
    seen_truncation, both = False, 0
    for t in range(50):
        a = synthetic_actions(7, t, n)
        obs, reward, terminated, truncated, info = dev.step(a)
        model.step(a)
        assert terminated.dtype == bool and truncated.dtype == bool and info["_final_obs"].dtype == bool
        assert np.array_equal(obs.reshape(n, -1), model.obs) and np.array_equal(reward, model.reward)
        assert np.array_equal(terminated, model.terminated != 0) and np.array_equal(truncated, model.truncated != 0)
        assert np.array_equal(info["_final_obs"], model.ended != 0)
        c, k = (int(x) for x in info["final_count"])
        assert [c, k] == list(model.counts)
        assert np.array_equal(info["final_obs_env"], model.ended_env) and info["final_obs_env"].shape == (c,)
        assert info["final_obs_compact"].shape == (k, 64, 64, 3)
        assert np.array_equal(info["final_obs_compact"].reshape(k, 12288), model.final_obs)
        ep = info["episode"]
        assert set(ep) == {"r", "l", "level", "level_known"} and all(v.shape == (c,) for v in ep.values())
        assert np.array_equal(ep["r"], model.ended_return) and np.array_equal(ep["l"], model.ended_length)
        if not seen_truncation and not truncated.any():
            o2, r2, t2, u2, i2 = ref.step(a)
            assert np.array_equal(obs, o2) and np.array_equal(reward, r2) and np.array_equal(terminated, t2) and not u2.any()
            if t2.any():
                both += 1
                assert np.array_equal(info["final_obs_env"], i2["final_obs_env"])
                assert np.array_equal(info["final_obs_compact"], i2["final_obs_compact"][:k])
        seen_truncation = seen_truncation or bool(truncated.any())
    assert seen_truncation and both >= 1
    assert dev.engine.calls == ["step_episodes"] * 50  # one engine call a step: no reset, no second step
    dev.close(), ref.close(), model.close()


def test_adapter_device_episodes_hands_out_views_without_a_copy():
    """output="torch" over the stand-in: what step() returns ARE the engine's buffers (full-size lists, the counts beside
    them), not copies cut to the counts; terminated / truncated are boolean."""
    n, T, cap = 8, 5, 3
    eng = OracleEpisodeEngine("maze", n, SAME_STEP, T, cap)
    dev = GymVectorAdapter(eng, output="torch", autoreset_mode="same_step", episodes="device")
    dev.reset()
    truncations = 0
    for t in range(6):
        obs, reward, terminated, truncated, info = dev.step(synthetic_actions(7, t, n))
        truncations += int(truncated.sum())
        ep = eng.episode
        assert reward is ep.reward and info["final_obs_compact"] is ep.final_obs and info["final_obs_env"] is ep.ended_env
        assert info["final_count"] is ep.counts and info["episode"]["r"] is ep.ended_return and info["episode"]["l"] is ep.ended_length
        assert info["episode"]["level"] is ep.ended_level and info["episode"]["level_known"] is ep.ended_level_known
        assert info["final_obs_env"].shape == (n,) and info["final_obs_compact"].shape == (cap, 64, 64, 3)
        assert terminated.dtype == bool and truncated.dtype == bool and info["_final_obs"].dtype == bool
        assert np.array_equal(terminated, ep.terminated != 0) and np.array_equal(truncated, ep.truncated != 0)
        assert np.array_equal(info["_final_obs"], ep.ended != 0)
    assert truncations >= 1  # (the fifth step of every episode that did not end before)
    assert eng.calls == ["reset"] + ["step_episodes"] * 6
    dev.close()


def test_adapter_device_episodes_next_step_and_refusals():
    n = 24
    dev = GymVectorAdapter(OracleEpisodeEngine("maze", n, NEXT_STEP, 0, 2), output="numpy", episodes="device")
    model = EpisodeModel("maze", n, NEXT_STEP, 0, 2)
    dev.reset(), model.first_reset()
    ended = 0
    for t in range(120):
        a = synthetic_actions(3, t, n)
        obs, reward, terminated, truncated, info = dev.step(a)
        model.step(a)
        assert np.array_equal(obs.reshape(n, -1), model.obs) and not truncated.any()
        assert np.array_equal(terminated, model.terminated != 0) and np.array_equal(info["episode"]["l"], model.ended_length)
        # next-step: the terminal frame is the obs row itself
        k = int(info["final_count"][1])
        assert np.array_equal(info["final_obs_compact"], obs[info["final_obs_env"][:k]])
        ended += int(info["final_count"][0])
    assert ended >= 3
    dev.close(), model.close()
    from test_gym_vector import OracleEngine
    plain = OracleEngine("maze", 2)
    with pytest.raises(ValueError):
        GymVectorAdapter(plain, episodes="device")  # an engine without step_episodes
    with pytest.raises(ValueError):
        GymVectorAdapter(plain, episodes="host")
    eng = OracleEpisodeEngine("maze", 2, NEXT_STEP)
    with pytest.raises(ValueError):
        GymVectorAdapter(eng, autoreset_mode="same_step", episodes="device")  # the engine was made for the other mode
    GymVectorAdapter(plain, output="numpy").step(np.zeros(2, np.int32))  # the default path: untouched
    plain.close(), eng.close()
