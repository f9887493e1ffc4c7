"""Policy-ready observations (include/procgen2_vec.h pgv_policy_obs_enable) without a GPU: the new symbols in the built
libraries and their bindings, the host half of procgen2_amd/csrc/pg_policy_obs.h compiled for the CPU
(tests/cpp/test_policy_obs.cpp), the model the GPU tests trust (tests/policy_obs_util.py) against independent formulations —
torch on the CPU for the values, a deque per env for the stack — the ground the GPU tests' protocol covers, counted on the
oracle, and the Gymnasium adapter over an oracle-backed stand-in."""
import collections
import os
import subprocess

import numpy as np
import pytest

from procgen2_amd import lib as pglib
from policy_obs_util import DTYPES, PolicySequence, PolicyStack, PolicyVec, gray, transform, value_table
from sequence_util import GAMES, PROTOCOL_N, PROTOCOL_STEPS, SequenceModel, protocol_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("pgv_policy_obs_enable", "pgv_policy_obs", "pgv_policy_obs_bytes_per_env", "pgv_policy_obs_restart", "pgv_policy_obs_push",
           "pgv_policy_obs_push_host")


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libMaze.so"])
def test_policy_obs_symbols_exported(engine_lib, libname):
    path = os.path.join(pglib.LIB_DIR, libname)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names


def test_policy_obs_calls_bound(engine_lib):
    for name in SYMBOLS:
        assert hasattr(engine_lib, name) and name in pglib.EXPORTED_VEC_SYMBOLS
    assert engine_lib.pgv_policy_obs_enable.restype is pglib.c_int32 and engine_lib.pgv_policy_obs_push.restype is pglib.c_int32
    assert engine_lib.pgv_policy_obs_bytes_per_env.restype is pglib.c_int64
    assert engine_lib.pgv_policy_obs.restype is pglib.c_void_p and engine_lib.pgv_policy_obs_restart.restype is pglib.c_void_p
    S = pglib.PolicyObsConfig
    # the struct as the header lays it out (LP64): four words, a pointer
    assert pglib.ctypes.sizeof(S) == 24
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16]
    assert pglib.POLICY_DTYPES == {"uint8": (0, 1), "float16": (1, 2), "bfloat16": (2, 2), "float32": (3, 4)}
    # NULL handles: nothing is enabled, nothing is touched
    assert engine_lib.pgv_policy_obs(None) is None and engine_lib.pgv_policy_obs_restart(None) is None
    assert engine_lib.pgv_policy_obs_bytes_per_env(None) == 0
    assert engine_lib.pgv_policy_obs_push(None, None) != 0 and b"pgv_policy_obs_push" in engine_lib.pgv_last_error()
    assert engine_lib.pgv_policy_obs_enable(None, None) != 0 and b"pgv_policy_obs_enable" in engine_lib.pgv_last_error()


def test_tables_and_ownership_on_the_host(tmp_path):
    """pg_policy_obs.h under g++: the 4 x 256 table against the literal anchors and against numpy's (handed over in a file),
    the gray rule, the walk of who writes which byte of an env's block, the listing."""
    tables = np.concatenate([value_table(name).astype(np.uint32) for name in ("uint8", "float16", "bfloat16", "float32")])
    assert tables.shape == (1024,)
    path = str(tmp_path / "tables.bin")
    tables.astype("<u4").tofile(path)
    exe = str(tmp_path / "test_policy_obs")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_policy_obs.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK table file", "OK table", "OK gray", "OK walk", "OK listing", "ALL OK"):
        assert section in out.stdout, section


def test_value_tables_have_the_anchors():
    f32, f16, bf16 = value_table("float32"), value_table("float16"), value_table("bfloat16")
    assert (f32[1], f16[1], bf16[1]) == (0x3B808081, 0x1C04, 0x3B81)
    assert (f16[128], bf16[128]) == (0x3804, 0x3F01)
    assert (f32[255], f16[255], bf16[255]) == (0x3F800000, 0x3C00, 0x3F80)
    for name in DTYPES:
        t = value_table(name)
        assert t.dtype == DTYPES[name] and len(set(t.tolist())) == 256 and t[0] == 0


def test_transform_against_torch_on_the_cpu():
    """The numpy model against an independent formulation: permute / float / 255 / .half() / .bfloat16() in torch."""
    import torch
    rng = np.random.default_rng(5)
    obs = rng.integers(0, 256, (7, 64, 64, 3), dtype=np.uint8)
    obs[0], obs[1] = 0, 255
    t = torch.from_numpy(obs).permute(0, 3, 1, 2).contiguous()
    f = t.float() / 255
    assert np.array_equal(transform(obs, False, "uint8"), t.numpy())
    assert np.array_equal(transform(obs, False, "float32"), f.numpy().view(np.uint32))
    assert np.array_equal(transform(obs, False, "float16"), f.half().view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(transform(obs, False, "bfloat16"), f.bfloat16().view(torch.int16).numpy().view(np.uint16))
    # gray: the rule in torch's integers, then the same conversions
    w = torch.from_numpy(obs.astype(np.int64))
    y = ((77 * w[..., 0] + 150 * w[..., 1] + 29 * w[..., 2] + 128) >> 8)[:, None]
    assert int(y.max()) == 255 and int(y.min()) == 0
    assert np.array_equal(gray(obs)[:, None], y.numpy().astype(np.uint8))
    g = y.float() / 255
    assert np.array_equal(transform(obs.reshape(7, -1), True, "uint8"), y.numpy().astype(np.uint8))
    assert np.array_equal(transform(obs, True, "float16"), g.half().view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(transform(obs, True, "bfloat16"), g.bfloat16().view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(transform(obs, True, "float32"), g.numpy().view(np.uint32))
    assert transform(obs, True, "float16").shape == (7, 1, 64, 64) and transform(obs, False, "float16").shape == (7, 3, 64, 64)


@pytest.mark.parametrize("K,gray_rule", [(1, False), (3, True), (4, False)])
def test_stack_model_against_a_deque_per_env(K, gray_rule):
    """Random frames, masks and flags: slot 0 is the oldest frame (Gymnasium's FrameStackObservation order); a flagged env
    that is pushed restarts with K copies and loses its flag; an env a mask leaves out keeps its stack and its flag."""
    rng = np.random.default_rng(K)
    n, C = 9, 1 if gray_rule else 3
    stack = PolicyStack(n, K, gray_rule, "uint8")
    assert stack.restart.all() and not stack.out.any()
    ques = [None] * n
    flags = np.ones(n, bool)
    for step in range(30):
        frame = rng.integers(0, 256, (n, 64, 64, 3), dtype=np.uint8)
        new = transform(frame, gray_rule, "uint8")
        if step % 4 == 1:
            where = rng.integers(0, 2, n).astype(np.uint8)
            stack.flag(where)
            flags |= where != 0
        if step == 17:
            stack.flag(None)
            flags[:] = True
        mask = None if step % 3 else rng.integers(0, 2, n).astype(np.uint8)
        if step == 0:
            mask = np.arange(n) % 2  # (some envs are first pushed later than others)
        stack.push(frame, mask)
        for i in range(n):
            if mask is not None and not mask[i]:
                continue
            if flags[i]:
                ques[i] = collections.deque([new[i]] * K, maxlen=K)
            else:
                ques[i].append(new[i])
            flags[i] = False
        for i in range(n):
            want = np.zeros((K * C, 64, 64), np.uint8) if ques[i] is None else np.concatenate(list(ques[i]))
            assert np.array_equal(stack.out[i], want), (step, i)
        assert np.array_equal(stack.restart != 0, flags), step


# The ground the GPU tests' protocol covers (tests/sequence_util.py: 300 envs, 160 steps as sequences), per game: pushes that
# find an env's restart flag set through an auto-reset; of those, the ones whose reset was served inside the sequence (the
# caller never saw its done); the ones whose done was the previous call's last row.
PUSH_COVERAGE = {"coinrun": (40, 39, 1), "maze": (78, 61, 18), "bossfight": (538, 458, 80), "climber": (92, 72, 20),
                 "caveflyer": (62, 50, 12), "chaser": (201, 148, 53), "jumper": (104, 87, 17)}


@pytest.mark.parametrize("game", GAMES)
def test_protocol_covers_restarts_through_auto_resets(game):
    m = SequenceModel(game, PROTOCOL_N, render=False)
    m.reset()
    flagged = inside = across = steps = 0
    for _, actions in protocol_calls():
        T = len(actions)
        before = m.engine_done.copy()
        _, dones = m.sequence(actions)
        found = np.vstack([before[None], dones[:T - 1]]) != 0  # the done row as sub-step t finds it
        flagged += int(found.any(axis=0).sum())
        inside += int(found[1:].any(axis=0).sum())
        across += int(found[0].sum())
        steps += T
    m.close()
    assert steps == PROTOCOL_STEPS == 160
    assert (flagged, inside, across) == PUSH_COVERAGE[game]
    assert inside >= 30 and across >= 1


def test_sequence_driver_point_five():
    """The model's own point 5: frames none, then the drawn frame, then a push by hand — what frames last leaves."""
    n = 40
    a, b = PolicySequence("maze", n, 3, True, "uint8"), PolicySequence("maze", n, 3, True, "uint8")
    a.first_reset(), b.first_reset()
    restarts = 0
    for k, (t, actions) in enumerate(protocol_calls(n, lengths=(1, 2, 3, 5, 8, 13) * 2)):
        a.sequence(actions, frames_last=True)
        b.sequence(actions, frames_last=False, draw=True)
        restarts += int(b.stack.restart.sum())
        b.push()
        assert np.array_equal(a.stack.out, b.stack.out) and np.array_equal(a.stack.restart, b.stack.restart) and np.array_equal(a.obs, b.obs)
    assert restarts >= 5
    a.close(), b.close()


class OraclePolicyEngine:
    """The adapter's engine contract with a policy_obs tensor, on the CPU: what ProcgenVecEnv(policy_obs=...) offers, made
    of the model (numpy arrays where the real one has device tensors; bit patterns viewed as the dtype)."""

    def __init__(self, game, n, K, gray_rule, dtype):
        self.m = PolicyVec(game, n, K, gray_rule, dtype)
        self.game, self.num_envs, self.dtype, self.fresh = game, n, dtype, True

    @property
    def policy_obs(self):
        return self.m.out.view(np.dtype(self.dtype))

    def reset(self, mask=None, seeds=None):
        assert seeds is None
        first, self.fresh = self.fresh and mask is None, False
        return (self.m.first_reset() if first else self.m.reset(mask)).reshape(self.num_envs, 64, 64, 3)

    def step(self, actions):
        obs, reward, done = self.m.step(np.asarray(actions))
        return obs.reshape(self.num_envs, 64, 64, 3), reward, done

    def close(self):
        self.m.close()


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_adapter_hands_out_the_policy_tensor(mode):
    """GymVectorAdapter(policy_obs=...) over the stand-in: the spaces, and reset / step returning the stacked tensor in the
    default path and the host same-step path — where an ended env holds K copies of its new first frame and the info keeps
    the HWC terminal frame."""
    from episodes_util import synthetic_actions
    from procgen2_amd.gym_vector import GymVectorAdapter
    n, K = 24, 3
    env = GymVectorAdapter(OraclePolicyEngine("maze", n, K, True, "float16"), output="numpy", autoreset_mode=mode, policy_obs=True)
    plain = GymVectorAdapter(OraclePolicyEngine("maze", n, K, True, "float16"), output="numpy", autoreset_mode=mode)
    assert env.single_observation_space.shape == (K, 64, 64) and env.single_observation_space.dtype == np.float16
    assert env.observation_space.shape == (n, K, 64, 64) and float(env.single_observation_space.high.flat[0]) == 1.0
    assert plain.single_observation_space.shape == (64, 64, 3) and plain.single_observation_space.dtype == np.uint8
    obs, info = env.reset()
    hwc, _ = plain.reset()
    assert obs.shape == (n, K, 64, 64) and obs.dtype == np.float16 and hwc.shape == (n, 64, 64, 3)
    first = transform(hwc, True, "float16").view(np.float16)
    assert np.array_equal(obs, np.tile(first, (1, K, 1, 1)))
    ended = 0
    for t in range(60):
        a = synthetic_actions(7, t, n)
        obs, reward, terminated, truncated, info = env.step(a)
        hwc, reward2, terminated2, _, info2 = plain.step(a)
        assert np.array_equal(reward, reward2) and np.array_equal(terminated, terminated2)
        assert np.array_equal(obs[:, -1:].view(np.uint16), transform(hwc, True, "float16")), t
        if mode == "same_step" and terminated.any():
            where = np.nonzero(terminated)[0]
            assert np.array_equal(info["final_obs_compact"], info2["final_obs_compact"]) and info["final_obs_compact"].shape[1:] == (64, 64, 3)
            for i in where:
                assert all(np.array_equal(obs[i, s], obs[i, -1]) for s in range(K)), (t, i)
            ended += where.size
    assert mode == "next_step" or ended >= 2, ended
    with pytest.raises(ValueError):
        GymVectorAdapter(_NoPolicy(n), policy_obs=True)  # an engine without the tensor
    env.close(), plain.close()


class _NoPolicy:
    def __init__(self, n):
        self.num_envs = n
