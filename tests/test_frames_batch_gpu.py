"""The batched human-size frames (pgv_render_frames, pg_frame.h TilePainter; need an MI355X): many envs, any size, one
64×64 tile per workgroup, straight into device memory — against the CPU oracle's pgo_render_frame, against the
single-frame path (pgv_render_frame), and through ProcgenVecEnv / GymVectorAdapter.  Bar: byte for byte."""
from ctypes import c_void_p

import numpy as np
import pytest

from engine_util import EngineVec
from oracle_util import assert_same_dump, oracle, oracle_state, register_textures

pytestmark = pytest.mark.gpu

from procgen2_amd import lib as pglib  # noqa: E402

from test_modes import NON_DEFAULT  # noqa: E402

# tests/test_parity_gpu.py FRAME_GAMES: every game, and every distribution mode that is not its game's default
FRAME_GAMES = [("coinrun", 0), ("maze", 0), ("bossfight", 0), ("climber", 0), ("caveflyer", 0), ("chaser", 0),
               ("jumper", 0)] + NON_DEFAULT
GAMES = ("coinrun", "maze", "bossfight", "climber", "caveflyer", "chaser", "jumper")
SIZES = ((512, 512), (160, 160), (200, 120), (64, 64), (131, 77))  # the last: both edges ragged, W·3 odd


def _actions(L, run_seed, step, n, offset=0):
    return np.array([L.pgo_synthetic_action(run_seed, step, offset + e) for e in range(n)], np.int32)


def frames_host(eng, indices, w, h, count=None, out=None):
    """pgv_render_frames_host: indices None → envs 0 .. count-1."""
    idx = None if indices is None else np.ascontiguousarray(indices, np.int32)
    k = (eng.n if count is None else count) if idx is None else idx.size
    if out is None:
        out = np.zeros((k, h, w, 3), np.uint8)
    pglib.check(eng.L, eng.L.pgv_render_frames_host(eng.h, None if idx is None else idx.ctypes.data_as(c_void_p), k, w, h,
                                                    out.ctypes.data_as(c_void_p)), "pgv_render_frames_host")
    return out


def oracle_frame(L, handle, w, h):
    want = np.zeros((h, w, 3), np.uint8)
    L.pgo_render_frame(handle, w, h, want.ctypes.data_as(c_void_p))
    return want


def assert_frame(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        raise AssertionError("%s: %d pixels differ, first at (y=%d, x=%d): %s, expected %s" %
                             (what, len(bad), bad[0][0], bad[0][1], got[bad[0][0], bad[0][1]], want[bad[0][0], bad[0][1]]))


def _oracle_envs(L, game, n, seed, mode=0):
    register_textures(game)
    hs = [L.pgo_make_mode(game.encode(), seed + i, 1, mode) for i in range(n)]
    for h in hs:
        L.pgo_reset(h, 0, 0)
    return hs


def _oracle_step(L, hs, pending, a):
    for i, h in enumerate(hs):
        if pending[i]:
            L.pgo_reset(h, 0, 0)
            pending[i] = False
        else:
            L.pgo_step(h, int(a[i]))
            pending[i] = bool(L.pgo_terminated(h))


@pytest.mark.parametrize("game,mode", FRAME_GAMES)
def test_batched_frames_match_the_oracle(game, mode):
    """Every env of the batch in one call, at five sizes, after the reset and along a 90-step rollout with auto-resets,
    byte for byte against pgo_render_frame of each env's oracle handle."""
    n = 6
    L = oracle()
    eng = EngineVec(game, n, seed_base=71, mode=mode)
    hs = _oracle_envs(L, game, n, 71, mode)
    eng.reset()

    def check(tag):
        for w, h in SIZES:
            got = frames_host(eng, None, w, h)
            for env in range(n):
                assert_frame(got[env], oracle_frame(L, hs[env], w, h), "%s: env %d of %d, %dx%d" % (tag, env, n, w, h))

    check("reset")
    pending = [False] * n
    for s in range(90):
        a = _actions(L, 4, s, n)
        eng.step(a)
        _oracle_step(L, hs, pending, a)
        if s % 30 == 29 or s == 7:
            check("step %d" % s)
    for h in hs:
        L.pgo_close(h)
    eng.close()


def test_indices_counts_and_bad_arguments():
    """A permuted subset with a repeated index, and NULL, give exactly those envs in that order; count = 0 succeeds and
    writes nothing; an index outside the batch yields a zero frame beside right neighbours; bad sizes and a NULL output
    fail with a message."""
    n, w, h = 7, 131, 77
    L = oracle()
    eng = EngineVec("coinrun", n, seed_base=12)
    hs = _oracle_envs(L, "coinrun", n, 12)
    eng.reset()
    pending = [False] * n
    for s in range(25):
        a = _actions(L, 2, s, n)
        eng.step(a)
        _oracle_step(L, hs, pending, a)
    want = [oracle_frame(L, hh, w, h) for hh in hs]
    order = [5, 2, 6, 2, 0]
    got = frames_host(eng, order, w, h)
    for k, env in enumerate(order):
        assert_frame(got[k], want[env], "indices %s: frame %d (env %d)" % (order, k, env))
    got = frames_host(eng, None, w, h)
    for env in range(n):
        assert_frame(got[env], want[env], "NULL indices: env %d" % env)
    got = frames_host(eng, None, w, h, count=3)  # NULL indices and a shorter count: envs 0 .. 2
    for env in range(3):
        assert_frame(got[env], want[env], "NULL indices, count 3: env %d" % env)

    canary = np.full((2, h, w, 3), 0xa5, np.uint8)
    assert eng.L.pgv_render_frames_host(eng.h, None, 0, w, h, canary.ctypes.data_as(c_void_p)) == 0
    assert (canary == 0xa5).all()
    import torch
    dev = torch.full((2, h, w, 3), 0xa5, dtype=torch.uint8, device="cuda")
    assert eng.L.pgv_render_frames(eng.h, None, 0, w, h, c_void_p(dev.data_ptr())) == 0
    pglib.check(eng.L, eng.L.pgv_sync(eng.h), "pgv_sync")
    assert bool((dev == 0xa5).all())

    strays = [1, n, 3, -1, 2147483647, 4]
    got = frames_host(eng, strays, w, h)
    for k, env in enumerate(strays):
        if 0 <= env < n:
            assert_frame(got[k], want[env], "out-of-range neighbours: frame %d (env %d)" % (k, env))
        else:
            assert not got[k].any(), "index %d must give a frame of zeros" % env

    buf = np.zeros((1, 8, 8, 3), np.uint8)
    p = buf.ctypes.data_as(c_void_p)
    for fn in (eng.L.pgv_render_frames_host, eng.L.pgv_render_frames):
        for args in ((None, 1, 0, 8, p), (None, 1, 8, 0, p), (None, 1, 4097, 8, p), (None, 1, 8, 4097, p), (None, 1, 8, 8, None),
                     (None, -1, 8, 8, p)):
            assert fn(eng.h, *args) != 0, args
            assert b"pgv_render_frames" in eng.L.pgv_last_error(), args
        assert fn(None, None, 1, 8, 8, p) != 0
    for hh in hs:
        L.pgo_close(hh)
    eng.close()


@pytest.mark.parametrize("game", GAMES)
def test_batched_frames_equal_the_single_frame_path(game):
    """Two painters, one draw list: pgv_render_frames == pgv_render_frame of the same envs."""
    n = 5
    eng = EngineVec(game, n, seed_base=33)
    eng.reset()
    for s in range(40):
        eng.step(None, run_seed=6)
    for w, h in ((512, 512), (200, 120), (131, 77), (96, 96)):
        got = frames_host(eng, None, w, h)
        for env in range(n):
            assert_frame(got[env], eng.frame(env, w, h), "%s env %d %dx%d against pgv_render_frame" % (game, env, w, h))
    eng.close()


@pytest.mark.parametrize("game", GAMES)
def test_thousands_of_64x64_frames_are_the_observations(game):
    """Where the 64×64 human frame IS the observation a big batch can be checked whole: render_frames(None, 64, 64) ==
    the obs slab for 4 096 envs after 20 synthetic steps.

    Which games that holds for was established on the CPU oracle alone first (pgo_render_frame(h, 64, 64) against
    pgo_obs(h), 12 envs a game, after the reset and after each of 60 synthetic steps with auto-resets, 732 frames a game):
    tried coinrun, maze, bossfight, climber, caveflyer, chaser, jumper — all seven qualified, no frame differed, so all
    seven are used."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n = 4096
    env = ProcgenVecEnv(game, n, seed_base=17)
    env.reset()
    for s in range(20):
        env.step_synthetic(run_seed=3)
    frames = env.render_frames(None, 64, 64)
    assert frames.shape == (n, 64, 64, 3) and frames.dtype == torch.uint8 and frames.device == env.obs.device
    same = (frames == env.obs).reshape(n, -1).all(dim=1)
    torch.cuda.synchronize()
    assert bool(same.all()), "%s: %d of %d envs differ, first env %d" % (game, int((~same).sum()), n, int((~same).nonzero()[0]))
    assert bool(frames.any())
    env.close()


def test_bossfight_step_and_reset_after_a_batched_non_square_frame():
    """D15 (tests/test_parity_gpu.py test_bossfight_step_and_reset_after_a_non_square_human_frame) with the two envs'
    200×120 frames taken in ONE batched call: the frames, the steps that follow, the masked reset and the state dump all
    equal the oracle doing pgo_render_frame on those two handles."""
    register_textures("bossfight")
    L = oracle()
    n, W, H = 8, 200, 120
    eng = EngineVec("bossfight", n, seed_base=9)
    hs = [L.pgo_make(b"bossfight", 9 + i, 1) for i in range(n)]
    for h in hs:
        L.pgo_reset(h, 0, 0)
    assert np.array_equal(eng.reset(), np.stack([np.ctypeslib.as_array(L.pgo_obs(h), shape=(12288,)) for h in hs]))
    pending = [False] * n
    for s in range(140):
        if s % 9 == 4:  # a human frame of two envs between steps; env 3 is also reset right after its frame
            got = frames_host(eng, [1, 3], W, H)
            for k, env in enumerate((1, 3)):
                assert_frame(got[k], oracle_frame(L, hs[env], W, H), "step %d env %d" % (s, env))
            if s % 18 == 4:
                mask = np.zeros(n, np.uint8)
                mask[3] = 1
                o = eng.reset(mask=mask)
                L.pgo_reset(hs[3], 0, 0)
                pending[3] = False
                assert np.array_equal(o[3], np.ctypeslib.as_array(L.pgo_obs(hs[3]), shape=(12288,))), s
                assert_same_dump(eng.state(3), oracle_state(hs[3]), "state env 3, step %d" % s)
        a = np.where(np.arange(n) % 2 == 0, 9, _actions(L, 3, s, n)).astype(np.int32)
        oe, re_, de = eng.step(a)
        for i, h in enumerate(hs):
            if pending[i]:
                L.pgo_reset(h, 0, 0)
                pending[i] = False
                assert re_[i] == 0.0 and de[i] == 0
            else:
                L.pgo_step(h, int(a[i]))
                pending[i] = bool(L.pgo_terminated(h))
                assert re_[i] == np.float32(L.pgo_reward(h)) and de[i] == int(L.pgo_terminated(h)), (s, i)
            assert np.array_equal(oe[i], np.ctypeslib.as_array(L.pgo_obs(h), shape=(12288,))), (s, i)
        if s % 35 == 20:
            for i in (1, 3):
                assert_same_dump(eng.state(i), oracle_state(hs[i]), "state env %d, step %d" % (i, s))
    for h in hs:
        L.pgo_close(h)
    eng.close()


def test_device_path_and_stream_order_through_python():
    """ProcgenVecEnv.render_frames with a device index tensor and out=: a step enqueued right behind it, with no host
    synchronisation in between, does not disturb the frames already produced, and frames asked for right after a step
    show that step — both against host-path frames of the same states, taken from a twin env that is synchronised at
    every turn.  out= is checked like the constructor's."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n, w, h = 48, 160, 96
    env = ProcgenVecEnv("climber", n, seed_base=21)
    twin = EngineVec("climber", n, seed_base=21)
    env.reset()
    twin.reset()
    acts = [torch.randint(0, 15, (n,), dtype=torch.int32, generator=torch.Generator().manual_seed(s)) for s in range(13)]
    for s in range(10):
        env.step(acts[s])
        twin.step(acts[s].numpy())
    order = [40, 3, 3, 17, 0, 47]
    idx = torch.tensor(order, dtype=torch.int32, device="cuda")
    out = torch.empty((len(order), h, w, 3), dtype=torch.uint8, device="cuda")
    dev_acts = [a.cuda() for a in acts]
    torch.cuda.synchronize()
    before = env.render_frames(idx, w, h, out=out)  # state after 10 steps …
    assert before.data_ptr() == out.data_ptr()
    env.step(dev_acts[10])                          # … a step right behind it, nothing synchronised …
    env.step(dev_acts[11])
    after = env.render_frames(idx, w, h)            # … and frames right behind that step
    env.step(dev_acts[12])
    torch.cuda.synchronize()
    want_before = frames_host(twin, order, w, h)
    twin.step(acts[10].numpy())
    twin.step(acts[11].numpy())
    want_after = frames_host(twin, order, w, h)
    assert np.array_equal(before.cpu().numpy(), want_before), "a later step disturbed frames already produced"
    assert np.array_equal(after.cpu().numpy(), want_after), "frames behind a step do not show that step"
    assert not np.array_equal(want_before, want_after)

    everyone = env.render_frames(width=96, height=64)
    assert everyone.shape == (n, 64, 96, 3)
    assert env.render_frames([], w, h).shape == (0, h, w, 3)
    for bad in (torch.empty((len(order), h, w, 3), dtype=torch.uint8), torch.empty((len(order), h, w + 1, 3), dtype=torch.uint8, device="cuda"),
                torch.empty((len(order), h, w, 3), dtype=torch.int8, device="cuda"),
                torch.empty((len(order), h, w, 6), dtype=torch.uint8, device="cuda")[..., ::2]):
        with pytest.raises(ValueError):
            env.render_frames(idx, w, h, out=bad)
    with pytest.raises(ValueError):
        env.render_frames(idx, 0, h)
    env.close()
    twin.close()


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_gym_render_batch_equals_the_stacked_single_renders(output):
    from procgen2_amd.gym_vector import ProcgenGymVectorEnv
    n = 5
    env = ProcgenGymVectorEnv("jumper", n, seed=8, output=output, render_mode="rgb_array", render_size=(200, 120))
    env.reset()
    for s in range(12):
        env.step(np.full(n, s % 15, np.int32))
    frames = env.render_batch()
    assert tuple(frames.shape) == (n, 120, 200, 3)
    if output == "torch":
        assert frames.is_cuda
        frames = frames.cpu().numpy()
    else:
        assert isinstance(frames, np.ndarray)
    assert np.array_equal(frames, np.stack([env.render(index=k) for k in range(n)]))
    some = env.render_batch([4, 1])
    some = some.cpu().numpy() if output == "torch" else some
    assert np.array_equal(some, frames[[4, 1]])
    env.close()
    plain = ProcgenGymVectorEnv("maze", 2)
    assert plain.render_batch() is None
    plain.close()
