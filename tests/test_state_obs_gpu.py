"""Symbolic observations on the device (include/procgen2_vec.h pgv_state_rows / pgv_tile_rows), held bit for bit to the
oracle's dumps: every game and mode, any indices, behind steps, resets, same-step auto-resets and frameless sequences."""
from ctypes import c_float, c_uint8, c_void_p

import numpy as np
import pytest

from engine_util import _dump
from episodes_util import SAME_STEP, EpisodeModel, synthetic_actions
from oracle_util import OracleVec
from state_obs_util import (GAMES, MODE_NAMES, N, NON_DEFAULT, RUN_SEED, SEED_BASE, STEPS, VARIABLE, Sample, assert_rows,
                            oracle_run)

from procgen2_amd import lib as pglib

pytestmark = pytest.mark.gpu


def make(game, n=N, **kw):
    from procgen2_amd.vec_env import ProcgenVecEnv
    env = ProcgenVecEnv(game, n, seed_base=SEED_BASE, **kw)
    env.reset()
    return env


def observe(env, envs=None):
    rows, lengths = env.state_obs(envs)
    tiles = env.tile_obs(envs)
    return rows.cpu().numpy(), lengths.cpu().numpy(), tiles.cpu().numpy()


def assert_matches(env, sample, what):
    rows, lengths, tiles = observe(env)
    assert_rows(rows, lengths, tiles, sample.states, sample.tiles, what)
    return set(int(x) for x in lengths)


@pytest.mark.parametrize("game", GAMES)
def test_parity_with_the_oracle(game):
    at, first_done = oracle_run(game)
    env = make(game)
    seen = set()
    for s in range(STEPS + 1):
        if s:
            env.step_synthetic(RUN_SEED)
        if s in at:
            seen |= assert_matches(env, at[s], "%s step %d" % (game, s))
    env.close()
    assert first_done is not None and first_done < max(at), "no episode ended before the last check"
    if game in VARIABLE:
        assert len(seen) >= 2, "an easy run: every row has length %s" % seen


@pytest.mark.parametrize("game,mode", NON_DEFAULT, ids=["%s-%s" % (g, MODE_NAMES[m]) for g, m in NON_DEFAULT])
def test_every_other_mode(game, mode):
    at, _ = oracle_run(game, mode, N, 64, 32)
    env = make(game, distribution_mode=mode)
    assert pglib.MODES[env.distribution_mode] == mode
    for s in range(64 + 1):
        if s:
            env.step_synthetic(RUN_SEED)
        if s in at:
            assert_matches(env, at[s], "%s mode %d step %d" % (game, mode, s))
    env.close()


@pytest.mark.parametrize("game", ["chaser", "maze", "coinrun"])  # rows of 573 / 10 / 194 floats, tile rows of 121 / 625 / 4096 bytes
def test_indices(game):
    import torch
    env = make(game)
    for _ in range(8):
        env.step_synthetic(RUN_SEED)
    all_rows, all_lengths, all_tiles = observe(env)
    idx = np.random.default_rng(3).integers(0, N, size=150).astype(np.int64)  # with repeats; three groups of rows
    outside = {0: -1, 63: N, 64: 2 ** 31 - 1, 149: -(2 ** 31)}
    for k, v in outside.items():
        idx[k] = v
    count, width, cells = idx.size, env.state_layout.width, env.state_layout.cells
    # one more row than asked for, filled with a canary
    rows = torch.full((count + 1, width), float("nan"), dtype=torch.float32, device=env.device)
    lengths = torch.full((count + 1,), -7, dtype=torch.int32, device=env.device)
    tiles = torch.full((count + 1, cells), 0xAB, dtype=torch.uint8, device=env.device)
    canary = rows[count].clone()
    got_rows, got_lengths = env.state_obs(idx.astype(np.int32), out=rows[:count], lengths_out=lengths[:count])
    got_tiles = env.tile_obs(idx.astype(np.int32), out=tiles[:count])
    assert got_rows.data_ptr() == rows.data_ptr() and got_tiles.data_ptr() == tiles.data_ptr()
    r, l, t = rows.cpu().numpy().view(np.uint32), lengths.cpu().numpy(), tiles.cpu().numpy()
    for k in range(count):
        if k in outside:
            assert not r[k].any() and l[k] == 0 and not t[k].any(), k
        else:
            assert np.array_equal(r[k], all_rows[idx[k]].view(np.uint32)) and l[k] == all_lengths[idx[k]], k
            assert np.array_equal(t[k], all_tiles[idx[k]]), k
    assert np.array_equal(r[count], canary.cpu().numpy().view(np.uint32)) and l[count] == -7 and (t[count] == 0xAB).all()

    # count == 0 succeeds and writes nothing; a misaligned output is refused with nothing written
    L, h = env.L, env._h
    rows.fill_(float("nan")), tiles.fill_(0xAB)
    torch.cuda.synchronize()
    assert L.pgv_state_rows(h, None, 0, c_void_p(rows.data_ptr()), None) == 0
    assert L.pgv_tile_rows(h, None, 0, c_void_p(tiles.data_ptr())) == 0
    assert L.pgv_state_rows(h, None, 2, c_void_p(rows.data_ptr() + 4), None) != 0
    assert b"aligned" in L.pgv_last_error()
    assert L.pgv_tile_rows(h, None, 2, c_void_p(tiles.data_ptr() + 1)) != 0
    assert b"aligned" in L.pgv_last_error()
    assert L.pgv_state_rows(h, None, -1, c_void_p(rows.data_ptr()), None) != 0
    assert L.pgv_state_rows(h, None, 2, None, None) != 0 and L.pgv_tile_rows(h, None, 2, None) != 0
    env.sync()
    assert torch.isnan(rows).all() and (tiles == 0xAB).all()
    env.close()


@pytest.mark.parametrize("game", ["coinrun", "chaser"])  # double-buffered entity tables; random streams in two buffers
def test_the_calls_change_nothing(game):
    import torch
    watched, plain = make(game), make(game)
    for s in range(32):
        a = watched.step_synthetic(RUN_SEED)
        b = plain.step_synthetic(RUN_SEED)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (game, s)
        first = watched.state_obs()[0].clone(), watched.state_obs()[1].clone(), watched.tile_obs().clone()
        second = watched.state_obs() + (watched.tile_obs(),)
        for x, y in zip(first, second):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (game, s)
    watched.close(), plain.close()


@pytest.mark.parametrize("game", GAMES)
def test_taps_and_host_forms_against_the_device_rows(game):
    """The parity taps pgv_dump_state / pgv_dump_tiles and the host-pointer forms give what the device rows hold, bit for
    bit, on both sides of the row kernel's group boundaries and for the last env; and the taps keep their contract: the
    full length whatever cap is, exactly min(cap, length) items written, -1 for an index outside the batch, 0 for
    bossfight's tiles."""
    env = make(game)
    for _ in range(24):
        env.step_synthetic(RUN_SEED)
    rows, lengths, tiles = observe(env)
    env.sync()
    L, h = env.L, env._h
    sampled = np.array([0, 1, 17, 63, 64, 65, 100, N - 1], np.int32)
    for e in (int(x) for x in sampled):
        st = _dump(lambda buf, m: L.pgv_dump_state(h, e, buf, m), c_float, np.float32)
        tl = _dump(lambda buf, m: L.pgv_dump_tiles(h, e, buf, m), c_uint8, np.uint8)
        assert lengths[e] == st.size and np.array_equal(rows[e, :st.size].view(np.uint32), st.view(np.uint32)), (game, e)
        assert tiles.shape[1] == tl.size and np.array_equal(tiles[e], tl), (game, e)
        # a short cap: the full length comes back, cap items are written, the canary behind them stays; cap 0 writes nothing
        for tap, ctype, whole, canary in ((L.pgv_dump_state, c_float, st, 7.5), (L.pgv_dump_tiles, c_uint8, tl, 0xAB)):
            for cap in (0, 3, whole.size - 1):
                if cap < 0 or cap >= whole.size:
                    continue  # (bossfight has no tiles to cut short)
                buf = (ctype * (whole.size + 1))(*([canary] * (whole.size + 1)))
                assert tap(h, e, buf, cap) == whole.size, (game, e, cap)
                got = np.array(buf[:], whole.dtype)
                assert np.array_equal(got[:cap].view(np.uint8), whole[:cap].view(np.uint8)), (game, e, cap)
                assert (got[cap:] == canary).all(), (game, e, cap)
    one_f, one_b = (c_float * 1)(7.5), (c_uint8 * 1)(0xAB)
    for outside in (-1, N):
        assert L.pgv_dump_state(h, outside, one_f, 1) == -1 and L.pgv_dump_tiles(h, outside, one_b, 1) == -1, (game, outside)
    assert one_f[0] == 7.5 and one_b[0] == 0xAB
    if game == "bossfight":
        assert L.pgv_dump_tiles(h, 0, one_b, 1) == 0 and one_b[0] == 0xAB
    # the host-pointer forms: the same rows for the sampled envs (uploaded indices), with and without the lengths, and for
    # the first envs under NULL indices; unaligned host buffers are fine
    lay = env.state_layout
    k = sampled.size
    raw = np.full(k * lay.width + 1, np.nan, np.float32)
    h_rows, h_lengths = raw[1:].reshape(k, lay.width), np.full(k, -7, np.int32)
    h_tiles = np.full((k, lay.cells), 0xAB, np.uint8)
    ptr = lambda x: c_void_p(x.ctypes.data)
    assert L.pgv_state_rows_host(h, ptr(sampled), k, ptr(h_rows), ptr(h_lengths)) == 0, L.pgv_last_error()
    assert L.pgv_tile_rows_host(h, ptr(sampled), k, ptr(h_tiles) if lay.cells else None) == 0, L.pgv_last_error()
    assert np.array_equal(h_rows.view(np.uint32), rows[sampled].view(np.uint32)) and np.array_equal(h_lengths, lengths[sampled])
    assert np.array_equal(h_tiles, tiles[sampled]) and np.isnan(raw[0])
    h_rows[:] = np.nan
    assert L.pgv_state_rows_host(h, None, k, ptr(h_rows), None) == 0, L.pgv_last_error()
    assert np.array_equal(h_rows.view(np.uint32), rows[:k].view(np.uint32))
    assert L.pgv_state_rows_host(h, None, 0, None, None) == 0 and L.pgv_tile_rows_host(h, None, 0, None) == 0
    assert L.pgv_state_rows_host(h, None, 1, None, None) != 0 and L.pgv_state_rows_host(h, None, -1, ptr(h_rows), None) != 0
    if lay.cells:
        h_tiles[:] = 0xAB
        assert L.pgv_tile_rows_host(h, None, k, ptr(h_tiles)) == 0 and np.array_equal(h_tiles, tiles[:k])
        assert L.pgv_tile_rows_host(h, None, 1, None) != 0
    env.close()


@pytest.mark.parametrize("game", GAMES)
def test_without_frames(game):
    n = 65
    env = make(game, n)
    o = OracleVec(game, n, seed_base=SEED_BASE, render=True)
    o.set_render(False)
    for call in range(4):
        env.step_sequence(steps=5, frames="none", run_seed=RUN_SEED)
        for _ in range(5):
            o.step(None, run_seed=RUN_SEED)
        rows, lengths, tiles = observe(env)
        want = Sample(o)
        assert_rows(rows, lengths, tiles, want.states, want.tiles, "%s call %d" % (game, call))
    env.close(), o.close()


@pytest.mark.parametrize("game", ["maze", "bossfight"])
def test_same_step_episodes(game):
    import torch
    n, limit = 65, 20
    env = make(game, n, autoreset_mode="same_step", max_episode_steps=limit)
    model = EpisodeModel(game, n, SAME_STEP, limit, 0, seed_base=SEED_BASE, render=False)
    model.first_reset()
    ended = 0
    for t in range(48):
        a = synthetic_actions(RUN_SEED, t, n)
        _, ep = env.step_episodes(torch.as_tensor(a))
        model.step(a)
        ended += int(model.ended.sum())
        rows, lengths, tiles = observe(env)
        want = Sample(model.o)
        assert_rows(rows, lengths, tiles, want.states, want.tiles, "%s step %d" % (game, t))
    assert ended >= n  # (the limit alone ends every env's episode twice)
    env.close(), model.close()


@pytest.mark.parametrize("game", ["coinrun", "chaser", "jumper"])
def test_fork(game):
    env = make(game, 16)
    for _ in range(10):
        env.step_synthetic(RUN_SEED)
    a, b = 3, 9
    rows, lengths, tiles = observe(env, [a, b])
    assert not np.array_equal(tiles[0], tiles[1]) or not np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32))
    env.fork([a], [b])
    rows2, lengths2, tiles2 = observe(env, [a, b])
    assert np.array_equal(rows2[0].view(np.uint32), rows2[1].view(np.uint32)) and lengths2[0] == lengths2[1]
    assert np.array_equal(tiles2[0], tiles2[1])
    assert np.array_equal(rows2[0].view(np.uint32), rows[0].view(np.uint32)) and np.array_equal(tiles2[0], tiles[0])
    env.close()


@pytest.mark.parametrize("game", ["climber", "bossfight"])
def test_python_surface(game):
    import torch
    from procgen2_amd.gym_vector import ProcgenGymVectorEnv
    n = 9
    env = make(game, n)
    lay = env.state_layout
    assert lay == pglib.state_layout(env.L, game, env.distribution_mode) == pglib.state_layout(env.L, game)
    assert len(lay.fixed_names) == lay.fixed and len(lay.record_names) == lay.record
    rows, lengths = env.state_obs()
    tiles = env.tile_obs()
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (n, lay.width) and rows.device == env.device
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (n,) and lengths.device == env.device
    assert tiles.dtype == torch.uint8 and tuple(tiles.shape) == (n, lay.cells) and tiles.device == env.device
    assert (lay.cells == 0) == (game == "bossfight")
    assert tuple(env.state_obs([])[0].shape) == (0, lay.width) and tuple(env.tile_obs([4, 4]).shape) == (2, lay.cells)
    out, lengths_out = torch.full_like(rows, 7.0), torch.full_like(lengths, 7)
    back = env.state_obs(out=out, lengths_out=lengths_out)
    assert back[0] is out and back[1] is lengths_out and torch.equal(out, rows) and torch.equal(lengths_out, lengths)
    with pytest.raises(ValueError):
        env.state_obs(out=torch.zeros((n, lay.width + 1), dtype=torch.float32, device=env.device))
    with pytest.raises(ValueError):
        env.tile_obs(out=torch.zeros((n, lay.cells), dtype=torch.int32, device=env.device))
    env.close()

    for output in ("torch", "numpy"):
        gym = ProcgenGymVectorEnv(game, n, seed=SEED_BASE, output=output, state_info=True)
        _, info = gym.reset()
        for step in range(3):
            want_rows, want_lengths = gym.engine.state_obs()
            want_tiles = gym.engine.tile_obs()
            assert ("tiles" in info) == (lay.cells > 0)
            assert np.array_equal(np.asarray(torch.as_tensor(info["state"]).cpu()).view(np.uint32), want_rows.cpu().numpy().view(np.uint32))
            assert np.array_equal(np.asarray(torch.as_tensor(info["state_length"]).cpu()), want_lengths.cpu().numpy())
            if lay.cells:
                assert np.array_equal(np.asarray(torch.as_tensor(info["tiles"]).cpu()), want_tiles.cpu().numpy())
            _, _, _, _, info = gym.step(np.full(n, step % 15, np.int64))
        gym.close()
        plain = ProcgenGymVectorEnv(game, n, seed=SEED_BASE, output=output)
        assert plain.reset()[1] == {}
        plain.close()
        # episodes="device": the step is one engine call with info entries of its own; the state entries ride along
        for mode in ("next_step", "same_step"):
            gym = ProcgenGymVectorEnv(game, n, seed=SEED_BASE, output=output, state_info=True, episodes="device", autoreset_mode=mode,
                                      max_episode_steps=2 if mode == "same_step" else 0, final_obs_capacity=4)
            _, info = gym.reset()
            for step in range(4):  # (same_step: every env is truncated and reset on steps 2 and 4 — the rows are the new episode's)
                want_rows, want_lengths = gym.engine.state_obs()
                assert ("tiles" in info) == (lay.cells > 0)
                assert np.array_equal(np.asarray(torch.as_tensor(info["state"]).cpu()).view(np.uint32), want_rows.cpu().numpy().view(np.uint32))
                assert np.array_equal(np.asarray(torch.as_tensor(info["state_length"]).cpu()), want_lengths.cpu().numpy())
                if lay.cells:
                    assert np.array_equal(np.asarray(torch.as_tensor(info["tiles"]).cpu()), gym.engine.tile_obs().cpu().numpy())
                _, _, _, _, info = gym.step(np.full(n, step % 15, np.int64))
                assert "_final_obs" in info and "episode" in info
            gym.close()
