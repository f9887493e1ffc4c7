"""Replays what bench.py --dump-outputs wrote on the CPU oracle, row by row (tests/test_bench_outputs_gpu.py; its own
tests in tests/test_bench_replay.py).

A dump holds what the last step of a bench run handed its caller, as float32: obs.npy of the envs at
bench.dump_rows(envs, DUMP_OBS_ENVS), reward.npy and done.npy of those at dump_rows(envs, DUMP_SCALAR_ENVS).  An env's
inputs depend on its global index alone (seed 1 + index, the device action hash with run_seed 0), so every dumped
observation row is replayed by itself: an OracleVec of that one env (made = bench's one reset()), the run's steps with
synthetic actions, drawn at the last one only (drawing does not feed back into the game).
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from ctypes import c_void_p

import numpy as np

from oracle_util import OracleVec, register_textures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mixed_blocks(envs):
    """bench.py --workload mixed on one GPU: each game's block of the slab as (game, first row, count), in
    vec_env.GAMES order, envs // 7 each and the last game taking the remainder.  (Rank r's envs of a game sit at global
    indices r * count + i; bench.py itself is left as it is, so it keeps its own copy of this arithmetic.)"""
    from procgen2_amd.vec_env import GAMES
    base = envs // len(GAMES)
    blocks, at = [], 0
    for k, game in enumerate(GAMES):
        count = base if k < len(GAMES) - 1 else envs - base * (len(GAMES) - 1)
        blocks.append((game, at, count))
        at += count
    return blocks


def row_env(workload, envs, row):
    """(game, global env index) of slab row `row` of a one-GPU bench run: `workload` is a game or "mixed"."""
    if workload != "mixed":
        return workload, row
    for game, at, count in mixed_blocks(envs):
        if at <= row < at + count:
            return game, row - at
    raise IndexError("row %d of a %d-env slab" % (row, envs))


def replay_row(game, mode, index, steps, run_seed=0):
    """Env `index` of a bench run `steps` steps after its reset: (obs u8 [12288], reward f32, done u8, episode ends)."""
    ora = OracleVec(game, 1, seed_base=1, env_offset=index, mode=mode)
    ora.set_render(False)
    ends = np.zeros(1, np.int32)
    ora.L.pgo_vec_run(ora.h, steps - 1, run_seed, index, ends.ctypes.data_as(c_void_p))
    ora.set_render(True)
    obs, reward, done = ora.step(None, run_seed=run_seed)
    out = obs[0].copy(), reward[0], done[0], int(ends[0]) + int(done[0])
    ora.close()
    return out


def check_dump(directory, workload, envs, steps, mode=None, threads=None):
    """Every dumped observation row of a one-GPU bench run of `workload` (a game or "mixed"; `mode` a distribution mode
    name or None) with `envs` envs, `steps` steps after the reset (settle + max(1, warmup) + steps), against the oracle:
    the frame byte for byte, the reward by bit pattern, the done flag.  Raises AssertionError naming the first rows
    that differ; returns (rows replayed, rows whose episode ended at least once on the way)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from procgen2_amd import lib as pglib
    assert steps >= 1, steps
    obs, reward, done = (np.load(os.path.join(directory, name + ".npy")) for name in ("obs", "reward", "done"))
    rows, scalar_rows = bench.dump_rows(envs, bench.DUMP_OBS_ENVS), bench.dump_rows(envs, bench.DUMP_SCALAR_ENVS)
    assert obs.dtype == reward.dtype == done.dtype == np.float32
    assert obs.shape == (rows.size, 64, 64, 3), ("obs.npy", obs.shape, "rows", rows.size)
    assert reward.shape == done.shape == (scalar_rows.size,), ("reward.npy / done.npy", reward.shape, done.shape)
    pixels = obs.astype(np.uint8).reshape(rows.size, -1)
    assert np.array_equal(pixels.reshape(obs.shape).astype(np.float32), obs), "obs.npy holds values that are not bytes"
    at = np.searchsorted(scalar_rows, rows)
    assert np.array_equal(scalar_rows[at], rows), "the reward and done of an observed env were not dumped"
    where = [row_env(workload, envs, int(r)) for r in rows]
    for game in sorted({g for g, _ in where}):
        register_textures(game)  # here, before the threads make their envs
    mode_id = pglib.mode_id(mode)
    with ThreadPoolExecutor(threads or bench.usable_cores()) as pool:
        got = list(pool.map(lambda w: replay_row(w[0], mode_id, w[1], steps), where))
    bad, ended = [], 0
    for k, ((game, index), (o, r, d, ends)) in enumerate(zip(where, got)):
        what = []
        if not np.array_equal(pixels[k], o):
            what.append("obs (%d bytes)" % int((pixels[k] != o).sum()))
        if reward[at[k]].view(np.uint32) != np.float32(r).view(np.uint32):
            what.append("reward %r, oracle %r" % (float(reward[at[k]]), float(r)))
        if done[at[k]] != float(d):
            what.append("done %r, oracle %d" % (float(done[at[k]]), int(d)))
        if what:
            bad.append("row %d (%s env %d): %s" % (rows[k], game, index, ", ".join(what)))
        ended += ends > 0
    assert not bad, "%s: %d of %d dumped rows differ from the oracle %d steps after the reset; %s" % (
        workload if mode is None else "%s %s" % (workload, mode), len(bad), rows.size, steps, "; ".join(bad[:4]))
    return rows.size, ended
