"""Every path of every distribution-mode variant against the oracle (need an MI355X).

A game's source is compiled once per distribution mode, and the variants are different kernels: other world sides, cell
indices that need a second byte, draw lists of another width, Level / GenLds / composer grids of another size.  Here every
one of the 18 (game, mode) pairs runs its default path AND every alternate path behind pgv_set_debug — the paths the engine
falls back to on its own for fat frames, levels not ready in time, the last words of a random stream, a rejected range draw
— side by side on one oracle run, each engine held to the oracle itself, bit for bit: dones, reward bit patterns and every
observation byte after every step, the frames masked resets return, state and tile dumps at the wavefronts' edges.

The batch is ragged on purpose (variant_paths_util.py): 131 envs leave a partial gang, a partial wavefront and a partial
pre-pass group.  tests/test_variant_paths.py asserts on the oracle alone that every case serves auto-resets and that the maze
cases run into the step cap together.
"""
import numpy as np
import pytest

import variant_paths_util as vp
from engine_util import EngineVec
from oracle_util import OracleVec, assert_same_dump
from test_modes import CHASER_STATE_FLOATS, NON_DEFAULT
from test_parity_gpu import _host_threads

pytestmark = pytest.mark.gpu


def _engines(game, n, mode, paths):
    engines = []
    for debug in paths:
        eng = EngineVec(game, n, seed_base=vp.SEED_BASE, mode=mode)
        assert eng.L.pgv_mode(eng.h) == mode
        if debug:
            eng.set_debug(debug)
        engines.append((vp.PATH_NAMES[debug], eng))
    return engines


def _same_frames(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("%s: obs differ in %d envs (first env %d, %d bytes)" %
                             (what, bad.size, bad[0], int((got[bad[0]] != want[bad[0]]).sum())))


def _same_rows(name, eng, a, s, obs, reward, done):
    oe, re_, de = eng.step(a)
    what = "%s, step %d" % (name, s)
    if not np.array_equal(de, done):
        raise AssertionError("%s: done differs, first env %d" % (what, np.nonzero(de != done)[0][0]))
    if not np.array_equal(re_.view(np.uint32), reward.view(np.uint32)):
        raise AssertionError("%s: reward bits differ, first env %d" % (what, np.nonzero(re_.view(np.uint32) != reward.view(np.uint32))[0][0]))
    _same_frames(oe, obs, what)


def _same_dumps(name, eng, ora, envs, s, floats=None):
    for e in envs:
        assert_same_dump(eng.state(e), ora.state(e), "%s, step %d: state of env %d" % (name, s, e))
        assert_same_dump(eng.tiles(e), ora.tiles(e), "%s, step %d: tiles of env %d" % (name, s, e))
        assert floats is None or eng.state(e).size == floats, (name, s, e)


@pytest.mark.parametrize("game,mode", vp.PAIRS)
def test_every_path_matches_the_oracle(game, mode):
    engines = _engines(game, vp.N, mode, vp.paths(game))
    floats = CHASER_STATE_FLOATS[mode] if game == "chaser" else None
    dumps = vp.dump_after(game, mode)

    def each_step(s, ora, a, obs, reward, done):
        for name, eng in engines:
            _same_rows(name, eng, a, s, obs, reward, done)
            if s in dumps:
                _same_dumps(name, eng, ora, vp.DUMP_ENVS, s, floats)

    def each_reset(s, ora, mask, seeds, obs):
        for name, eng in engines:
            _same_frames(eng.reset(mask=mask, seeds=seeds), obs, "%s, masked reset after step %d" % (name, s))

    def at_start(ora):
        for name, eng in engines:
            _same_frames(eng.reset(), ora.reset_obs(), "%s, first reset" % name)

    try:
        ends, cap_ends = vp.run_on_oracle(game, mode, each_step, each_reset, at_start, render=True, threads=_host_threads())
        vp.assert_covers(game, mode, ends, cap_ends)
    finally:
        for _, eng in engines:
            eng.close()


@pytest.mark.parametrize("n", vp.SMALL_NS)
@pytest.mark.parametrize("game,mode", NON_DEFAULT)
def test_variants_at_one_and_65_envs(game, mode, n):
    """A one-env engine of a variant, and 65 envs — one env in a second wavefront: the default path and the complete render
    path against the oracle, 80 steps with one unseeded masked reset of env 0 after step 40."""
    engines = _engines(game, n, mode, vp.SMALL_PATHS)
    ora = OracleVec(game, n, seed_base=vp.SEED_BASE, mode=mode)
    try:
        for name, eng in engines:
            _same_frames(eng.reset(), ora.reset_obs(), "%s, first reset" % name)
        mask = (np.arange(n) == 0).astype(np.uint8)
        for s in range(vp.SMALL_STEPS):
            a = vp.actions(s, n)
            obs, reward, done = ora.step(a)
            for name, eng in engines:
                _same_rows(name, eng, a, s, obs, reward, done)
            if s == vp.SMALL_RESET_AFTER:
                obs = ora.reset(mask=mask)
                for name, eng in engines:
                    _same_frames(eng.reset(mask=mask), obs, "%s, masked reset after step %d" % (name, s))
        for name, eng in engines:
            _same_dumps(name, eng, ora, sorted({0, n - 1}), vp.SMALL_STEPS - 1)
    finally:
        ora.close()
        for _, eng in engines:
            eng.close()
