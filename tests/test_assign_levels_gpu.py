"""Assigned levels (include/procgen2_vec.h pgv_assign_levels), the GPU half: the HIP engine against the reference model
of tests/assign_util.py (held to the oracle by tests/test_assign_levels.py), bit for bit, through the Python surface
(ProcgenVecEnv.assign_levels / level_numbers / level_known) and the C ABI.
"""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

from assign_util import GAME_STEPS, AssignModel, actions_of, run_schedule, scheduled_level
from oracle_util import OBS_BYTES, assert_same_dump, register_textures
from test_levels import _fresh_make_obs

pytestmark = pytest.mark.gpu

NO_PREFETCH = 256  # pgv_set_debug bit 8
PREFETCHING = ("coinrun", "maze", "climber", "caveflyer", "jumper")


class Engine:
    """ProcgenVecEnv driven with host arrays, as the model is."""

    def __init__(self, game, n, seed_base=1, num_levels=0, start_level=0, debug=0):
        import torch
        from procgen2_amd.vec_env import ProcgenVecEnv
        self.torch = torch
        self.v = ProcgenVecEnv(game, n, seed_base=seed_base, num_levels=num_levels, start_level=start_level)
        self.n = n
        if debug:
            assert self.v.L.pgv_set_debug(self.v._h, debug) == 0
        self.generator_launches = lambda: self.v.L.pgv_generator_launches(self.v._h)

    def _out(self):
        v = self.v
        return (v.obs.reshape(self.n, OBS_BYTES).cpu().numpy(), v.reward.cpu().numpy(), v.done.cpu().numpy())

    def reset(self, mask=None, seeds=None):
        self.v.reset(mask=mask, seeds=seeds)
        return self._out()[0]

    def step(self, actions):
        self.v.step(self.torch.as_tensor(np.asarray(actions, np.int32)))
        return self._out()

    def assign(self, indices, levels):
        self.v.assign_levels([int(x) for x in levels], None if indices is None else [int(i) for i in indices])

    def levels(self):
        v = self.v
        assert v.level_numbers.dtype == self.torch.uint32 and v.level_known.dtype == self.torch.uint8
        assert tuple(v.level_numbers.shape) == (self.n,) and tuple(v.level_known.shape) == (self.n,)
        return v.level_numbers.view(self.torch.int32).cpu().numpy().view(np.uint32), v.level_known.cpu().numpy()

    def state(self, e):
        from engine_util import _dump
        return _dump(lambda buf, m: self.v.L.pgv_dump_state(self.v._h, e, buf, m), ctypes.c_float, np.float32)

    def tiles(self, e):
        from engine_util import _dump
        return _dump(lambda buf, m: self.v.L.pgv_dump_tiles(self.v._h, e, buf, m), ctypes.c_uint8, np.uint8)

    def close(self):
        self.v.close()


class Pair:
    """The engine and the model side by side: one script drives both, check() holds the engine to the model."""

    def __init__(self, eng, model):
        self.eng, self.model = eng, model
        self.got = self.want = None

    def first_reset(self):
        """The engine's first reset; the model had it when it was made (as OracleVec has)."""
        self.got = (self.eng.reset(), None, None)
        self.want = (self.model.first_reset(), None, None)
        return self.want[0]

    def reset(self, mask=None, seeds=None):
        obs = self.eng.reset(mask=mask, seeds=seeds)
        self.model.reset(mask=mask, seeds=seeds)
        self.got = (obs, None, None)
        self.want = (self.model.obs, None, None)
        return self.want[0]

    def step(self, actions):
        self.got = self.eng.step(actions)
        self.want = self.model.step(actions)
        return self.want

    def assign(self, indices, levels):
        self.eng.assign(indices, levels)
        self.model.assign(indices, levels)

    def check(self, what):
        (oe, re_, de), (om, rm, dm) = self.got, self.want
        if de is not None:
            assert np.array_equal(de, dm), "done, " + what
            assert np.array_equal(re_.view(np.uint32), rm.view(np.uint32)), "reward bits, " + what
        numbers, known = self.eng.levels()
        assert np.array_equal(known, self.model.level_known), "level_known, %s: envs %s" % (what, np.nonzero(known != self.model.level_known)[0][:8])
        assert np.array_equal(numbers, self.model.level_numbers), "level_numbers, %s: envs %s" % (what, np.nonzero(numbers != self.model.level_numbers)[0][:8])
        if not np.array_equal(oe, om):
            bad = np.nonzero((oe != om).any(axis=1))[0]
            raise AssertionError("obs differ at %s in %d envs (first envs %s)" % (what, bad.size, bad[:8]))


# (prefetch on and off where the game prefetches)
LOCKSTEP = [(game, steps, num_levels, prefetch) for game, steps in GAME_STEPS for num_levels in (7, 0)
            for prefetch in (True, False) if prefetch or game in PREFETCHING]


@pytest.mark.parametrize("game,steps,num_levels,prefetch", LOCKSTEP)
def test_engine_with_assignments_matches_the_model(game, steps, num_levels, prefetch):
    """Lock-step against the model: assignments right after a reset, in the step after `done` (the late path), overwritten
    before use, dropped by a reseeding reset; a third of the envs never named; a masked reset without seeds that consumes
    assignments.  Every step: obs bytes, reward bits, dones, level_numbers and level_known."""
    n = 96
    eng = Engine(game, n, seed_base=3, num_levels=num_levels, start_level=50, debug=0 if prefetch else NO_PREFETCH)
    numbers, known = eng.levels()  # valid from pgv_make on
    assert (known == (1 if num_levels else 0)).all() and (num_levels or (numbers == 0).all())
    model = AssignModel(game, n, seed_base=3, num_levels=num_levels, start_level=50)
    pair = Pair(eng, model)
    run_schedule(pair, pair.assign, steps, n, check=pair.check)
    for e in range(0, n, 12):
        assert_same_dump(eng.state(e), model.state(e), "state env %d" % e)
        assert_same_dump(eng.tiles(e), model.tiles(e), "tiles env %d" % e)
    print("\n%s num_levels=%d prefetch=%s: %d assigned levels installed by explicit resets, %d by auto-resets"
          % (game, num_levels, prefetch, model.assigned_by_reset, model.assigned_by_auto))
    assert model.assigned_by_reset >= 1
    if game in ("maze", "bossfight", "chaser"):
        assert model.assigned_by_auto >= 8
    eng.close()
    model.close()


@pytest.mark.parametrize("game,steps", [("maze", 300), ("coinrun", 300), ("chaser", 200)])
@pytest.mark.parametrize("num_levels", [0, 7])
def test_the_moment_of_an_assignment_does_not_show(game, steps, num_levels):
    """Two engines, the same level for every episode of every env.  One hears of an episode's level right after the reset
    before it and has its stream drained every step — the generator's side stream has rebuilt the slot long before the
    level is due; the other hears of it in the step before the reset is due — the install finds the slot not ready and the
    level is generated inside the step; a third as the second, without prefetch.  Equal frames, every step."""
    n = 128
    runs = []
    for when, debug in (("early", 0), ("late", 0), ("late", NO_PREFETCH)):
        if debug and game not in PREFETCHING:
            continue
        eng = Engine(game, n, seed_base=3, num_levels=num_levels, start_level=50, debug=debug)
        episode = [0] * n
        everyone = list(range(n))
        trace = [eng.reset().copy()]
        if when == "early":
            eng.assign(everyone, [scheduled_level(e, 1) for e in everyone])
        pending = np.zeros(n, bool)
        for s in range(steps):
            obs, reward, done = eng.step(actions_of(s, n))
            numbers, known = eng.levels()
            trace.append((obs.copy(), reward.copy(), done.copy(), numbers, known))
            fresh = [e for e in everyone if pending[e]]
            pending = done.astype(bool)
            ended = [e for e in everyone if pending[e]]
            for e in fresh:
                episode[e] += 1
            if when == "early" and fresh:
                eng.assign(fresh, [scheduled_level(e, episode[e] + 1) for e in fresh])
                eng.torch.cuda.synchronize()  # (the whole device: the generator's side stream too)
            if when == "late" and ended:
                eng.assign(ended, [scheduled_level(e, episode[e] + 1) for e in ended])
        runs.append((when, debug, trace, sum(episode)))
        eng.close()
    assert runs[0][3] >= 8, "episodes ended: %d" % runs[0][3]
    for when, debug, trace, _ in runs[1:]:
        assert np.array_equal(trace[0], runs[0][2][0]), "first reset"
        for s, (a, b) in enumerate(zip(trace[1:], runs[0][2][1:])):
            for x, y, what in zip(a, b, ("obs", "reward", "done", "level_numbers", "level_known")):
                assert np.array_equal(x, y), "%s differs at step %d (%s, debug %d)" % (what, s, when, debug)


@pytest.mark.parametrize("game", ["maze", "bossfight"])
@pytest.mark.parametrize("num_levels", [0, 7])
def test_a_pending_assignment_travels_in_records_and_snapshots(game, num_levels):
    """save_envs of an env that holds a pending assignment, load_envs into a slot of an engine of another size and seed:
    both go on identically through the assigned level and the one after.  The same through save_state / load_state."""
    import torch
    src = Engine(game, 8, seed_base=3, num_levels=num_levels, start_level=50)
    dst = Engine(game, 5, seed_base=77, num_levels=num_levels, start_level=50)
    src.reset()
    dst.reset()
    for s in range(7):
        src.step(actions_of(s, 8))
    for s in range(4):  # (a step counter of the other parity)
        dst.step(actions_of(s + 100, 5))
    src.assign([2, 5], [4242, 77])
    records = src.v.save_envs([2])
    dst.v.load_envs(records, [4])
    snap = src.v.save_state()
    resets, was_done, numbers_seen = 0, False, []
    tail = []
    for s in range(7, 1300):
        a = actions_of(s, 8)
        b = np.zeros(5, np.int32)
        b[4] = a[2]
        os_, rs, ds = src.step(a)
        od, rd, dd = dst.step(b)
        ns, ks = src.levels()
        nd, kd = dst.levels()
        tail.append((a, os_.copy(), rs.copy(), ds.copy(), ns, ks))
        assert ds[2] == dd[4] and rs[2:3].view(np.uint32) == rd[4:5].view(np.uint32), s
        assert np.array_equal(os_[2], od[4]), "obs, step %d" % s
        assert (ns[2], ks[2]) == (nd[4], kd[4]), s
        if was_done:
            resets += 1
            numbers_seen.append((int(ns[2]), int(ks[2])))
        was_done = bool(ds[2])
        if resets >= 2 and len(tail) >= 40:
            break
    assert resets >= 2, "the env did not get through two episodes"
    assert numbers_seen[0] == (4242, 1), numbers_seen
    assert numbers_seen[1][1] == (1 if num_levels else 0) and numbers_seen[1][0] != 4242
    dst.close()
    # the whole batch, into a fresh engine (snapshots load into an engine of the same size and shard)
    other = Engine(game, 8, seed_base=1234, num_levels=num_levels, start_level=50)
    other.v.load_state(snap)
    for k, (a, o, r, d, nums, known) in enumerate(tail):
        o2, r2, d2 = other.step(a)
        n2, k2 = other.levels()
        assert np.array_equal(d, d2) and np.array_equal(r.view(np.uint32), r2.view(np.uint32)) and np.array_equal(o, o2), k
        assert np.array_equal(nums, n2) and np.array_equal(known, k2), k
    # a snapshot of the layout before this one (its magic) is refused, and so are records under any other tag (the record
    # layout version is one of the words the tag is mixed from)
    from procgen2_amd.lib import EngineError
    old = snap.copy()
    assert old[:4].tobytes() == b"5NGP"
    old[0] = ord("4")
    with pytest.raises(EngineError):
        other.v.load_state(old)
    stale = type(records)(records.data, records.tag ^ 1)
    with pytest.raises(EngineError):
        other.v.load_envs(stale, [0])
    assert torch.equal(other.v.save_envs([0]).data, other.v.save_envs([0]).data)
    other.close()
    src.close()


@pytest.mark.parametrize("game", ["coinrun", "caveflyer", "jumper"])
@pytest.mark.parametrize("built_ahead", [True, False])
def test_a_reseeding_reset_that_drops_an_assignment_finds_the_envs_own_chain(game, built_ahead):
    """Free mode with prefetch.  Envs with a history of levels of their own are assigned a level; built_ahead: the device is
    drained, so the side stream has built every assigned level on a fresh chain (fresh containers) before the reset WITH
    seeds comes that drops the assignments — otherwise the reset follows at once.  Either way the reset and the levels
    after it are what the model's env gives, whose containers went on from its own history: the assigned numbers range
    over few levels while the histories differ, so fresh and continued containers are both among them."""
    n = 48
    eng = Engine(game, n, seed_base=3)
    model = AssignModel(game, n, seed_base=3)
    pair = Pair(eng, model)
    pair.first_reset()
    pair.check("first reset")
    for k in range(2):
        pair.reset()
        pair.check("reset %d of the envs' own history" % k)
    pair.assign(list(range(n)), [1000 + e % 5 for e in range(n)])
    if built_ahead:
        eng.torch.cuda.synchronize()
    pair.reset(seeds=np.arange(n, dtype=np.int32) % 7 + 20)
    pair.check("reseeding reset")
    assert (eng.levels()[1] == 0).all() and model.assigned_by_reset == 0
    for k in range(3):
        pair.reset()
        pair.check("reset %d after the reseeding reset" % k)
    for e in range(0, n, 12):
        assert_same_dump(eng.state(e), model.state(e), "state env %d" % e)
    eng.close()
    model.close()


def test_every_finished_env_assigned_from_a_table_on_the_device_at_scale():
    """4096 free-mode maze envs, 505 steps (mazes time out at 500): every finished env is assigned a level from a 200-level
    table, on the device, without a host synchronisation in the assignment; every reset frame is the oracle's fresh make
    of the number level_numbers reports."""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n = 4096
    register_textures("maze")
    v = ProcgenVecEnv("maze", n, seed_base=1)
    v.reset()
    gen = torch.Generator(device=v.device)
    gen.manual_seed(5)
    table = torch.arange(3000, 3200, device=v.device, dtype=torch.int64)
    everyone = torch.arange(n, device=v.device, dtype=torch.int32)
    nobody = torch.full((n,), -1, device=v.device, dtype=torch.int32)
    frames = {}
    pending = np.zeros(n, bool)
    checked = 0
    for s in range(505):
        obs, _, done = v.step_synthetic(2)
        # (an index outside the batch is skipped: the envs that did not finish are named -1, and nothing waits for a count)
        v.assign_levels(table[torch.randint(0, 200, (n,), device=v.device, generator=gen)], torch.where(done != 0, everyone, nobody))
        if pending.any():
            rows = torch.as_tensor(np.nonzero(pending)[0], device=v.device)
            got = obs.reshape(n, OBS_BYTES)[rows].cpu().numpy()
            numbers = v.level_numbers.view(torch.int32)[rows].cpu().numpy().view(np.uint32)
            assert (v.level_known[rows] == 1).all(), s
            for row, number in zip(got, numbers):
                assert 3000 <= number < 3200
                if int(number) not in frames:
                    frames[int(number)] = _fresh_make_obs("maze", int(number))
                assert np.array_equal(row, frames[int(number)]), (s, int(number))
            checked += int(pending.sum())
        pending = done.cpu().numpy().astype(bool)
    assert checked >= n
    assert len(frames) > 150, "levels seen: %d" % len(frames)
    v.close()


def test_assign_levels_arguments():
    from procgen2_amd import lib as pglib
    for num_levels in (0, 7):
        eng = Engine("maze", 16, seed_base=2, num_levels=num_levels, start_level=50)
        L, h = eng.v.L, eng.v._h
        first = eng.reset().copy()
        levels = np.array([5, 6, 7, 8], np.int32)
        idx = np.array([3, 99, -1, 16], np.int32)  # one env of the batch, three indices outside it
        assert L.pgv_assign_levels(h, None, 0, None) == 0 and L.pgv_assign_levels_host(h, None, 0, None) == 0
        assert L.pgv_assign_levels(h, None, -1, None) != 0 and b"negative" in L.pgv_last_error()
        assert L.pgv_assign_levels(h, None, 4, None) != 0 and b"NULL" in L.pgv_last_error()
        assert L.pgv_assign_levels_host(h, None, -1, levels.ctypes.data_as(c_void_p)) != 0 and b"negative" in L.pgv_last_error()
        assert L.pgv_assign_levels_host(h, idx.ctypes.data_as(c_void_p), 4, None) != 0 and b"NULL" in L.pgv_last_error()
        assert L.pgv_assign_levels(None, None, 0, None) != 0
        assert L.pgv_level_numbers(None) is None and L.pgv_level_known(None) is None
        pglib.check(L, L.pgv_assign_levels_host(h, idx.ctypes.data_as(c_void_p), 4, levels.ctypes.data_as(c_void_p)), "pgv_assign_levels_host")
        with pytest.raises(ValueError):
            eng.v.assign_levels([1, 2, 3])  # no indices: one level per env
        with pytest.raises(ValueError):
            eng.v.assign_levels([1, 2, 3], [0, 1])
        eng.v.assign_levels([], [])
        # an engine that never assigns: known everywhere in level-seed mode, nowhere in free mode
        numbers, known = eng.levels()
        assert (known == (1 if num_levels else 0)).all()
        obs = eng.reset()  # consumes env 3's assignment; the indices outside the batch named nobody
        numbers, known = eng.levels()
        assert known[3] == 1 and numbers[3] == 5 and np.array_equal(obs[3], _fresh_make_obs("maze", 5))
        others = np.arange(16) != 3
        assert (known[others] == (1 if num_levels else 0)).all()
        if not num_levels:
            assert (numbers[others] == 0).all()
        # duplicates: one of them wins
        eng.assign([7, 7, 7], [21, 22, 23])
        eng.reset(mask=(np.arange(16) == 7).astype(np.uint8))
        numbers, known = eng.levels()
        assert known[7] == 1 and numbers[7] in (21, 22, 23)
        assert first.shape == obs.shape
        eng.close()
