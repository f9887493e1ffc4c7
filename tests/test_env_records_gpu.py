"""Per-env state records (pgv_save_envs / pgv_load_envs, include/procgen2_vec.h) held to the CPU oracle.

The oracle has no notion of a record and needs none: an env's trajectory is a function of its seed and its actions, so
the oracle plays the plain, unpermuted run and every engine slot is held to whichever oracle env it now contains.  All
engines get EXPLICIT actions whose values are the synthetic ones of the plain run, A[t][i] = pgo_synthetic_action(RUN_SEED,
t, env_offset + i): slot p that holds oracle env i is given A[t][i].  With test_snapshot's N, SEED_BASE and RUN_SEED the
oracle's run is the one that file plans on, so the moments at which records are taken (P0 … P4) are its `snapshot_plan`,
chosen by the oracle alone, and `_check_plan` keeps them from being vacuous.

One oracle run a case serves three engines side by side (the oracle, with drawing on, is what a case costs):
  A  shuffles its whole batch at every moment (record p into slot (37 p + 11) mod 200) and stays on the oracle;
  S  only saves; at every moment 77 of its envs — chosen from the oracle's dones — go into foreign engines B of 77 envs;
  R  (ten cases) rewinds: saves at P1 and P3, plays 51 / 52 steps, loads the records back and replays them.
"""
import time
from ctypes import c_void_p

import numpy as np
import pytest

from oracle_util import OracleVec, assert_same_dump
from test_env_records import FOREIGN_N, PARTIAL, REWIND_IDS, chosen_envs
from test_snapshot import (CASES, FOREIGN_RUN_SEED, FOREIGN_SEED, N, RUN_SEED, SEED_BASE, Case, _actions, _check_plan,
                           _host_threads, _same_outputs, oracle_dones, snapshot_plan)

from procgen2_amd import lib as pglib

pytestmark = pytest.mark.gpu


def _engine(game, n, **kw):
    from engine_util import EngineVec

    class RecordsEngine(EngineVec):
        """EngineVec plus the record calls, through the host-pointer entry points."""

        @property
        def record_bytes(self):
            return int(self.L.pgv_env_record_bytes(self.h))

        @property
        def tag(self):
            return int(self.L.pgv_env_record_tag(self.h))

        def save_envs(self, indices=None, count=None):
            idx = None if indices is None else np.ascontiguousarray(indices, np.int32)
            count = (self.n if idx is None else idx.size) if count is None else count
            out = np.full((count, self.record_bytes), 0xA5, np.uint8)
            pglib.check(self.L, self.L.pgv_save_envs_host(self.h, None if idx is None else idx.ctypes.data_as(c_void_p), count,
                                                          out.ctypes.data_as(c_void_p)), "pgv_save_envs_host")
            return out

        def load_envs(self, records, indices=None, tag=None):
            records = np.ascontiguousarray(records, np.uint8)
            idx = None if indices is None else np.ascontiguousarray(indices, np.int32)
            assert idx is None or idx.size == records.shape[0]
            pglib.check(self.L, self.L.pgv_load_envs_host(self.h, None if idx is None else idx.ctypes.data_as(c_void_p),
                                                          records.shape[0], records.ctypes.data_as(c_void_p),
                                                          self.tag if tag is None else tag), "pgv_load_envs_host")

    return RecordsEngine(game, n, **kw)


def _foreign(case, n, steps, fresh=False, **over):
    """An engine of the case's configuration that belongs to another rollout (test_snapshot._foreign_engine), of another
    size and shard: another seed_base and env_offset, reset and stepped `steps` times with other actions — or fresh, as a
    new process has it: never reset, never stepped."""
    cfg = dict(case.config())
    cfg["env_offset"] = case.env_offset + 4096
    cfg.update(over)
    eng = _engine(case.game, n, seed_base=FOREIGN_SEED, **cfg)
    if not fresh:
        eng.reset()
        for _ in range(steps):
            eng.step_quiet(run_seed=FOREIGN_RUN_SEED)
    return eng


def _rows(want, envs):
    return want[0][envs], want[1][envs], want[2][envs]


def _same_states(tag, eng, slots, ora, envs):
    for slot, env in zip(slots, envs):
        assert_same_dump(eng.state(int(slot)), ora.state(int(env)), "%s: state of slot %d (oracle env %d)" % (tag, slot, env))
        assert_same_dump(eng.tiles(int(slot)), ora.tiles(int(env)), "%s: tiles of slot %d (oracle env %d)" % (tag, slot, env))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_records_stay_on_the_oracle(case):
    """Shuffle (A), part of a batch into foreign engines of another size (S → B, with B′ for the slots nobody loads into)
    and rewind (R), every byte of every step to the end of the run; see the module's docstring.

    B at a moment: 77 envs, another env_offset; its step counter has the parity of S's at P1 (38 foreign steps), the other
    one at P2 (freshly made: counter 0, never reset) — 37 foreign steps otherwise.  The 77 source envs: those whose episode
    ended in the moment's step (their reset is pending), then those that end later, then the lowest-numbered rest
    (test_env_records.chosen_envs); the first chosen env goes into slot 76.  At P1, P2 (and maze's P4) all 77 are loaded; at
    P0 and P3 the first 40, and B's slots 0 … 36 must go on as B′'s — the same foreign history, nothing loaded."""
    n = N
    dones = oracle_dones(case)
    plan = snapshot_plan(case, dones)
    _check_plan(case, dones, plan)
    threads = _host_threads()
    rewinds = case.id in REWIND_IDS
    A = _engine(case.game, n, seed_base=SEED_BASE, **case.config())
    S = _engine(case.game, n, seed_base=SEED_BASE, **case.config())
    R = _engine(case.game, n, seed_base=SEED_BASE, **case.config()) if rewinds else None
    ora = OracleVec(case.game, n, seed_base=SEED_BASE, **case.config())
    L = ora.L
    holds = np.arange(n)                  # holds[p]: the oracle env in A's slot p
    perm = (37 * np.arange(n) + 11) % n   # record p goes into slot perm[p]
    assert len(set(perm)) == n and (perm != np.arange(n)).all()
    followers = []                        # (tag, B, slots, envs, B′ or None)
    windows = []                          # R: [first step after the save, length, records, [(actions, outputs)]]

    def moment(s, want):
        nonlocal holds
        names = plan[s]
        tag = "%s %s (after step %d)" % (case.id, "+".join(names), s)
        # -- A: the whole batch, shuffled
        rec = A.save_envs()
        assert np.array_equal(A.save_envs(), rec), tag + ": a second save at once differs from the first"
        assert (rec[:, :4].view(np.uint32) != 0).all(), tag + ": a saved record is marked empty"
        A.load_envs(rec, perm)
        moved = np.empty_like(holds)
        moved[perm] = holds
        holds = moved
        _same_outputs(tag + ", A right after the shuffle", A._fetch(), _rows(want, holds))
        slots = np.arange(0, n, 25)
        _same_states(tag + ", A after the shuffle", A, slots, ora, holds[slots])
        # -- S → B: 77 chosen envs into foreign engines
        chosen = chosen_envs(dones, s, FOREIGN_N)
        assert dones[s + 1:, chosen].any(), tag + ": none of the chosen envs ends an episode later"
        kinds = ([FOREIGN_N] if {"P1", "P2", "P4"} & set(names) else []) + ([PARTIAL] if {"P0", "P3"} & set(names) else [])
        for loaded in kinds:
            fresh, steps = "P2" in names, 38 if "P1" in names else 37
            B = _foreign(case, FOREIGN_N, steps, fresh)
            twin = _foreign(case, FOREIGN_N, steps, fresh) if loaded < FOREIGN_N else None
            envs = chosen[:loaded]
            into = FOREIGN_N - 1 - np.arange(loaded)
            rec = S.save_envs(envs)
            if s >= 0:
                assert int((rec[:, 4] & 1).sum()) == int(dones[s][envs].sum()), tag + ": pending resets in the records"
            B.load_envs(rec, into)
            btag = "%s, B (%d loaded)" % (tag, loaded)
            _same_outputs(btag + " right after the load", _rows(B._fetch(), into), _rows(want, envs))
            _same_states(btag + " after the load", B, into[::10], ora, envs[::10])
            if twin is not None:
                rest = np.arange(FOREIGN_N - loaded)
                _same_outputs(btag + ": the slots nobody loaded into", _rows(B._fetch(), rest), _rows(twin._fetch(), rest))
            followers.append((btag, B, into, envs, twin))
        # -- R: save for a rewind
        if rewinds and ("P1" in names or "P3" in names):
            length = 51 if "P1" in names else 52
            assert dones[s + 1:s + 1 + length].any(), tag + ": no episode ends inside the replayed window"
            windows.append([s + 1, length, R.save_envs(), []])

    everyone = [("A", A), ("S", S)] + ([("R", R)] if rewinds else [])
    want = None
    for name, v in everyone:
        _same_outputs("%s %s reset" % (case.id, name), (v.reset(), v.reward, v.done), (ora.reset_obs(), ora.reward, ora.done))
    if -1 in plan:
        moment(-1, (ora.obs, ora.reward, ora.done))
    for s in range(case.steps):
        a = _actions(L, RUN_SEED, s, n, case.env_offset)
        want = ora.step(a, threads=threads)
        assert np.array_equal(want[2], dones[s]), "the oracle's own plan run differs at step %d" % s
        _same_outputs("%s A step %d" % (case.id, s), A.step(a[holds]), _rows(want, holds))
        _same_outputs("%s S step %d" % (case.id, s), S.step(a), want)
        if rewinds:
            _same_outputs("%s R step %d" % (case.id, s), R.step(a), want)
        for btag, B, into, envs, twin in followers:
            b = a[:FOREIGN_N].copy()
            b[into] = a[envs]
            got = B.step(b)
            _same_outputs("%s, step %d" % (btag, s), _rows(got, into), _rows(want, envs))
            if twin is not None:
                rest = np.arange(FOREIGN_N - into.size)
                _same_outputs("%s, step %d: the slots nobody loaded into" % (btag, s), _rows(got, rest), _rows(twin.step(b), rest))
        for w in windows:
            if w[0] <= s < w[0] + w[1]:
                w[3].append((a, tuple(x.copy() for x in want)))
            if s == w[0] + w[1] - 1:  # back to the save (R's counter is 51 / 52 further), and the same steps again
                R.load_envs(w[2])
                for k, (ak, wk) in enumerate(w[3]):
                    _same_outputs("%s R replays step %d of the window from step %d" % (case.id, k, w[0]), R.step(ak), wk)
                w[3] = None
        if s in plan:
            moment(s, want)
    assert not rewinds or (len(windows) >= 1 and all(w[3] is None for w in windows)), "a window was not replayed"
    slots = np.arange(0, n, 25)
    _same_states(case.id + " A at the end", A, slots, ora, holds[slots])
    _same_states(case.id + " S at the end", S, slots, ora, slots)
    for btag, B, into, envs, twin in followers:
        _same_states(btag + " at the end", B, into[::10], ora, envs[::10])
        B.close()
        if twin is not None:
            twin.close()
    for _, v in everyone:
        v.close()
    ora.close()


@pytest.mark.parametrize("count", [1, 63, 65, 129])
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("game", ["bossfight", "chaser"])
def test_records_at_sizes_around_a_wavefront(game, n, count):
    """The code that brings the random streams home takes a wavefront per 64 envs, the record kernels a workgroup per 64
    records.  After steps 61 and 150 `count` records with source indices k mod n (repeats where count > n) go into slots
    0 … count − 1 of a foreign engine of 130 envs; slot k is held to oracle env k mod n for the rest of 260 steps."""
    case = Case(game)
    A = _engine(game, n, seed_base=SEED_BASE)
    ora = OracleVec(game, n, seed_base=SEED_BASE)
    L = ora.L
    src = np.arange(count) % n
    _same_outputs("reset", (A.reset(), A.reward, A.done), (ora.reset_obs(), ora.reward, ora.done))
    followers = []
    for s in range(260):
        a = _actions(L, RUN_SEED, s, n)
        want = ora.step(a)
        _same_outputs("%s n=%d A step %d" % (game, n, s), A.step(a), want)
        for at, B in followers:
            b = np.zeros(130, np.int32)
            b[:count] = a[src]
            _same_outputs("%s n=%d count=%d B of step %d, step %d" % (game, n, count, at, s), _rows(B.step(b), np.arange(count)),
                          _rows(want, src))
        if s in (61, 150):
            rec = A.save_envs(src)
            B = _foreign(case, 130, 37)
            followers.append((s, B))
            B.load_envs(rec)
            _same_outputs("%s n=%d count=%d right after the load at step %d" % (game, n, count, s),
                          _rows(B._fetch(), np.arange(count)), _rows(want, src))
            ks = sorted({0, count // 2, count - 1})
            _same_states("after the load at step %d" % s, B, ks, ora, [k % n for k in ks])
    for _, B in followers:
        B.close()
    A.close()
    ora.close()


@pytest.mark.parametrize("game", ["coinrun", "chaser", "bossfight"])
def test_records_at_full_size(game, capsys):
    """65 536 envs, records in device memory (torch tensors).  T never saves; S saves all its envs after steps 60 and 150 and
    loads the second set rotated by 12 345 slots.  Both are then stepped 100 times with explicit actions — S's rotated
    with its envs — and agree on every reward and done of every step and on every observation byte after 50 and 100
    steps.  (T at this size is what test_every_env_at_full_size_matches_the_oracle holds to the oracle.)"""
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv
    n, shift = 65536, 12345
    T, S = ProcgenVecEnv(game, n, seed_base=1), ProcgenVecEnv(game, n, seed_base=1)
    T.reset()
    S.reset()
    rec, took_save = None, 0.0
    for s in range(151):
        T.step_synthetic(RUN_SEED)
        S.step_synthetic(RUN_SEED)
        if s in (60, 150):
            rec = None  # (one set of records in device memory at a time)
            torch.cuda.synchronize()
            t0 = time.time()
            rec = S.save_envs()
            torch.cuda.synchronize()
            took_save = time.time() - t0
    into = (torch.arange(n, device=S.device, dtype=torch.int32) + shift) % n
    torch.cuda.synchronize()
    t0 = time.time()
    S.load_envs(rec, into)
    torch.cuda.synchronize()
    took_load = time.time() - t0
    with capsys.disabled():
        print("\n%s: pgv_env_record_bytes = %d, %d records = %.1f MB, saved in %.4f s, loaded in %.4f s (wall, with the host's sync)"
              % (game, S.env_record_bytes, n, rec.data.numel() / 1e6, took_save, took_load))
    del rec

    def same(tag, obs=False):
        torch.cuda.synchronize()
        assert torch.equal(torch.roll(S.done, -shift), T.done), tag + ": done"
        assert torch.equal(torch.roll(S.reward, -shift).view(torch.int32), T.reward.view(torch.int32)), tag + ": reward bits"
        if obs:
            assert torch.equal(torch.roll(S.obs, -shift, 0), T.obs), tag + ": obs"

    same("%s right after the load" % game, obs=True)
    gen = torch.Generator(device="cpu").manual_seed(5)
    ends = 0
    for s in range(100):
        a = torch.randint(0, 15, (n,), generator=gen, dtype=torch.int32).to(T.device)
        T.step(a)
        S.step(torch.roll(a, shift))
        same("%s step %d after the load" % (game, s), obs=s in (49, 99))
        ends += int(T.done.sum())
    assert ends > 1000, ends
    T.close()
    S.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals and edges
# ---------------------------------------------------------------------------------------------------------------------
def _twins(game, n, seed_base, steps, run_seed, **cfg):
    out = []
    for _ in range(2):
        v = _engine(game, n, seed_base=seed_base, **cfg)
        v.reset()
        for _ in range(steps):
            v.step_quiet(run_seed=run_seed)
        out.append(v)
    return out


@pytest.mark.parametrize("what", ["tag", "mode", "num_levels"])
def test_refused_records_leave_the_engine_untouched(what):
    """A wrong tag, records of mode "easy" offered to a default engine, records of num_levels = 7 offered to num_levels = 0:
    refused with a message, and the engine's whole-batch snapshot is the same bytes before and after."""
    base = dict(mode=0, num_levels=0)
    other = dict(base, **{"tag": {}, "mode": {"mode": 1}, "num_levels": {"num_levels": 7}}[what])
    src = _engine("coinrun", 40, seed_base=5, **other)
    src.reset()
    for _ in range(25):
        src.step_quiet(run_seed=2)
    rec, tag = src.save_envs(), src.tag
    eng, twin = _twins("coinrun", 48, 8, 10, 6, **base)
    if what == "tag":
        assert tag == eng.tag and src.record_bytes == eng.record_bytes, "size and tag do not depend on num_envs or the seed"
        tag ^= 1
    else:
        assert tag != eng.tag and tag != 0
    before = eng.save_state()
    with pytest.raises(pglib.EngineError, match="another configuration"):
        eng.load_envs(rec, tag=tag)
    assert np.array_equal(eng.save_state(), before)
    src.close()
    for s in range(20):
        _same_outputs("step %d after the refusal" % s, eng.step(None, run_seed=6), twin.step(None, run_seed=6))
    eng.close()
    twin.close()


@pytest.mark.parametrize("game", ["coinrun", "chaser"])
def test_record_edges(game):
    """Indices outside the batch (save: an empty record; load: skipped), a zero-filled buffer (loads nothing), count = 0,
    a negative count and a NULL buffer (refused): after all of it the engine is as its twin; then a load of two records
    beside an empty one changes exactly those two slots, and the other 68 go on as the twin's for 40 steps."""
    n = 70
    eng, twin = _twins(game, n, 8, 12, 6)
    src = _engine(game, 30, seed_base=5)
    src.reset()
    for _ in range(25):
        src.step_quiet(run_seed=2)
    rec = src.save_envs([3, -1, 30, 7, 2 ** 31 - 1, -2 ** 31])
    assert list(rec[:, :4].view(np.uint32)[:, 0] != 0) == [True, False, False, True, False, False]
    assert not rec[[1, 2, 4, 5]].any(), "an empty record is written out, as zeros"
    eng.load_envs(rec[[1, 2]], [5, 6])                             # empty records
    eng.load_envs(np.zeros((n, eng.record_bytes), np.uint8))        # a zero-filled buffer
    eng.load_envs(rec[[0, 3, 0]], [-1, n, 2 ** 31 - 1])             # good records, indices outside the batch
    assert eng.L.pgv_save_envs_host(eng.h, None, 0, None) == 0 and eng.L.pgv_load_envs_host(eng.h, None, 0, None, eng.tag) == 0
    assert eng.L.pgv_save_envs(eng.h, None, 0, None) == 0 and eng.L.pgv_load_envs(eng.h, None, 0, None, eng.tag) == 0
    assert eng.L.pgv_save_envs_host(eng.h, None, -1, rec.ctypes.data_as(c_void_p)) != 0 and b"negative" in eng.L.pgv_last_error()
    assert eng.L.pgv_load_envs_host(eng.h, None, 3, None, eng.tag) != 0 and b"NULL" in eng.L.pgv_last_error()
    _same_outputs("after loads that load nothing", eng._fetch(), twin._fetch())
    for e in range(0, n, 9):
        assert_same_dump(eng.state(e), twin.state(e), "state env %d after loads that load nothing" % e)
    # … and a real load of two records beside a skipped one changes exactly those two slots
    eng.load_envs(rec[[0, 1, 3]], [10, 11, 12])
    got, want = eng._fetch(), twin._fetch()
    keep = np.setdiff1d(np.arange(n), [10, 12])
    _same_outputs("the slots not named by the load", _rows(got, keep), _rows(want, keep))
    _same_outputs("the loaded slots", _rows(got, [10, 12]), _rows(src._fetch(), [3, 7]))
    for s in range(40):  # (device-made actions hash the slot, not the env: the twin's slots get the same ones)
        _same_outputs("step %d after the load: the slots not named by it" % s, _rows(eng.step(None, run_seed=6), keep),
                      _rows(twin.step(None, run_seed=6), keep))
    for v in (eng, twin, src):
        v.close()


@pytest.mark.parametrize("where", ["source", "destination"])
@pytest.mark.parametrize("game", ["coinrun", "maze", "jumper"])
def test_records_between_engines_with_and_without_level_prefetch(game, where):
    """pgv_set_debug bit 8 (every reset generates its level inside the step) on the source only, on the destination only:
    the prefetch slots travel as they are, and either engine serves them — still on the oracle, through auto-resets."""
    n, steps, at = 64, 330, 120
    case = Case(game)
    dones = oracle_dones(case, n=n)
    assert dones[at + 1:steps].any(), "an episode must end after the records move"
    A = _engine(game, n, seed_base=SEED_BASE)
    B = _foreign(case, n, 37)
    (A if where == "source" else B).set_debug(1 << 8)
    ora = OracleVec(game, n, seed_base=SEED_BASE)
    _same_outputs("reset", (A.reset(), A.reward, A.done), (ora.reset_obs(), ora.reward, ora.done))
    back = np.arange(n)[::-1].copy()
    for s in range(steps):
        a = _actions(ora.L, RUN_SEED, s, n)
        want = ora.step(a)
        _same_outputs("%s A step %d" % (game, s), A.step(a), want)
        if s > at:
            _same_outputs("%s B step %d" % (game, s), B.step(a[back]), _rows(want, back))
        if s == at:
            B.load_envs(A.save_envs(), back)  # env i into slot n − 1 − i
            _same_outputs("%s B right after the load" % game, B._fetch(), _rows(want, back))
    for v in (A, B, ora):
        v.close()


# ---------------------------------------------------------------------------------------------------------------------
# the torch path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["coinrun", "chaser", "bossfight"])
def test_vec_env_fork_on_a_side_stream(game):
    """ProcgenVecEnv.save_envs / load_envs / fork with the caller on a stream of its own and no torch.cuda.synchronize()
    between save, load and step: env 0 forked into every other slot, then every slot stepped with the same actions — all N
    observation rows stay equal, and equal the oracle's for that env.  Then records[idx] and a load under other indices."""
    import torch
    from procgen2_amd.vec_env import EnvRecords, ProcgenVecEnv
    n, before, after = 96, 40, 60
    ora = OracleVec(game, n, seed_base=SEED_BASE)
    L = ora.L
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = ProcgenVecEnv(game, n, seed_base=SEED_BASE)
        assert env.env_record_bytes % 16 == 0 and env.env_record_tag != 0
        env.reset()
        ora.reset_obs()
        for s in range(before):
            a = _actions(L, RUN_SEED, s, n)
            ora.step(a)
            env.step(torch.from_numpy(a))
        rec = env.fork(torch.zeros(n - 1, dtype=torch.int32), torch.arange(1, n))
        assert isinstance(rec, EnvRecords) and tuple(rec.data.shape) == (n - 1, env.env_record_bytes) and rec.tag == env.env_record_tag
        rows = []
        for s in range(before, before + after):
            a = _actions(L, RUN_SEED, s, n)
            obs, reward, done = env.step(torch.full((n,), int(a[0]), dtype=torch.int32))
            rows.append((obs.clone(), reward.clone(), done.clone(), tuple(x[0].copy() for x in ora.step(a))))
        # records[idx]: the records of envs 5 and 9 (copies of env 0 as it is NOW) put aside, the batch reset, and those
        # two loaded under other indices, out of order
        later = env.save_envs()[torch.tensor([9, 5])]
        assert later.tag == rec.tag and len(later) == 2 and len(env.save_envs()[3:7]) == 4
        env.reset()
        env.load_envs(later, [70, 2])
        obs = env.obs.clone()
    side.synchronize()
    for k, (obs_k, reward_k, done_k, (oo, ro, do)) in enumerate(rows):
        obs_k = obs_k.cpu().numpy().reshape(n, -1)
        assert (obs_k == oo[None, :]).all(), "obs, step %d after the fork" % k
        assert (reward_k.cpu().numpy().view(np.uint32) == ro.view(np.uint32)).all() and (done_k.cpu().numpy() == do).all(), k
    obs = obs.cpu().numpy().reshape(n, -1)
    assert np.array_equal(obs[70], rows[-1][3][0]) and np.array_equal(obs[2], rows[-1][3][0])
    with pytest.raises(ValueError):
        env.load_envs(later, [1, 2, 3])
    env.close()
    ora.close()
