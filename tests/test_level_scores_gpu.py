"""Level replay scores (include/procgen2_vec.h pgv_level_scores_enable) on the GPU: the level ring's law, the update against a
plain numpy loop over the ring's own views, and the refusals.  maze, levels 5 .. 7, N = 70: a workgroup of 64 envs and one of 6.
L = 2R + 3 rows, T = L + 2 slots, 54 calls, so the first stretch lies over slot 0.  Capacities 1024 and 1025: the last that goes
through the workgroups' own tables and the first that does not.  The score's bound: fix() is off by at most 2^-17 a step, so is
the mean; the sum's conversion, the division and the product by 2^-16 (exact) are at most two float32 ulps more."""
import ctypes

import numpy as np
import pytest
import torch

from episodes_util import synthetic_actions
from history_util import RUN_SEED
from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import ProcgenVecEnv

pytestmark = pytest.mark.gpu

N, R = pglib.LEVEL_SCORE_ENVS + 6, pglib.LEVEL_SCORE_ROWS
L, L2 = 2 * R + 3, R + 1
T, CALLS = L + 2, 54
FIRST_LEVEL, MASK = 5, 6
CAPACITIES = [pglib.LEVEL_SCORE_LDS_LEVELS, pglib.LEVEL_SCORE_LDS_LEVELS + 1]
CUSTOM_ENVS, CUSTOM_IDS = [3, 10, 65, 69], [900, 5000, 6, FIRST_LEVEL + CAPACITIES[0]]  # inside, outside, a seeded level's, the bound's
MODES = {"next_step": {}, "same_step": dict(max_episode_steps=7)}
f32 = np.float32
SIGNAL = np.random.default_rng(31).standard_normal((L, N)).astype(f32)


def make(mode, capacity, n=N, slots=T):
    return ProcgenVecEnv("maze", n, seed_base=1, num_levels=3, start_level=FIRST_LEVEL, autoreset_mode=mode, history=dict(capacity=slots, gray=True),
                         transitions=True, level_scores=dict(first_level=FIRST_LEVEL, capacity=capacity, known=("seeded", "custom")), **MODES[mode])


@pytest.mark.parametrize("mode", list(MODES))
def test_the_ring_holds_the_level_words_of_every_push(mode):
    v = make(mode, 3)
    ls = v.level_scores
    assert not ls.level_known.any() and not ls.level.any()  # "no level" before the first push

    def newest_is_now():
        slot = (v.history.head - 1) % T
        assert torch.equal(ls.level[slot], v.level_numbers.view(torch.int32)) and torch.equal(ls.level_known[slot], v.level_known), v.history.head
    v.reset()
    newest_is_now()
    for t in range(40):
        v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, N)))
        newest_is_now()
        if t == 17:
            before = ls.level.clone()
            v.assign_levels(np.full(len(range(0, N, 3)), 6, np.int32), indices=np.arange(0, N, 3))  # what the named envs build at the reset
            v.reset(mask=(np.arange(N) % 3 == 0).astype(np.uint8))  # their words change, nobody else's
            newest_is_now()
            slot = (v.history.head - 1) % T
            assert bool((ls.level[slot][0::3] == 6).all()) and torch.equal(ls.level[slot][1::3], before[slot][1::3])
    v.close()


@pytest.fixture(scope="module", params=[(m, k) for m in MODES for k in CAPACITIES], ids=lambda p: "%s-%d" % p)
def run(request):
    """(engine, the ring's views as numpy, capacity) after 54 calls with one install of caller-made levels behind call 30."""
    mode, capacity = request.param
    v = make(mode, capacity)
    v.reset()
    for t in range(CALLS):
        v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, N)))
        if t == 30:
            status = v.set_levels(v.get_levels(envs=CUSTOM_ENVS), ids=CUSTOM_IDS, indices=CUSTOM_ENVS)
            assert not status.any()
    ls, tr = v.level_scores, v.transitions
    tr.reward[:, 1::2] -= 0.75  # (maze pays nothing below 0: every second env's returns are negative, zero or positive)
    ring = [x.cpu().numpy() for x in (tr.flags, tr.reward, v.history.began, ls.level, ls.level_known)]
    ring[3] = ring[3].view(np.uint32)
    rows = (v.history.head - 1 - L + np.arange(L)) % T
    assert (ring[4][rows] == 2).any() and (ring[0][rows] & (pglib.TR_VOID if mode == "next_step" else pglib.TR_TRUNCATED)).any()
    yield v, ring, capacity, mode
    v.close()


def reference(ring, first, signal, kind, partial, capacity):
    """The header's points 4 to 6, per env and per row: {k: [sum, steps, segments, max_return, the float64 sum of the signal]}."""
    flags, reward, began, level, known = ring
    v = np.abs(signal) if kind == "abs" else np.where(signal > 0, signal, f32(0))
    fix = np.rint(v * f32(65536)).astype(np.int64)
    out = {}
    for i in range(N):
        seg = None  # [level, known, whole, sum, steps, ret, raw]
        for t in range(len(signal) + 1):  # (the row behind the stretch stands for "not live")
            s, s1 = (first + t) % T, (first + t + 1) % T
            fl = int(flags[s, i]) if t < len(signal) else 0
            live = bool(fl & pglib.TR_RECORDED) and not fl & pglib.TR_VOID
            complete = live and bool(fl & (pglib.TR_TERMINATED | pglib.TR_TRUNCATED))
            if live and seg is None:
                seg = [level[s, i], known[s, i], began[s, i] != 0, 0, 0, f32(0), 0.0]
            if live:
                seg[3], seg[4], seg[5], seg[6] = seg[3] + int(fix[t, i]), seg[4] + 1, seg[5] + reward[s, i], seg[6] + float(v[t, i])
            if seg is None or (live and not complete and not began[s1, i]):
                continue
            k = (int(seg[0]) - FIRST_LEVEL) % 2 ** 32
            if (complete or partial) and (MASK >> int(seg[1])) & 1 and k < capacity:
                e = out.setdefault(k, [0, 0, 0, f32(-np.inf), 0.0])
                e[0], e[1], e[2], e[4] = e[0] + seg[3], e[1] + seg[4], e[2] + 1, e[4] + seg[6]
                e[3] = max(e[3], seg[5]) if complete and seg[2] else e[3]
            seg = None
    return out


@pytest.mark.parametrize("partial", [True, False])
@pytest.mark.parametrize("kind", ["abs", "positive"])
def test_update_is_the_loop(run, kind, partial):
    v, ring, K, mode = run
    ls, head = v.level_scores, v.history.head
    ls.score.zero_(), ls.episodes.zero_(), ls.max_return.fill_(-np.inf), ls.stamp.fill_(-1)
    want = [np.zeros(K, f32), np.zeros(K, np.int32), np.full(K, -np.inf, f32), np.full(K, -1, np.int64)]
    for first, sig, alpha, stamp in ((head - 1 - L, SIGNAL, 1.0, None), (head - 1 - L2, SIGNAL[:L2] * f32(3), 0.25, 77)):
        ref = reference(ring, first, sig, kind, partial, K)
        assert ref and (alpha != 1.0 or not partial or (len(ref) >= 4 and 895 in ref and (CAPACITIES[0] in ref) == (K > CAPACITIES[0])))  # id 900; the bound's id
        for k, e in ref.items():  # the header's point 7
            m = (f32(e[0]) / f32(e[1])) * (f32(1) / f32(65536))
            want[0][k] = m if want[1][k] == 0 else ((f32(1) - f32(alpha)) * want[0][k]) + (f32(alpha) * m)
            want[1][k], want[2][k], want[3][k] = want[1][k] + e[2], max(want[2][k], e[3]), head if stamp is None else stamp
        segments, steps = v.level_scores_update(first, len(sig), sig, kind, alpha, partial, stamp, totals=True)
        got = [x.cpu().numpy() for x in (ls.score, ls.episodes, ls.max_return, ls.stamp)]
        assert (int(segments), int(steps)) == (sum(e[2] for e in ref.values()), sum(e[1] for e in ref.values()))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
        if alpha == 1.0:  # the rule, not the rounding
            assert mode != "same_step" or ((want[2] >= 0).any() and want[2][895] < 0 and np.isfinite(want[2][895]))  # whole episodes: the time limit's
            for k, e in ref.items():
                mean = e[4] / e[1]
                assert abs(float(got[0][k]) - mean) <= 2.0 ** -17 + 2 * float(np.spacing(f32(mean))), (k, got[0][k], mean)


@pytest.fixture(scope="module")
def small():
    v, plain = make("same_step", 8, n=4, slots=6), ProcgenVecEnv("maze", 4, seed_base=1, history=dict(capacity=6), transitions=True)
    v.reset()
    for t in range(4):
        v.step_episodes(torch.as_tensor(synthetic_actions(RUN_SEED, t, 4)))
    v.level_scores_update(1, 3, np.ones((3, 4), f32))
    yield v, plain, torch.ones(3 * 4 + 2, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    v.close(), plain.close()


REFUSALS = [("NULL", dict(null=True)), ("NULL", dict(enable=None)), ("struct_size", dict(size=32)), ("kind", dict(kind=2)), ("alpha", dict(alpha=1.5)), ("alpha", dict(alpha=-0.1)), ("alpha", dict(alpha=np.nan)),
            ("NULL", dict(signal=None)), ("aligned", dict(signal=2)), ("aligned", dict(totals=4)), ("length", dict(length=0)), ("held", dict(first=4)),
            ("held", dict(first=2, length=3)), ("held", dict(first=-2)), ("pgv_level_scores_enable", dict(plain=True)),
            ("already", dict(enable=(0, 8, 2))), ("capacity", dict(enable=(0, 0, 2), plain=True)), ("capacity", dict(enable=(0, (1 << 24) + 1, 2), plain=True)),
            ("known_mask", dict(enable=(0, 8, 0), plain=True)), ("known_mask", dict(enable=(0, 8, 3), plain=True)), ("known_mask", dict(enable=(0, 8, 8), plain=True))]


@pytest.mark.parametrize("word,case", REFUSALS)
def test_the_refusals(small, word, case):
    v, plain, signal, totals = small
    ls = v.level_scores
    before = [x.clone() for x in (ls.score, ls.episodes, ls.max_return, ls.stamp, ls.level)]
    env = plain if case.get("plain") else v
    if "enable" in case:
        cfg = case["enable"] and ctypes.byref(pglib.LevelScoresConfig(16, *case["enable"]))
        who, rc = "pgv_level_scores_enable", env.L.pgv_level_scores_enable(env._h, cfg)
    else:
        q = pglib.level_score_update(None if case.get("signal", 0) is None else signal.data_ptr() + case.get("signal", 0), case.get("kind", "abs"),
                                     case.get("alpha", 0.5), totals=totals.data_ptr() + case.get("totals", 0))
        q.struct_size = case.get("size", q.struct_size)
        who, rc = "pgv_level_scores_update", env.L.pgv_level_scores_update(env._h, case.get("first", 1), case.get("length", 1), None if case.get("null") else ctypes.byref(q))
    msg = env.L.pgv_last_error().decode()
    assert rc != 0 and who in msg and word in msg, msg
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (ls.score, ls.episodes, ls.max_return, ls.stamp, ls.level))) and plain.level_scores is None
