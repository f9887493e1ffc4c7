"""V-trace over the transition ring (include/procgen2_vec.h pgv_transitions_vtrace) on the GPU: the kernel against a plain
per-env loop in np.float32 over the ring tests/transitions_util.py keeps, bit for bit; against the published sums in float64;
against transition_gae (the GAE law); and the refusals.

N = 131: three tiles of 64 envs, the last of 3.  T = 40 slots and 58 calls, so every stretch first(L) .. lies over slot 0.
Measured on the float32 model alone (no kernel), over both runs, both sets of thresholds, with and without trunc_values, at
L = 2R + 5: its largest deviation from the float64 sums is 6.5e-7 in vs and 1.07e-6 in the advantages, at |vs| up to 4.6."""
import ctypes

import numpy as np
import pytest
import torch

from episodes_util import SAME_STEP, synthetic_actions
from history_util import N, RUN_SEED
from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import ProcgenVecEnv
from transitions_util import CUT, RECORDED, TERMINATED, TRUNCATED, VOID, TransitionsEpisodes, TransitionsVec

pytestmark = pytest.mark.gpu

R = pglib.VTRACE_ROWS
T, CALLS = 2 * R + 8, 58
LENGTHS = [1, R - 1, R, R + 1, 2 * R + 5]
BARS = [(1.0, 1.0, 1.0), (1.3, 0.8, 2.0)]
GAMMA, LAM, SCALE, CLIP = 0.99, 0.95, 0.37, 2.0
F64_BOUND = 4 * 1.07e-6  # four times what the float32 model itself is off by (above)
f32 = np.float32
rng = np.random.default_rng(23)
V = rng.standard_normal((2 * R + 6, N)).astype(f32)
RHO = np.exp(0.5 * rng.standard_normal((2 * R + 5, N))).astype(f32)
TV = rng.standard_normal((2 * R + 5, N)).astype(f32)


def first_of(L):
    return T - (L + 1) // 2


@pytest.fixture(scope="module", params=["maze", "bossfight"])
def run(request):
    """(engine, model) after 58 calls.  maze: same-step episodes with a limit of 7 (TERMINATED and TRUNCATED rows); bossfight:
    plain steps (VOID rows), a reset of every fourth env behind call 41 (CUT rows) and a push by hand as call 44 (not recorded)."""
    game = request.param
    more = dict(autoreset_mode=SAME_STEP, max_episode_steps=7) if game == "maze" else {}
    v = ProcgenVecEnv(game, N, seed_base=1, history=dict(capacity=T, gray=True), transitions=True, **more)
    m = TransitionsEpisodes(game, N, SAME_STEP, T, True, max_episode_steps=7) if game == "maze" else TransitionsVec(game, N, T, True)
    v.reset(), m.first_reset()
    for t in range(CALLS):
        a = synthetic_actions(RUN_SEED, t, N)
        if game == "maze":
            v.step_episodes(torch.as_tensor(a)), m.step(a)
        elif t == 44:
            v.history_push(), m.push()
        else:
            v.step(torch.as_tensor(a)), m.step(a)
            if t == 41:
                mask = (np.arange(N) % 4 == 0).astype(np.uint8)
                v.reset(mask=mask), m.reset(mask)
    assert np.array_equal(v.transitions.flags.cpu().numpy(), m.tr.flags) and np.array_equal(v.history.began.cpu().numpy(), m.ring.began)
    assert (np.abs(m.tr.reward) == 10).any() and (m.tr.reward == 0).any()  # one clips at 0.37 and 2.0, the other does not
    yield v, m
    v.close(), m.close()


def rows_of(tr, first, L):
    """(dead, ends, reward) [L, N] of the stretch, from the model's ring."""
    h = tr.h
    s, s1 = (first + np.arange(L)) % h.T, (first + 1 + np.arange(L)) % h.T
    fl = tr.flags[s]
    dead = ((fl & RECORDED) == 0) | ((fl & VOID) != 0)
    own = fl & (TERMINATED | TRUNCATED)
    return dead, np.where((own == 0) & (h.began[s1] != 0), CUT, own), tr.reward[s]


def model_f32(tr, L, bars, tv):
    """The header's point 6, per env and per row, every operation one np.float32 rounding."""
    dead, ends, reward = rows_of(tr, first_of(L), L)
    g, lam, scale, clip, (rho_bar, c_bar, pg_bar) = f32(GAMMA), f32(LAM), f32(SCALE), f32(CLIP), map(f32, bars)
    vs, pg = np.zeros((L, N), f32), np.zeros((L, N), f32)
    for i in range(N):
        carry, nxt = f32(0), V[L, i]
        for t in range(L - 1, -1, -1):
            v, e, w = V[t, i], ends[t, i], RHO[t, i]
            if dead[t, i]:
                vs[t, i], carry, nxt = v, f32(0), v
                continue
            nv = V[t + 1, i] if e == 0 else (f32(0) if tv is None else tv[t, i]) if e == TRUNCATED else f32(0)
            s = reward[t, i] * scale
            r = clip if s > clip else -clip if s < -clip else s
            x = (w if w < rho_bar else rho_bar) * ((r + g * nv) - v)
            if e == 0:
                x = x + (g * (lam * (w if w < c_bar else c_bar))) * carry
            vs[t, i] = x + v
            pg[t, i] = (w if w < pg_bar else pg_bar) * ((r + g * (nxt if e == 0 else nv)) - v)
            carry, nxt = x, vs[t, i]
    return vs, pg


def sums_f64(tr, L, bars, tv):
    """Espeholt et al. (2018), eq. 1 with the remark's lambda, in float64: vs_t = V_t + sum_k gamma^(k-t) (prod_(t<=i<k) c_i) delta_k
    over the rows of one episode from t on, and the advantage rho_pg (r + gamma vs_(t+1) - V_t)."""
    dead, ends, reward = rows_of(tr, first_of(L), L)
    v, rho = V[:L + 1].astype(np.float64), RHO[:L].astype(np.float64)
    r = np.clip(reward.astype(np.float64) * SCALE, -CLIP, CLIP)
    boot = np.where(ends == 0, v[1:], np.where(ends == TRUNCATED, 0.0 if tv is None else tv[:L], 0.0))
    delta = np.minimum(rho, bars[0]) * (r + GAMMA * boot - v[:L])
    c = LAM * np.minimum(rho, bars[1])
    vs = v.copy()
    for t in range(L):
        weight = np.where(dead[t], 0.0, 1.0)  # gamma^(k-t) prod c_i, 0 once the episode is over
        for k in range(t, L):
            weight = np.where(dead[k], 0.0, weight)
            vs[t] += weight * delta[k]
            weight = np.where(ends[k] != 0, 0.0, weight * GAMMA * c[k])
    pg = np.minimum(rho, bars[2]) * (r + GAMMA * np.where(ends == 0, vs[1:], boot) - v[:L])
    return vs[:L], np.where(dead, 0.0, pg)


def bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)


@pytest.mark.parametrize("L", LENGTHS)
def test_vtrace_is_the_model_bit_for_bit(run, L):
    v, m = run
    for bars in BARS[1:] + BARS[:1]:
        assert bars[0] == 1.0 or all(((RHO[:L] < b).any() and (RHO[:L] > b).any()) for b in bars)  # each clip binds on some cells only
        for tv in (None, TV):
            want_vs, want_pg = model_f32(m.tr, L, bars, tv)
            for adv in (False, True):
                vs, pg = v.transition_vtrace(first_of(L), L, V[:L + 1], RHO[:L], GAMMA, LAM, *bars, trunc_values=None if tv is None else tv[:L],
                                             reward_scale=SCALE, reward_clip=CLIP, advantages=adv)
                assert np.array_equal(bits(vs), bits(want_vs)), (L, bars, tv is None, adv)
                assert pg is None if not adv else np.array_equal(bits(pg), bits(want_pg)), (L, bars, tv is None)
            if L == LENGTHS[-1]:  # the rule, not the rounding
                ref_vs, ref_pg = sums_f64(m.tr, L, bars, tv)
                assert np.abs(vs.cpu().numpy() - ref_vs).max() <= F64_BOUND and np.abs(pg.cpu().numpy() - ref_pg).max() <= F64_BOUND


@pytest.mark.parametrize("lam", [0.95, 1.0])
def test_the_gae_law(run, lam):
    """Without ratios and with the defaults, vs is transition_gae's returns."""
    v, _ = run
    for L in LENGTHS:
        vs, _ = v.transition_vtrace(first_of(L), L, V[:L + 1], gamma=GAMMA, lam=lam, trunc_values=TV[:L])
        assert np.array_equal(bits(vs), bits(v.transition_gae(first_of(L), L, V[:L + 1], GAMMA, lam, TV[:L])[1])), L


def test_the_refusals(run):
    v, _ = run
    h, fn, head = v._h, v.L.pgv_transitions_vtrace, v.history.head
    vals = torch.zeros(3 * N + 2, device="cuda")
    out = torch.full((2 * N + 2,), 3.0, device="cuda")

    def refused(first, length, word, size=None, env=h, **fields):
        q = pglib.vtrace(**{**dict(gamma=0.99, lam=1.0, values=vals.data_ptr(), vs=out.data_ptr()), **fields})
        q.struct_size = size or q.struct_size
        assert fn(env, first, length, ctypes.byref(q)) != 0
        msg = v.L.pgv_last_error().decode()
        assert "pgv_transitions_vtrace" in msg and word in msg, msg

    refused(head - 2, 2, "held"), refused(head - T - 1, 2, "held"), refused(head - 3, 0, "length"), refused(head - 3, 1, "struct_size", size=64)
    refused(head - 3, 1, "NULL", values=None), refused(head - 3, 1, "NULL", vs=None)
    for name in ("values", "rhos", "trunc_values", "vs", "pg_advantages"):
        refused(head - 3, 1, "aligned", **{name: out.data_ptr() + 2})
    plain = ProcgenVecEnv("maze", 4, seed_base=1, history=dict(capacity=4))
    refused(0, 1, "pgv_transitions_enable", env=plain._h)
    plain.close()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
