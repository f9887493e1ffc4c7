"""Frame codes (include/procgen2_vec.h pgv_frame_codes_enable) on the GPU against numpy in int64 over bytes the tests write into
the ring themselves.  maze, N = 8, T = 6, nine pushes, so the held pushes 3 .. 8 lie over the ring's wrap.  Counts 1, 33 and 95:
a lone row, one row past a tile of 32, a ragged last tile past two.  Slot 0 holds the frames of all 0, all 255 and all 128
(every projection exactly 0 under +-1 weights, and exactly the bound under weights of -128 and 127)."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import ProcgenVecEnv

pytestmark = pytest.mark.gpu

N, T, PUSHES, SEED = 8, 6, 9, 5
i64 = np.int64


def make(gray, bits, table=64, weights=None, frame_codes=True):
    fc = dict(bits=bits, seed=SEED, table=table, weights=weights) if frame_codes else None
    v = ProcgenVecEnv("maze", N, history=dict(capacity=T, gray=gray), frame_codes=fc)
    v.reset()
    for _ in range(PUSHES - 1):
        v.step(torch.zeros(N, dtype=torch.int32))
    assert v.history.head == PUSHES
    f = v.history.frames
    f.copy_(torch.from_numpy(np.random.default_rng(bits + gray).integers(0, 256, tuple(f.shape), dtype=np.uint8)))
    f[0, 0], f[0, 1], f[0, 2] = 0, 255, 128
    f[1, 3], f[2, 4] = f[4, 5], f[4, 5]  # distinct pairs, identical bytes
    return v


def entries(count):
    """pushes, envs, valid: the three special frames of slot 0 (push 6) and every kind of invalid entry where there is room."""
    rng = np.random.default_rng(count)
    p, e = rng.integers(PUSHES - T, PUSHES, count), rng.integers(0, N, count)
    if count > 8:
        p[:8], e[:8] = [6, 6, 6, PUSHES, PUSHES - T - 1, -1, 4, 4], [0, 1, 2, 0, 0, 0, -1, N]
    return p.astype(i64), e.astype(np.int32), (p >= PUSHES - T) & (p < PUSHES) & (e >= 0) & (e < N)


def reference(v, p, e, ok):
    t = v.frame_code_table
    w, frames = t.weights.cpu().numpy(), v.history.frames.cpu().numpy()
    x = np.stack([frames[pp % T, ee].reshape(-1) if k else np.full(w.shape[1], 128, np.uint8) for pp, ee, k in zip(p, e, ok)])
    proj = (w.astype(i64) @ (x.astype(i64) - 128).T).T * ok[:, None]
    bit = ((proj >= 0) & ok[:, None]).reshape(len(p), -1, 32).astype(np.uint64)
    return proj, (bit << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def mix32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d); x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


@pytest.fixture(scope="module", params=[(g, b) for g in (True, False) for b in (32, 96, 256)], ids=lambda p: "%s-%d" % ("gray" if p[0] else "rgb", p[1]))
def engine(request):
    v = make(*request.param)
    yield v
    v.close()


@pytest.mark.parametrize("count", [1, 33, 95])
def test_projection_and_codes_equal_numpy_int64(engine, count):
    p, e, ok = entries(count)
    got = engine.frame_codes(p, e, proj=True)
    proj, codes = reference(engine, p, e, ok)
    assert got.visits is None and np.array_equal(got.valid.cpu().numpy(), ok.astype(np.uint8))
    assert np.array_equal(got.proj.cpu().numpy().astype(i64), proj)
    assert np.array_equal(got.codes.cpu().numpy().view(np.uint32), codes)
    if count > 8:
        assert not proj[2].any() and (codes[2] == 0xFFFFFFFF).all() and not codes[3:8].any()  # exact zeros count as >= 0; invalid rows are zeros


def test_generated_weights_are_frame_code_weight(engine):
    t = engine.frame_code_table
    j, d = np.arange(t.bits, dtype=np.uint32)[:, None], np.arange(t.planes * 4096, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        want = np.where(mix32(mix32(np.uint32(SEED) ^ (j * np.uint32(0x9E3779B9))) + d) & np.uint32(1), 1, -1).astype(np.int8)
    assert np.array_equal(t.weights.cpu().numpy(), want)


@pytest.mark.parametrize("gray", [True, False], ids=["gray", "rgb"])
def test_a_callers_weights_reach_the_exact_extremes(gray):
    D = (1 if gray else 3) * 4096
    w = torch.from_numpy(np.random.default_rng(3).integers(-128, 128, (32, D), dtype=np.int8)).cuda()
    w[0], w[1] = -128, 127
    v = make(gray, 32, table=0, weights=w)
    assert v.frame_code_table.weights.data_ptr() == w.data_ptr() and v.frame_code_table.keys is None
    p, e, ok = entries(33)
    got = v.frame_codes(p, e, proj=True)
    proj, codes = reference(v, p, e, ok)
    assert np.array_equal(got.proj.cpu().numpy().astype(i64), proj) and np.array_equal(got.codes.cpu().numpy().view(np.uint32), codes)
    assert proj[0, 0] == D * 128 * 128 and proj[0, 1] == -D * 128 * 127 and proj[1, 0] == -D * 127 * 128 and proj[1, 1] == D * 127 * 127
    with pytest.raises(pglib.EngineError, match="table"):
        v.frame_codes(p, e, count="add")
    v.close()


def multiplicity(codes, salts, ok):
    keys = [tuple(c) + (s,) for c, s in zip(codes.tolist(), salts)]
    tally = collections.Counter(k for k, good in zip(keys, ok) if good)
    return np.array([tally[k] if good else 0 for k, good in zip(keys, ok)]), len(tally)


def test_counts():
    v = make(True, 64)
    t = v.frame_code_table
    p, e, ok = entries(60)
    p[8:14], e[8:14] = [7, 8, 4, 4, 4, 7], [3, 4, 5, 5, 5, 3]  # slots 1, 2, 4: identical bytes; repeated pairs
    codes = reference(v, p, e, ok)[1]
    mult, distinct = multiplicity(codes, [0] * 60, ok)
    assert mult[10] >= 5 and mult[3] == 0
    assert np.array_equal(v.frame_codes(p, e, count="add").visits.cpu().numpy(), mult)
    assert np.array_equal(v.frame_codes(p, e, count="add").visits.cpu().numpy(), 2 * mult)
    before = (t.keys.clone(), t.visits.clone())
    assert np.array_equal(v.frame_codes(p, e, count="look").visits.cpu().numpy(), 2 * mult)
    assert torch.equal(t.keys, before[0]) and torch.equal(t.visits, before[1]) and int(t.used) == distinct and int(t.dropped) == 0
    absent = [(pp, ee) for pp in range(3, 9) for ee in range(N) if (pp, ee) not in set(zip(p.tolist(), e.tolist())) and (pp % T, ee) not in ((1, 3), (2, 4))][0]
    assert v.frame_codes([absent[0]], [absent[1]], count="look").visits.item() == 0  # a frame never added
    salts = np.arange(60, dtype=np.int32) % 2
    salted, distinct2 = multiplicity(codes, salts.tolist(), ok)
    got = v.frame_codes(p, e, salts=salts, count="add", clear=True)  # different salts count apart, in a table emptied first
    assert np.array_equal(got.visits.cpu().numpy(), salted) and int(t.used) == distinct2 and int(t.visits.sum()) == ok.sum()
    v.frame_codes([], [], clear=True)
    assert int(t.used) == 0 and not t.keys.any() and not t.visits.any()
    v.close()


def test_a_full_table_drops_rows_and_says_so():
    v = make(True, 64, table=8)
    pairs = [(pp, ee) for pp in range(3, 9) for ee in range(N) if (pp % T, ee) not in ((1, 3), (2, 4))][:40]  # 40 distinct frames
    p, e = np.array([a for a, _ in pairs] + [a for a, _ in pairs[:10]], i64), np.array([b for _, b in pairs] + [b for _, b in pairs[:10]], np.int32)
    ok = np.ones(50, bool)
    mult, distinct = multiplicity(reference(v, p, e, ok)[1], [0] * 50, ok)
    visits = v.frame_codes(p, e, count="add").visits.cpu().numpy()
    t = v.frame_code_table
    assert distinct == 40 and int(t.used) == 8 and bool(((visits == 0) | (visits == mult)).all()) and int(t.dropped) == int((visits == 0).sum())
    v.close()


def test_refusals_and_feature_off():
    v = make(True, 32, frame_codes=False)
    q, L = pglib.frame_code_query(None), v.L
    assert v.frame_code_table is None
    assert L.pgv_frame_codes(v._h, None, None, 0, ctypes.byref(q)) != 0 and b"pgv_frame_codes_enable first" in L.pgv_last_error()
    with pytest.raises(pglib.EngineError):
        v.frame_codes([3], [0])
    for bits, table in ((0, 8), (48, 8), (288, 8), (64, 4), (64, 24), (64, 1 << 29)):
        with pytest.raises(pglib.EngineError, match="bits|table_capacity"):
            pglib.frame_codes_enable(L, v._h, bits, 0, table)
    pglib.frame_codes_enable(L, v._h, 64, 0, 0)
    with pytest.raises(pglib.EngineError, match="already"):
        pglib.frame_codes_enable(L, v._h, 64, 0, 0)
    q = pglib.frame_code_query("look")
    assert L.pgv_frame_codes(v._h, None, None, 0, ctypes.byref(q)) != 0 and b"table" in L.pgv_last_error()
    q = pglib.frame_code_query(None)
    assert L.pgv_frame_codes(v._h, None, None, -1, ctypes.byref(q)) != 0 and b"negative" in L.pgv_last_error()
    assert L.pgv_frame_codes(v._h, None, None, 0, ctypes.byref(q)) == 0  # count == 0: nothing to do
    v.close()
    bare = ProcgenVecEnv("maze", N)
    with pytest.raises(pglib.EngineError, match="pgv_history_enable first"):
        pglib.frame_codes_enable(bare.L, bare._h, 64, 0, 8)
    bare.close()
