"""Augmented history gathers (include/procgen2_vec.h pgv_history_gather_aug), the GPU half: the HIP engine against the model
of tests/history_aug_util.py, bit for bit — rows and params — over the seven configurations, both edge rules, both colour
modes, the four element types and K = 1, 3, 4, 8; the identity law against the plain gather; real frames; that the call
changes nothing and writes inside its rows only; the refusals; count = 0.

N = 5 envs and T = 4 slots throughout: the kernel has a workgroup per entry, so what matters is the entries (256 of them),
the windows and the row sizes, not the batch.  tests/test_history_aug.py counts, on the model, what the configurations draw.
"""
import ctypes
from ctypes import c_float, c_void_p

import numpy as np
import pytest
import torch

from engine_util import _dump
from episodes_util import synthetic_actions
from history_aug_util import COLORS, CONFIGS, EDGES, ENTRIES, SEED, aug_params_many, augment, config
from history_util import HistoryRing, HistoryVec, cut_and_wrapped
from policy_obs_util import DTYPES, value_table
from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import ProcgenVecEnv

pytestmark = pytest.mark.gpu

N, T, RUN_SEED = 5, 4, 7


def bits(t):
    """A torch tensor's bit patterns as numpy, on the host."""
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def make(game, gray):
    return ProcgenVecEnv(game, N, seed_base=1, history=dict(capacity=T, gray=gray))


def augment_arg(cfg):
    return dict(size=(cfg["H"], cfg["W"]), pad=cfg["pad"], edge=cfg["edge"], cutout=(cfg["lo"], cfg["hi"]) if cfg["hi"] else None,
                cutout_color=cfg["color"], seed=cfg["seed"])


def entries_of(ring, count=ENTRIES):
    """`count` (push, env) pairs: every held pair, over and over, and at five places in between p = head, p = head - T - 1,
    p = -1, env = -1 and env = N."""
    held = [(p, i) for p in range(max(0, ring.head - ring.T), ring.head) for i in range(ring.n)]
    odd = {3: (ring.head, 0), 50: (ring.head - ring.T - 1, 1), 101: (-1, 2), 200: (ring.head - 1, -1), count - 1: (ring.head - 1, ring.n)}
    pairs = [odd[k] if k in odd else held[(k * 7) % len(held)] for k in range(count)]
    return [p for p, _ in pairs], [i for _, i in pairs]


def check_aug(v, ring, pushes, envs, K, cfg, dtypes, what):
    """The rows of every dtype of `dtypes` and the params against the model.  The model's bytes are worked out once: a dtype's
    rows are its value table over them (the u8 table is the identity)."""
    want8, want_params = augment(ring, pushes, envs, K, "uint8", cfg)
    p, i = torch.as_tensor(pushes, dtype=torch.int64, device="cuda"), torch.as_tensor(envs, dtype=torch.int32, device="cuda")
    for dtype in dtypes:
        got, params = v.history_gather(p, i, stack=K, dtype=dtype, augment=augment_arg(cfg), return_params=True)
        assert got.dtype == getattr(torch, dtype) and tuple(got.shape) == want8.shape and got.is_contiguous(), (what, dtype)
        assert params.dtype == torch.int32 and np.array_equal(params.cpu().numpy(), want_params), ("params", what, dtype)
        assert np.array_equal(bits(got), value_table(dtype)[want8]), ("rows", what, dtype)
    return want8, want_params


class RandomRing:
    """coinrun, six steps with masked resets in between, then the ring's frames overwritten with random bytes — every
    neighbouring pixel differs, so a shift that is off by one cannot hide — and the model built from those bytes and the
    began bytes read back."""

    def __init__(self, gray):
        self.v = v = make("coinrun", gray)
        v.reset()
        for t in range(6):
            v.step(torch.as_tensor(synthetic_actions(RUN_SEED, t, N)))
            if t == 1:  # after the second step: envs 1 and 3
                v.reset(mask=torch.as_tensor([0, 1, 0, 1, 0], dtype=torch.uint8))
            if t == 3:  # … and once more where the slot is still held at the end (the one above has left the ring by then)
                v.reset(mask=torch.as_tensor([0, 0, 0, 1, 0], dtype=torch.uint8))
        v.sync()
        shape = (T, N, 1 if gray else 3, 64, 64)
        noise = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
        v.history.frames.copy_(torch.as_tensor(noise, device="cuda"))
        torch.cuda.synchronize()
        self.ring = ring = HistoryRing(N, T, gray, frames=noise)
        ring.began = v.history.began.cpu().numpy().copy()
        ring.pending = v.history.pending.cpu().numpy().copy()
        ring.head = v.history.head
        self.pushes, self.envs = entries_of(ring)
        assert {(p, i) for p in range(ring.head - T, ring.head) for i in range(N)} <= set(zip(self.pushes, self.envs))


@pytest.fixture(scope="module", params=[False, True], ids=["rgb", "gray"])
def random_ring(request):
    r = RandomRing(request.param)
    yield r
    r.v.close()


def test_the_random_ring_cuts_stacks(random_ring):
    """On the model: held slots carry began bytes of both values, some stack is cut by a began byte, some by the oldest held
    push — what the comparisons below then went through."""
    ring = random_ring.ring
    assert ring.head == 7 and ring.T == T
    held = [ring.began[p % T] for p in range(ring.head - T, ring.head)]
    assert any(row.any() for row in held) and any((row == 0).any() for row in held)
    assert cut_and_wrapped(ring, 4)[0] >= 1 and cut_and_wrapped(ring, 3)[0] >= 1
    oldest = ring.head - T
    assert any(len(set(ring.walk(p, i, 4))) < 4 and min(ring.walk(p, i, 4)) == oldest and not ring.began[oldest % T][i]
               for p in range(oldest, ring.head) for i in range(N))
    assert len(set(ring.walk(ring.head - 1, 0, 3))) == 3  # … and some stack is whole


@pytest.mark.parametrize("shape", CONFIGS, ids=["%dx%d_pad%d_cut%d_%d" % s for s in CONFIGS])
def test_random_ring_matches_the_model(random_ring, shape):
    """256 entries, seed 1: both edges x both colour modes x the four dtypes x K = 1, 3, 4, and one K = 8 u8 case."""
    v, ring, pushes, envs = random_ring.v, random_ring.ring, random_ring.pushes, random_ring.envs
    zero_rows = [k for k, (p, i) in enumerate(zip(pushes, envs)) if not ring.held(p) or not 0 <= i < N]
    assert len(zero_rows) == 5
    for edge in EDGES:
        for color in COLORS:
            cfg = config(shape, edge=edge, color=color, seed=SEED)
            for K in (1, 3, 4):
                want8, params = check_aug(v, ring, pushes, envs, K, cfg, list(DTYPES), (shape, edge, color, K))
                assert not want8[zero_rows].any()
    cfg = config(shape, edge="replicate", color="random", seed=SEED)
    _, params = check_aug(v, ring, pushes, envs, 8, cfg, ["uint8"], (shape, "K=8"))
    # the law of the params: the rows the host gives, the seventh word cut to the one byte a gray ring used
    host = aug_params_many(cfg, np.arange(ENTRIES))
    a = pglib.gather_aug(cfg["H"], cfg["W"], cfg["pad"], cfg["edge"], cfg["lo"], cfg["hi"], cfg["color"], cfg["seed"])
    row = (ctypes.c_int32 * 8)()
    for e in (0, 1, 77, ENTRIES - 1):
        assert v.L.pgv_gather_aug_params(ctypes.byref(a), e, row) == 0 and list(row) == host[e].tolist()
    if ring.C == 1:
        host[:, 6] &= 0xFF
    assert np.array_equal(params, host)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_identity_law(random_ring, dtype):
    """64 x 64, pad 0, no cutout: pgv_history_gather's rows bit for bit, whatever the seed and the edge rule."""
    v, pushes, envs = random_ring.v, random_ring.pushes, random_ring.envs
    for K in (1, 4, 8):
        plain = v.history_gather(pushes, envs, stack=K, dtype=dtype)
        assert bool(plain.any())
        for edge in EDGES:
            for seed in (0, 1, 0xFFFFFFFF):
                got, params = v.history_gather(pushes, envs, stack=K, dtype=dtype, augment=dict(size=64, pad=0, edge=edge, seed=seed), return_params=True)
                assert tuple(got.shape) == tuple(plain.shape) and np.array_equal(bits(got), bits(plain)), (K, edge, seed)
                assert not bool(params.any())


@pytest.mark.parametrize("game", ["maze", "bossfight"])
def test_real_frames(game):
    """Ten steps beside the oracle: configurations (1) and (2), f16, K = 4, over every held pair after every call."""
    v, model = make(game, False), HistoryVec(game, N, T, False)
    v.reset(), model.first_reset()
    one, two = config(CONFIGS[0], seed=SEED), config(CONFIGS[1], edge="zero", color="random", seed=SEED + 1)
    for t in range(-1, 10):
        if t >= 0:
            a = synthetic_actions(RUN_SEED, t, N)
            v.step(torch.as_tensor(a)), model.step(a)
        ring = model.ring
        assert v.history.head == ring.head and np.array_equal(v.history.frames.cpu().numpy(), ring.frames)
        pushes, envs = entries_of(ring, 32)
        for cfg in (one, two):
            want8, _ = check_aug(v, ring, pushes, envs, 4, cfg, ["float16"], (game, t))
            assert want8.any()
    v.close(), model.close()


def state_of(v, env):
    return _dump(lambda buf, m: v.L.pgv_dump_state(v._h, env, buf, m), c_float, np.float32)


def test_no_side_effects_and_no_byte_outside_the_rows(random_ring):
    """Ring, began bytes, pending flags and head as they were; a second call gives the same bytes; rows of every size class
    (16-byte units; 8-byte units with rows of 8 mod 16 bytes) written into exactly `count` rows inside a larger tensor of
    0xA5 leave both guards alone, a zero row at the very end included."""
    v, ring = random_ring.v, random_ring.ring
    h = v.history
    before = (h.frames.clone(), h.began.clone(), h.pending.clone(), h.head)
    count, guard = 7, 4096
    pushes, envs = entries_of(ring, count)  # (the last entry names env N: a row of zeros)
    for shape, dtype, K in ((CONFIGS[4], "uint8", 1), (CONFIGS[4], "uint8", 3), (CONFIGS[3], "uint8", 1), (CONFIGS[6], "uint8", 3),
                            (CONFIGS[3], "float16", 1), (CONFIGS[4], "float32", 4), (CONFIGS[1], "float16", 4), (CONFIGS[2], "bfloat16", 8)):
        cfg = config(shape, color="random", seed=SEED)
        want8, want_params = augment(ring, pushes, envs, K, "uint8", cfg)
        es = pglib.POLICY_DTYPES[dtype][1]
        body = want8.size * es
        assert body == count * K * ring.C * cfg["H"] * cfg["W"] * es
        slab = torch.full((guard + body + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        out = slab[guard:guard + body].view(getattr(torch, dtype)).view(want8.shape)
        got = v.history_gather(pushes, envs, stack=K, dtype=dtype, out=out, augment=augment_arg(cfg))
        assert got is out and np.array_equal(bits(out), value_table(dtype)[want8]), (shape, dtype, K)
        assert bool((slab[:guard] == 0xA5).all()) and bool((slab[guard + body:] == 0xA5).all()), (shape, dtype, K)
        again = v.history_gather(pushes, envs, stack=K, dtype=dtype, augment=augment_arg(cfg))
        assert np.array_equal(bits(again), bits(out))
    assert bool((h.frames == before[0]).all()) and bool((h.began == before[1]).all()) and bool((h.pending == before[2]).all()) and h.head == before[3]


def test_the_next_step_equals_a_twin_that_never_gathered():
    v, twin = make("bossfight", False), make("bossfight", False)
    v.reset(), twin.reset()
    cfg = augment_arg(config(CONFIGS[1], color="random", seed=5))
    for t in range(6):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, N))
        v.step(a), twin.step(a)
        pushes, envs = [v.history.head - 1 - (k % T) for k in range(9)], [k % (N + 1) for k in range(9)]
        v.history_gather(pushes, envs, stack=4, dtype="float16", augment=cfg, return_params=True)
        assert bool((v.obs == twin.obs).all()) and bool((v.reward == twin.reward).all()) and bool((v.done == twin.done).all()), t
        assert v.history.head == twin.history.head and bool((v.history.frames == twin.history.frames).all()), t
        assert bool((v.history.began == twin.history.began).all()) and bool((v.history.pending == twin.history.pending).all()), t
    for i in range(N):
        assert np.array_equal(state_of(v, i).view(np.uint32), state_of(twin, i).view(np.uint32))
    assert v.L.pgv_snapshot_bytes(v._h) == v.L.pgv_snapshot_bytes(twin._h) and v.env_record_bytes == twin.env_record_bytes
    v.close(), twin.close()


def test_refusals_on_a_live_engine():
    """Without history=, a misaligned d_out or params, NULL pointers, bad ranges: a message by name, no byte written, and the
    engine as it was — it goes on equal to a twin that saw none of it."""
    plain, v, twin = ProcgenVecEnv("maze", N, seed_base=1), make("maze", False), make("maze", False)
    L = v.L
    plain.reset(), v.reset(), twin.reset()
    for t in range(3):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, N))
        v.step(a), twin.step(a)
    G = "pgv_history_gather_aug"
    p = torch.full((4,), v.history.head - 1, dtype=torch.int64, device="cuda")
    i = torch.arange(4, dtype=torch.int32, device="cuda")
    rows = torch.full((4 * 8 * 3 * 4096 * 4 + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    par = torch.full((4 * 8 + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    P, I, O = c_void_p(p.data_ptr()), c_void_p(i.data_ptr()), c_void_p(rows.data_ptr())
    torch.cuda.synchronize()

    def refused(rc, word):
        assert rc != 0, "not refused"
        msg = L.pgv_last_error().decode()
        assert G in msg and word in msg, msg

    def aug(**change):
        f = dict(dict(out_height=56, out_width=56, pad=4, edge=0, cutout_min=4, cutout_max=24, cutout_color=1, seed=1, params=par.data_ptr()), **change)
        size = f.pop("size", ctypes.sizeof(pglib.GatherAug))
        return ctypes.byref(pglib.GatherAug(size, f["out_height"], f["out_width"], f["pad"], f["edge"], f["cutout_min"], f["cutout_max"],
                                            f["cutout_color"], f["seed"], f["params"]))

    refused(L.pgv_history_gather_aug(plain._h, P, I, 4, 4, 1, aug(), O), "pgv_history_enable")
    with pytest.raises(pglib.EngineError):
        plain.history_gather([0], [0], augment=dict(size=56, seed=1))
    h = v._h
    refused(L.pgv_history_gather_aug(h, P, I, 4, 0, 1, aug(), O), "stack"), refused(L.pgv_history_gather_aug(h, P, I, 4, 9, 1, aug(), O), "stack")
    refused(L.pgv_history_gather_aug(h, P, I, 4, 4, 4, aug(), O), "dtype"), refused(L.pgv_history_gather_aug(h, P, I, -1, 4, 1, aug(), O), "count")
    refused(L.pgv_history_gather_aug(h, P, I, 4, 4, 1, aug(), c_void_p(rows.data_ptr() + 8)), "16-byte aligned")
    refused(L.pgv_history_gather_aug(h, P, I, 0, 4, 1, aug(), c_void_p(rows.data_ptr() + 8)), "16-byte aligned")
    refused(L.pgv_history_gather_aug(h, P, I, 4, 4, 1, aug(params=par.data_ptr() + 2), O), "4-byte aligned")
    refused(L.pgv_history_gather_aug(h, None, I, 4, 4, 1, aug(), O), "NULL"), refused(L.pgv_history_gather_aug(h, P, None, 4, 4, 1, aug(), O), "NULL")
    refused(L.pgv_history_gather_aug(h, P, I, 4, 4, 1, aug(), None), "NULL"), refused(L.pgv_history_gather_aug(h, P, I, 4, 4, 1, None, O), "aug is NULL")
    refused(L.pgv_history_gather_aug(h, P, I, 4, 4, 1, aug(size=40), O), "struct_size")
    for change, word in ((dict(out_height=0), "out_height"), (dict(out_height=65), "out_height"), (dict(out_width=60), "out_width"),
                         (dict(out_width=72), "out_width"), (dict(pad=17), "pad"), (dict(pad=-1), "pad"), (dict(edge=2), "edge"),
                         (dict(cutout_color=2), "colour"), (dict(cutout_min=25), "cutout_min"), (dict(cutout_min=0), "cutout_min"),
                         (dict(cutout_max=65), "cutout")):
        refused(L.pgv_history_gather_aug(h, P, I, 4, 4, 1, aug(**change), O), word)
    torch.cuda.synchronize()
    assert bool((rows == 0x5A).all()) and bool((par == 0x5A5A5A5A).all())
    # … and the call as it should be goes through, params inside their rows
    assert L.pgv_history_gather_aug(h, P, I, 4, 4, 1, aug(), O) == 0, L.pgv_last_error()
    torch.cuda.synchronize()
    assert bool((par[32:] == 0x5A5A5A5A).all()) and bool((rows[4 * 12 * 56 * 56 * 2:] == 0x5A).all()) and bool((rows[:4 * 12 * 56 * 56 * 2] != 0x5A).any())
    assert np.array_equal(par[:32].cpu().numpy().reshape(4, 8), aug_params_many(config(CONFIGS[1], color="random", seed=1) | dict(pad=4), np.arange(4)))
    for t in range(3, 8):
        a = torch.as_tensor(synthetic_actions(RUN_SEED, t, N))
        v.step(a), twin.step(a)
        assert bool((v.obs == twin.obs).all()) and bool((v.reward == twin.reward).all()) and bool((v.done == twin.done).all()), t
        assert v.history.head == twin.history.head and bool((v.history.frames == twin.history.frames).all()), t
        assert bool((v.history.began == twin.history.began).all()) and bool((v.history.pending == twin.history.pending).all()), t
    plain.close(), v.close(), twin.close()


def test_nothing_to_gather(random_ring):
    """count = 0 succeeds, touches neither buffer, and the Python call gives empty tensors of the right shape."""
    v = random_ring.v
    rows = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    par = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a = pglib.gather_aug(56, 56, 0, "replicate", 4, 24, "random", 1, par.data_ptr())
    assert v.L.pgv_history_gather_aug(v._h, None, None, 0, 4, 1, ctypes.byref(a), c_void_p(rows.data_ptr())) == 0
    assert v.L.pgv_history_gather_aug(v._h, None, None, 0, 4, 1, ctypes.byref(a), None) == 0
    torch.cuda.synchronize()
    assert bool((rows == 0x5A).all()) and bool((par == 0x5A5A5A5A).all())
    empty, params = v.history_gather([], [], stack=4, dtype="float16", augment=dict(size=(56, 48), seed=1), return_params=True)
    assert tuple(empty.shape) == (0, 4 * random_ring.ring.C, 56, 48) and empty.dtype == torch.float16
    assert tuple(params.shape) == (0, 8) and params.dtype == torch.int32
