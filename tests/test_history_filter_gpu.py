"""Filtered history gathers (include/procgen2_vec.h pgv_history_gather_filter), the GPU half: the HIP engine against the
model of tests/history_filter_util.py on tests/test_history_aug_gpu.py's random-byte ring (N = 5, T = 4, rgb and gray) —
bit for bit against the float32 restatement, within a derived bound of the float64 one — and the identity law, the
refusals, the bytes round the rows and count = 0.

The bound, per element of output plane o with n = C*k*k terms and |v| <= 1: E = (n + 2) * 2^-24 * (|b_o| + sum |w_o|) (a
rounding of each v, each product and each sum, first order), plus the format's half ulp — relative 2^-11 (binary16) or 2^-8
(bfloat16) of |ref| + E — plus 2^-25 for binary16's subnormals.  The clamp only ever lessens an error."""
import ctypes
import functools
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from history_filter_util import element_bits, element_values, filter_models, turned_images
from procgen2_amd import lib as pglib
from test_history_aug_gpu import RandomRing, bits, entries_of

pytestmark = pytest.mark.gpu

ENTRIES, SEED = 64, 1
# (H', W', pad, edge, cutout, flip and rot90): the border-only row, 8- and 16-byte rows, an odd height, all four turns
SHAPES = [(64, 64, 0, "replicate", None, False), (8, 8, 16, "zero", None, False), (1, 8, 0, "replicate", None, False),
          (63, 24, 1, "replicate", (24, 40), False), (56, 56, 4, "replicate", (4, 24), True)]
HALF_ULP = {"float32": (0.0, 0.0), "float16": (2.0 ** -11, 2.0 ** -25), "bfloat16": (2.0 ** -8, 0.0)}


@pytest.fixture(scope="module", params=[False, True], ids=["rgb", "gray"])
def random_ring(request):
    r = RandomRing(request.param)
    r.pushes, r.envs = entries_of(r.ring, ENTRIES)  # (p = head at 3, p = head - T - 1 at 50, env = N at the end)
    r.pushes[20], r.envs[20], r.pushes[37], r.envs[37] = -1, 2, r.ring.head - 1, -1  # … and the other two of the five
    yield r
    r.v.close()


def arguments(shape, seed=SEED):
    H, W, pad, edge, cutout, turn = shape
    lo, hi = cutout or (0, 0)
    cfg = dict(H=H, W=W, pad=pad, lo=lo, hi=hi, edge=edge, color="random", seed=seed)
    augment = dict(size=(H, W), pad=pad, edge=edge, cutout=cutout, cutout_color="random", seed=seed)
    return cfg, dict(augment, flip=True, rot90=True) if turn else augment


def weights_of(C, kernel, per_entry, extras):
    rng = np.random.default_rng(100 * kernel + 10 * per_entry + C)
    w = rng.normal(0.0, 0.2, (ENTRIES if per_entry else 1, C, C, kernel, kernel)).astype(np.float32)
    b = rng.normal(0.0, 0.2, (ENTRIES if per_entry else 1, C)).astype(np.float32) if extras else None
    return w, b, (0.0, 1.0) if extras else None


@functools.lru_cache(maxsize=2)
def models(r, shape, kernel, per_entry, extras, K):
    """The model of a case, shared by its three dtypes."""
    cfg, _ = arguments(shape)
    G, params, held = turned_images(r.ring, r.pushes, r.envs, K, cfg, shape[5], shape[5])
    assert (~held).sum() == 5 and (not shape[5] or set(params[:, 7]) == set(range(8)))
    return filter_models(G, held, *weights_of(r.ring.C, kernel, per_entry, extras)) + (params,)


@pytest.mark.parametrize("dtype", list(HALF_ULP))
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "bias_clamp"])
@pytest.mark.parametrize("per_entry", [False, True], ids=["shared", "per_entry"])
@pytest.mark.parametrize("kernel", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_pad%d" % s[:3] for s in SHAPES])
def test_filter_matches_the_model(random_ring, shape, kernel, per_entry, extras, K, dtype):
    r = random_ring
    want32, want64, E, want_params = models(r, shape, kernel, per_entry, extras, K)
    w, b, clamp = weights_of(r.ring.C, kernel, per_entry, extras)
    flt = dict(weights=torch.as_tensor(w if per_entry else w[0]), bias=None if b is None else torch.as_tensor(b if per_entry else b[0]), clamp=clamp)
    got, params = r.v.history_gather(r.pushes, r.envs, stack=K, dtype=dtype, augment=arguments(shape)[1], filter=flt, return_params=True)
    assert got.dtype == getattr(torch, dtype) and tuple(got.shape) == want32.shape and got.is_contiguous()
    assert np.array_equal(params.cpu().numpy(), want_params)
    got = bits(got)
    assert np.array_equal(got, element_bits(want32, dtype))
    relative, absolute = HALF_ULP[dtype]
    error, bound = np.abs(element_values(got, dtype) - want64), E + relative * (np.abs(want64) + E) + absolute
    print("largest error / bound: %.3f" % float((error / bound).max()))
    assert (error <= bound).all()
    again = r.v.history_gather(r.pushes, r.envs, stack=K, dtype=dtype, augment=arguments(shape)[1], filter=flt)
    assert np.array_equal(bits(again), got)


@pytest.mark.parametrize("dtype", list(HALF_ULP))
def test_the_identity_law(random_ring, dtype):
    """kernel 1, the identity matrix, no bias, clamp, flip or rotation: pgv_history_gather_aug's rows bit for bit; and
    augment=None stands for the plain gather's rows."""
    r, C = random_ring, random_ring.ring.C
    eye = torch.eye(C).view(C, C, 1, 1)
    for shape in SHAPES:
        _, augment = arguments(shape[:5] + (False,))
        want = r.v.history_gather(r.pushes, r.envs, stack=4, dtype=dtype, augment=augment)
        got, params = r.v.history_gather(r.pushes, r.envs, stack=4, dtype=dtype, augment=augment, filter=dict(weights=eye), return_params=True)
        assert bool(want.any()) and np.array_equal(bits(got), bits(want)) and not bool(params[:, 7].any()), shape
    got = r.v.history_gather(r.pushes, r.envs, stack=4, dtype=dtype, filter=dict(weights=eye))
    assert np.array_equal(bits(got), bits(r.v.history_gather(r.pushes, r.envs, stack=4, dtype=dtype)))


@pytest.mark.parametrize("kernel", [1, 3])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=["%dx%d_pad%d" % s[:3] for s in (SHAPES[1], SHAPES[3])])
def test_a_full_stack_matches_the_model(random_ring, shape, kernel):
    """K = 8, all the head's walk holds, over T = 4: every held entry's walk repeats a frame at least four times, so every
    row takes both sides of the distinct-frame test, restaging (and at kernel 3 rebuilding the image) in between.  Per-entry
    weights, bias and clamp, float32, held to the model as every other case is."""
    test_filter_matches_the_model(random_ring, shape, kernel, True, True, 8, "float32")


@pytest.mark.parametrize("dtype", list(HALF_ULP))
def test_the_identity_chain_at_a_full_stack(random_ring, dtype):
    """K = 8 at 64 x 64, pad 0, no cutout: the plain gather's rows are the augmented gather's, and those the filtered
    gather's with the identity matrix — the four kernels' one walk."""
    r, C = random_ring, random_ring.ring.C
    _, augment = arguments(SHAPES[0])
    plain = r.v.history_gather(r.pushes, r.envs, stack=8, dtype=dtype)
    augmented = r.v.history_gather(r.pushes, r.envs, stack=8, dtype=dtype, augment=augment)
    filtered = r.v.history_gather(r.pushes, r.envs, stack=8, dtype=dtype, augment=augment, filter=dict(weights=torch.eye(C).view(C, C, 1, 1)))
    assert tuple(plain.shape) == (ENTRIES, 8 * C, 64, 64) and bool(plain.any())
    assert np.array_equal(bits(plain), bits(augmented)) and np.array_equal(bits(augmented), bits(filtered))


def test_refusals_guards_and_nothing_to_gather(random_ring):
    """Every refusal of the filter by name with no byte written; a good call writes its rows and params and nothing beside
    them, a zero row at the very end included; count = 0 succeeds and writes nothing."""
    r, C, L = random_ring, random_ring.ring.C, random_ring.v.L
    count, K, guard = 7, 4, 4096
    pushes, envs = entries_of(r.ring, count)  # (the last entry names env N: a row of zeros)
    p, i = torch.as_tensor(pushes, dtype=torch.int64, device="cuda"), torch.as_tensor(envs, dtype=torch.int32, device="cuda")
    w, b = torch.full((C * C * 9 + 1,), 0.01, device="cuda"), torch.full((C + 1,), 0.5, device="cuda")
    body = count * K * C * 56 * 56 * 2
    slab = torch.full((guard + body + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    par = torch.full((count * 8 + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    aug = pglib.gather_aug(56, 56, 4, "replicate", 4, 24, "random", SEED, par.data_ptr())

    def call(n=count, dtype=1, a=aug, size=None, **change):
        f = pglib.gather_filter(**dict(dict(kernel=3, weights=w.data_ptr(), bias=b.data_ptr(), clamp=(0.0, 1.0), flip=True, rot90=True), **change))
        f.struct_size = f.struct_size if size is None else size
        return L.pgv_history_gather_filter(r.v._h, c_void_p(p.data_ptr()), c_void_p(i.data_ptr()), n, K, dtype, ctypes.byref(a), ctypes.byref(f),
                                           c_void_p(slab.data_ptr() + guard))

    tall = pglib.gather_aug(56, 48, 4, "replicate", 0, 0, "black", SEED, None)
    for word, change in (("struct_size", dict(size=8)), ("kernel", dict(kernel=2)), ("kernel", dict(kernel=0)), ("weights is NULL", dict(weights=None)),
                         ("weights_stride", dict(weights_stride=C * C)), ("bias_stride", dict(bias_stride=C + 1)), ("4-byte", dict(weights=w.data_ptr() + 2)),
                         ("4-byte", dict(bias=b.data_ptr() + 1)), ("rot90", dict(a=tall)), ("uint8", dict(dtype=0)), ("lo <= hi", dict(clamp=(1.0, 0.0))),
                         ("lo <= hi", dict(clamp=(0.0, float("nan")))), ("out_width", dict(a=pglib.gather_aug(56, 60, seed=1))), ("count", dict(n=-1))):
        assert call(**change) != 0, word
        msg = L.pgv_last_error().decode()
        assert "pgv_history_gather_filter" in msg and word in msg, msg
    assert L.pgv_history_gather_filter(r.v._h, None, None, 0, K, 1, ctypes.byref(aug), None, None) != 0 and b"filter is NULL" in L.pgv_last_error()
    assert call(n=0) == 0 and call(n=0, a=tall, rot90=False) == 0
    torch.cuda.synchronize()
    assert bool((slab == 0xA5).all()) and bool((par == 0x5A5A5A5A).all())
    with pytest.raises(ValueError):
        r.v.history_gather(pushes, envs, dtype="uint8", filter=dict(weights=torch.eye(C).view(C, C, 1, 1)))
    with pytest.raises(ValueError):
        r.v.history_gather(pushes, envs, filter=dict(weights=torch.zeros(C, C, 2, 2)))
    with pytest.raises(ValueError):
        r.v.history_gather(pushes, envs, augment=dict(size=(56, 48), seed=1, rot90=True))
    # the good call: per-entry strides would need 7 sets, so one set; its rows and params rows, the guards as they were
    assert call() == 0, L.pgv_last_error()
    torch.cuda.synchronize()
    assert bool((slab[:guard] == 0xA5).all()) and bool((slab[guard + body:] == 0xA5).all()) and bool((par[count * 8:] == 0x5A5A5A5A).all())
    rows = slab[guard:guard + body].view(torch.float16).view(count, K * C, 56, 56)
    assert not bool(rows[-1].any()) and bool(rows[0].any()) and bool((par[:count * 8].view(count, 8)[:, 7] < 8).all())
    empty, params = r.v.history_gather([], [], stack=4, augment=dict(size=56, seed=1, flip=True), return_params=True)
    assert tuple(empty.shape) == (0, 4 * C, 56, 56) and tuple(params.shape) == (0, 8)
