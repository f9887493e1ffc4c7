"""The model of the filtered history gathers (include/procgen2_vec.h pgv_history_gather_filter) in numpy, on top of
tests/history_aug_util.py's: the turn draws, G by np.rot90, and the filter restated twice — in float32 in the header's order,
every product and sum an array operation of its own, and in float64.  It shares no code with the engine."""
import numpy as np

from history_aug_util import augment, draw, word


def turns_many(seed, entries, flip, rot90):
    """int32 [len(entries)]: f | r << 1, the eighth params word."""
    e = np.asarray(entries, np.uint64)
    f = (word(seed, e, 7) >> np.uint64(31)).astype(np.int64) if flip else 0
    r = draw(seed, e, 4, 8) if rot90 else 0
    return (np.zeros(len(e), np.int64) + f + 2 * r).astype(np.int32)


def turned_images(ring, pushes, envs, K, cfg, flip, rot90):
    """(G u8 [B, K, C, H', W'], params int32 [B, 8], held bool [B])."""
    A, params = augment(ring, pushes, envs, K, "uint8", cfg)
    params[:, 7] = turns_many(cfg["seed"], np.arange(len(pushes)), flip, rot90)
    G = A.reshape(len(pushes), K, ring.C, cfg["H"], cfg["W"]).copy()
    for b, t in enumerate(params[:, 7]):
        G[b] = np.rot90(G[b][..., ::-1] if t & 1 else G[b], t >> 1, axes=(-2, -1))
    held = np.array([ring.held(int(p)) and 0 <= int(i) < ring.n for p, i in zip(pushes, envs)])
    return G, params, held


def filter_models(G, held, w, b, clamp):
    """(float32 model, float64 model, the bound's E), each [B, K*C, H', W'].  w [B or 1, C, C, k, k], b [B or 1, C] or None."""
    B, K, C, H, W = G.shape
    k = w.shape[-1]
    pad = [(0, 0)] * 3 + [(k // 2, k // 2)] * 2
    v32, v64 = np.pad(G.astype(np.float32) / np.float32(255), pad), np.pad(G.astype(np.float64) / 255.0, pad)
    zero = np.zeros((1, C), np.float32) if b is None else b
    acc32 = np.broadcast_to(zero[:, None, :, None, None], G.shape).astype(np.float32)
    acc64 = acc32.astype(np.float64)
    for o in range(C):
        for i in range(C):
            for ky in range(k):
                for kx in range(k):
                    ww = w[:, o, i, ky, kx][:, None, None, None]
                    product = ww * v32[:, :, i, ky:ky + H, kx:kx + W]  # float32, rounded
                    acc32[:, :, o] = acc32[:, :, o] + product
                    acc64[:, :, o] += ww.astype(np.float64) * v64[:, :, i, ky:ky + H, kx:kx + W]
    if clamp is not None:
        lo, hi = np.float32(clamp[0]), np.float32(clamp[1])
        acc32 = np.where(acc32 < lo, lo, np.where(acc32 > hi, hi, acc32))
        acc64 = np.clip(acc64, clamp[0], clamp[1])
    E = (C * k * k + 2) * 2.0 ** -24 * (np.abs(zero.astype(np.float64)) + np.abs(w.astype(np.float64)).sum(axis=(2, 3, 4)))  # [B or 1, C]
    E = np.broadcast_to(E[:, None, :, None, None], G.shape)
    acc32[~held], acc64[~held] = 0, 0
    shape = (B, K * C, H, W)
    return acc32.reshape(shape), acc64.reshape(shape), E.reshape(shape)


def element_bits(x32, dtype):
    """float32 → the elements' bit patterns: one rounding to nearest even (bfloat16 by integer arithmetic)."""
    if dtype == "float32":
        return x32.view(np.uint32)
    if dtype == "float16":
        return x32.astype(np.float16).view(np.uint16)
    u = x32.view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def element_values(bits, dtype):
    """The elements' values as float64."""
    if dtype == "bfloat16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    return bits.view(np.float32 if dtype == "float32" else np.float16).astype(np.float64)
