"""The model of the augmented history gathers (include/procgen2_vec.h pgv_history_gather_aug) in pure numpy: the draws of an
entry from the header's formulas, and the augmented rows as plain per-pixel index arithmetic — np.clip for the replicate
edge, boolean masks for the zero edge and the cutout — over tests/history_util.py's HistoryRing (its walk, its held rule) and
tests/policy_obs_util.py's values.  It shares no code with the engine.  The GPU tests trust this model; tests/test_history_aug.py
holds the engine's host half to it and counts what the configurations reach.
"""
import numpy as np

from policy_obs_util import DTYPES, value_table

# (H', W', pad, cutout_min, cutout_max)
CONFIGS = [(64, 64, 4, 0, 0), (56, 56, 0, 4, 24), (8, 8, 16, 1, 1), (1, 8, 0, 0, 0), (63, 24, 1, 24, 40), (64, 64, 0, 64, 64), (33, 40, 16, 8, 8)]
EDGES = ("replicate", "zero")
COLORS = ("black", "random")
ENTRIES, SEED = 256, 1  # what the GPU test gathers

M = np.uint64(0xFFFFFFFF)


def config(shape, edge="replicate", color="black", seed=SEED):
    H, W, pad, lo, hi = shape
    return dict(H=H, W=W, pad=pad, lo=lo, hi=hi, edge=edge, color=color, seed=seed)


def mix32(x):
    """The engine's hash on uint32 values held in uint64 (scalars or arrays)."""
    x = np.asarray(x, np.uint64) & M
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M
    return x ^ (x >> np.uint64(16))


def word(seed, e, j):
    e = np.asarray(e, np.uint64)
    inner = mix32((np.uint64(seed) + np.uint64(0x9E3779B9) * (e + np.uint64(1))) & M)
    return mix32(inner ^ np.uint64((j * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF))


def draw(seed, e, m, j):
    return ((word(seed, e, j) * np.asarray(m, np.uint64)) >> np.uint64(32)).astype(np.int64)


def aug_params_many(cfg, entries, gray=False):
    """int32 [len(entries), 8]: oy, ox, cy, cx, ch, cw, colour, 0."""
    e = np.asarray(entries, np.uint64)
    H, W, pad, lo, hi, seed = cfg["H"], cfg["W"], cfg["pad"], cfg["lo"], cfg["hi"], cfg["seed"]
    out = np.zeros((len(e), 8), np.int64)
    out[:, 0] = -pad + draw(seed, e, 64 + 2 * pad - H + 1, 0)
    out[:, 1] = -pad + draw(seed, e, 64 + 2 * pad - W + 1, 1)
    if hi > 0:
        ch = np.minimum(H, lo + draw(seed, e, hi - lo + 1, 2))
        cw = np.minimum(W, lo + draw(seed, e, hi - lo + 1, 3))
        out[:, 2] = draw(seed, e, (H - ch + 1).astype(np.uint64), 4)
        out[:, 3] = draw(seed, e, (W - cw + 1).astype(np.uint64), 5)
        out[:, 4], out[:, 5] = ch, cw
        if cfg["color"] == "random":
            out[:, 6] = (word(seed, e, 6) & np.uint64(0xFF if gray else 0xFFFFFF)).astype(np.int64)
    return out.astype(np.int32)


def aug_params(cfg, e, gray=False):
    return aug_params_many(cfg, [e], gray)[0]


def augment(ring, pushes, envs, K, dtype, cfg, entries=None):
    """(bit patterns [B, K*C, H', W'], params int32 [B, 8]) of the entries (pushes[b], envs[b]) of a HistoryRing.  entries:
    the rows' positions in the call they are part of (what the draws go by), default 0 .. B-1."""
    table, C, H, W = value_table(dtype), ring.C, cfg["H"], cfg["W"]
    params = aug_params_many(cfg, np.arange(len(pushes)) if entries is None else entries, gray=ring.C == 1)
    out = np.zeros((len(pushes), K * C, H, W), DTYPES[dtype])
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    for b, (p, i) in enumerate(zip(pushes, envs)):
        p, i = int(p), int(i)
        if not ring.held(p) or not 0 <= i < ring.n:
            continue
        oy, ox, cy, cx, ch, cw, colour, _ = (int(v) for v in params[b])
        sy, sx = oy + y, ox + x
        inside = (sy >= 0) & (sy < 64) & (sx >= 0) & (sx < 64)
        cut = (y >= cy) & (y < cy + ch) & (x >= cx) & (x < cx + cw)
        for j, f in enumerate(ring.walk(p, i, K)):
            stored = ring.frames[f % ring.T][i]  # [C, 64, 64]
            byte = stored[:, np.clip(sy, 0, 63), np.clip(sx, 0, 63)]  # [C, H', W']: the nearest pixel of the frame
            if cfg["edge"] == "zero":
                byte = np.where(inside[None], byte, 0)
            byte = byte.astype(np.uint8)
            for c in range(C):
                byte[c][cut] = (colour >> (8 * c)) & 0xFF
            out[b, (K - 1 - j) * C:(K - j) * C] = table[byte]
    return out, params


def windows_outside(cfg, entries=ENTRIES):
    """How many of the entries' windows lie entirely outside the frame."""
    p = aug_params_many(cfg, np.arange(entries)).astype(np.int64)
    oy, ox = p[:, 0], p[:, 1]
    return int(((oy + cfg["H"] <= 0) | (oy >= 64) | (ox + cfg["W"] <= 0) | (ox >= 64)).sum())
