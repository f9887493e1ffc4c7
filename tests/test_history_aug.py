"""Augmented history gathers (include/procgen2_vec.h pgv_history_gather_aug) without a GPU: the new symbols in the built
libraries and their bindings, the engine's host half — pgv_gather_aug_params — against the model the GPU tests trust
(tests/history_aug_util.py), every refusal of a config, procgen2_amd/csrc/pg_history_aug.h compiled for the CPU
(tests/cpp/test_history_aug.cpp), what the seven configurations reach with the GPU test's seed, and the ValueErrors of
ProcgenVecEnv.history_gather(augment=...)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from history_aug_util import COLORS, CONFIGS, ENTRIES, SEED, aug_params, aug_params_many, augment, config, windows_outside
from history_util import HistoryRing
from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("pgv_history_gather_aug", "pgv_gather_aug_params")


@pytest.mark.parametrize("libname", ["libprocgen2_hip.so", "libMaze.so"])
def test_aug_symbols_exported(engine_lib, libname):
    path = os.path.join(pglib.LIB_DIR, libname)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= names


def test_aug_calls_bound(engine_lib):
    L = engine_lib
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pglib.EXPORTED_VEC_SYMBOLS
    assert L.pgv_history_gather_aug.restype is pglib.c_int32 and L.pgv_gather_aug_params.restype is pglib.c_int32
    assert len(L.pgv_history_gather_aug.argtypes) == 8 and len(L.pgv_gather_aug_params.argtypes) == 3
    S = pglib.GatherAug
    # the struct as the header lays it out (LP64): nine words, four bytes of padding, a pointer
    assert ctypes.sizeof(S) == 48
    assert [f for f, _ in S._fields_] == ["struct_size", "out_height", "out_width", "pad", "edge", "cutout_min", "cutout_max", "cutout_color", "seed", "params"]
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert pglib.AUG_EDGES == {"replicate": 0, "zero": 1} and pglib.AUG_CUTOUT_COLORS == {"black": 0, "random": 1}
    a = pglib.gather_aug(56, 48, pad=3, edge="zero", cutout_min=2, cutout_max=9, cutout_color="random", seed=2**32 + 5)
    assert (a.struct_size, a.out_height, a.out_width, a.pad, a.edge, a.cutout_min, a.cutout_max, a.cutout_color, a.seed, a.params) == (
        48, 56, 48, 3, 1, 2, 9, 1, 5, None)
    # NULL handles: refused by name, nothing touched
    assert L.pgv_history_gather_aug(None, None, None, 0, 4, 1, ctypes.byref(a), None) != 0 and b"pgv_history_gather_aug" in L.pgv_last_error()
    row = (ctypes.c_int32 * 8)()
    assert L.pgv_gather_aug_params(None, 0, row) != 0 and b"pgv_gather_aug_params" in L.pgv_last_error()


def engine_params(L, cfg, entries):
    a = pglib.gather_aug(cfg["H"], cfg["W"], cfg["pad"], cfg["edge"], cfg["lo"], cfg["hi"], cfg["color"], cfg["seed"])
    row = (ctypes.c_int32 * 8)()
    out = np.zeros((len(entries), 8), np.int32)
    ref = ctypes.byref(a)
    for k, e in enumerate(entries):
        assert L.pgv_gather_aug_params(ref, int(e), row) == 0, L.pgv_last_error()
        out[k] = row[:]
    return out


@pytest.mark.parametrize("shape", CONFIGS)
def test_params_match_the_model(engine_lib, shape):
    """pgv_gather_aug_params against the model: entries 0 .. 4 095, seeds 0, 1 and 2^32 - 1, both colour modes."""
    entries = np.arange(4096)
    for seed in (0, 1, 0xFFFFFFFF):
        for color in COLORS:
            cfg = config(shape, color=color, seed=seed)
            want = aug_params_many(cfg, entries)
            got = engine_params(engine_lib, cfg, entries)
            assert np.array_equal(got, want), (shape, seed, color)
            H, W, pad, lo, hi = shape
            assert (want[:, 0] >= -pad).all() and (want[:, 0] + H <= 64 + pad).all() and (want[:, 1] >= -pad).all() and (want[:, 1] + W <= 64 + pad).all()
            assert (want[:, 2] + want[:, 4] <= H).all() and (want[:, 3] + want[:, 5] <= W).all() and (want[:, 2:6] >= 0).all()
            assert not want[:, 7].any() and (want[:, 6] >= 0).all() and (want[:, 6] <= 0xFFFFFF).all()
            if hi == 0 or color == "black":
                assert not want[:, 6].any()
            if hi == 0:
                assert not want[:, 2:6].any()
    # the draws know nothing of the edge rule, and a far entry is as good as a near one
    cfg = config(shape, edge="zero", color="random", seed=9)
    assert np.array_equal(engine_params(engine_lib, cfg, [0, 77, 2**31 - 1]), aug_params_many(config(shape, color="random", seed=9), [0, 77, 2**31 - 1]))
    assert np.array_equal(aug_params(cfg, 77), aug_params_many(cfg, [5, 77])[1])


def test_every_refusal_of_a_config(engine_lib):
    L = engine_lib
    row = (ctypes.c_int32 * 8)()
    good = dict(out_height=56, out_width=56, pad=4, edge=0, cutout_min=4, cutout_max=24, cutout_color=1, seed=1)

    def call(entry=0, out=row, size=None, params=None, **change):
        f = dict(good, **change)
        a = pglib.GatherAug(ctypes.sizeof(pglib.GatherAug) if size is None else size, f["out_height"], f["out_width"], f["pad"], f["edge"],
                            f["cutout_min"], f["cutout_max"], f["cutout_color"], f["seed"], params)
        return L.pgv_gather_aug_params(ctypes.byref(a), entry, out)

    assert call() == 0
    before = list(row)
    bad = [dict(out_height=0), dict(out_height=65), dict(out_height=-1), dict(out_width=0), dict(out_width=4), dict(out_width=12), dict(out_width=60),
           dict(out_width=72), dict(pad=-1), dict(pad=17), dict(edge=2), dict(edge=-1), dict(cutout_color=2), dict(cutout_color=-1),
           dict(cutout_min=25), dict(cutout_min=0), dict(cutout_min=-1), dict(cutout_max=65, cutout_min=65), dict(cutout_max=65),
           dict(cutout_min=-1, cutout_max=0), dict(cutout_max=-1, cutout_min=-1), dict(size=ctypes.sizeof(pglib.GatherAug) - 1), dict(size=0),
           dict(params=0x1002), dict(params=0x1001), dict(entry=-1), dict(entry=-2**31), dict(out=None)]
    for change in bad:
        assert call(**change) != 0, change
        assert b"pgv_gather_aug_params" in L.pgv_last_error(), change
        assert list(row) == before, change
    assert L.pgv_gather_aug_params(None, 0, row) != 0 and b"aug is NULL" in L.pgv_last_error()
    # the edges of every range are taken
    for change in (dict(out_height=1), dict(out_height=64), dict(out_width=8), dict(out_width=64), dict(pad=0), dict(pad=16), dict(edge=1),
                   dict(cutout_color=0), dict(cutout_min=0, cutout_max=0), dict(cutout_min=1, cutout_max=1), dict(cutout_min=64, cutout_max=64),
                   dict(params=0x1004), dict(entry=2**31 - 1)):
        assert call(**change) == 0, (change, L.pgv_last_error())


def test_what_the_configurations_reach():
    """What the GPU test relies on, on the model alone: with its seed and its 256 entries every configuration draws both ends
    of the oy range and both ends of the ox range; (3) has windows entirely outside the frame; (5) clamps every rectangle to
    the output and has rows of 8 mod 16 bytes; (6) is all cutout."""
    for shape in CONFIGS:
        H, W, pad, lo, hi = shape
        p = aug_params_many(config(shape, color="random", seed=SEED), np.arange(ENTRIES))
        assert p[:, 0].min() == -pad and p[:, 0].max() == 64 + pad - H, shape
        assert p[:, 1].min() == -pad and p[:, 1].max() == 64 + pad - W, shape
    assert windows_outside(config(CONFIGS[2])) == 94
    assert all(windows_outside(config(s)) == 0 for k, s in enumerate(CONFIGS) if k != 2)
    five = aug_params_many(config(CONFIGS[4]), np.arange(ENTRIES))
    assert (five[:, 5] == 24).all() and (five[:, 4] >= 24).all() and (63 * 24 * 3) % 16 == 8 and (63 * 24) % 16 == 8
    six = aug_params_many(config(CONFIGS[5]), np.arange(ENTRIES))
    assert (six[:, :6] == [0, 0, 0, 0, 64, 64]).all()


def test_model_by_hand():
    """The model on a ring made up by hand: the identity configuration is the plain gather; a shifted window, both edges,
    and a cutout, pixel by pixel."""
    rng = np.random.default_rng(11)
    ring = HistoryRing(2, 3, False)
    frames = rng.integers(0, 256, (4, 2, 64, 64, 3), dtype=np.uint8)
    for p in range(4):
        if p == 2:
            ring.flag(np.array([0, 1]))
        ring.push(frames[p])
    pushes, envs = [3, 3, 0, 2, 3], [0, 1, 0, 1, 2]
    plain = ring.gather(pushes, envs, 3, "float16")
    for edge in ("replicate", "zero"):
        rows, params = augment(ring, pushes, envs, 3, "float16", config((64, 64, 0, 0, 0), edge=edge, seed=123))
        assert np.array_equal(rows, plain) and not params.any()
    assert not plain[2].any() and not plain[4].any() and plain[0].any()
    for edge in ("replicate", "zero"):
        cfg = config((40, 48, 9, 5, 11), edge=edge, color="random", seed=3)
        rows, params = augment(ring, pushes, envs, 3, "uint8", cfg)
        assert rows.shape == (5, 9, 40, 48) and not rows[2].any() and not rows[4].any()
        for b in (0, 1, 3):
            oy, ox, cy, cx, ch, cw, colour, _ = (int(v) for v in params[b])
            walk = ring.walk(pushes[b], envs[b], 3)
            for s in range(3):
                stored = ring.frames[walk[2 - s] % 3][envs[b]]
                for c in range(3):
                    for y in range(0, 40, 3):
                        for x in range(0, 48, 5):
                            sy, sx = oy + y, ox + x
                            if cy <= y < cy + ch and cx <= x < cx + cw:
                                want = (colour >> (8 * c)) & 0xFF
                            elif 0 <= sy <= 63 and 0 <= sx <= 63:
                                want = stored[c, sy, sx]
                            elif edge == "zero":
                                want = 0
                            else:
                                want = stored[c, min(max(sy, 0), 63), min(max(sx, 0), 63)]
                            assert rows[b, s * 3 + c, y, x] == want, (edge, b, s, c, y, x)
    assert ring.walk(3, 1, 3) == [3, 2, 2]  # (a stack cut by the began byte went through it)


def test_pg_history_aug_on_the_host(tmp_path):
    """pg_history_aug.h under g++: the draws against a transcription, aug_source_byte_index over every pixel of every window
    the seven configurations can draw, the output offsets, a case above 2^32 bytes included."""
    exe = str(tmp_path / "test_history_aug")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "procgen2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_history_aug.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK draws", "OK source index", "OK offsets", "ALL OK"):
        assert section in out.stdout, section


def test_augment_value_errors():
    """history_gather(augment=...) refuses what it does not know before it asks for an engine."""
    from procgen2_amd.vec_env import ProcgenVecEnv, _augment_config
    good = dict(size=56, pad=4, edge="zero", cutout=(4, 24), cutout_color="random", seed=7)
    a = _augment_config(good)
    assert (a.out_height, a.out_width, a.pad, a.edge, a.cutout_min, a.cutout_max, a.cutout_color, a.seed) == (56, 56, 4, 1, 4, 24, 1, 7)
    a = _augment_config(dict(size=(33, 40), seed=0))
    assert (a.out_height, a.out_width, a.pad, a.edge, a.cutout_min, a.cutout_max, a.cutout_color, a.seed) == (33, 40, 0, 0, 0, 0, 0, 0)
    bad = [dict(good, colour="black"), {k: v for k, v in good.items() if k != "seed"}, {k: v for k, v in good.items() if k != "size"},
           dict(good, size=0), dict(good, size=65), dict(good, size=60), dict(good, size=(56,)), dict(good, size=(0, 8)), dict(good, size=(8, 4)),
           dict(good, size=(8, 72)), dict(good, size=56.0), dict(good, size=True), dict(good, size="56"), dict(good, pad=-1), dict(good, pad=17),
           dict(good, pad=1.5), dict(good, pad=None), dict(good, edge="wrap"), dict(good, edge=0), dict(good, cutout=(0, 4)), dict(good, cutout=(5, 4)),
           dict(good, cutout=(1, 65)), dict(good, cutout=8), dict(good, cutout=(1, 2, 3)), dict(good, cutout=(1.0, 2)), dict(good, cutout_color="white"),
           dict(good, cutout_color=1), dict(good, seed=-1), dict(good, seed=2**32), dict(good, seed=1.0), dict(good, seed=None), dict(good, seed=True),
           [("size", 56)], "crop"]
    for augment_arg in bad:
        with pytest.raises(ValueError):
            _augment_config(augment_arg)
    # … and history_gather itself raises them first: on an object that has no engine behind it at all
    v = ProcgenVecEnv.__new__(ProcgenVecEnv)
    v.history = None
    for augment_arg in bad[:6]:
        with pytest.raises(ValueError):
            v.history_gather([0], [0], augment=augment_arg)
    with pytest.raises(ValueError):
        v.history_gather([0], [0], return_params=True)
    with pytest.raises(pglib.EngineError):
        v.history_gather([0], [0], augment=good)
