"""Per-env state records (pgv_save_envs / pgv_load_envs): what can be checked without a GPU.

The plan of tests/test_env_records_gpu.py — which envs go into the foreign engines, which windows are replayed — is made
from the oracle's dones alone; here it is shown not to be vacuous for any case.  Plus the ABI's bookkeeping: the header
documents every new symbol, lib.py declares it, the library exports it."""
import os
import re

import numpy as np
import pytest

from test_snapshot import CASES, N, Case, _check_plan, oracle_dones, snapshot_plan

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_SYMBOLS = ["pgv_env_record_bytes", "pgv_env_record_tag", "pgv_save_envs", "pgv_load_envs", "pgv_save_envs_host",
                  "pgv_load_envs_host"]
FOREIGN_N, PARTIAL = 77, 40  # envs of a foreign engine; how many of them are loaded at P0 and P3
REWIND_IDS = ("coinrun", "maze", "bossfight", "climber", "caveflyer", "chaser", "jumper", "chaser-float_abs", "coinrun-levels7",
              "bossfight-levels7")
PREFETCH_GAMES = {"coinrun": 330, "maze": 560, "jumper": 330}  # game: steps of the run with prefetch off on one side
PREFETCH_N, PREFETCH_AT = 64, 120


def chosen_envs(dones, s, count):
    """The `count` envs that leave the batch after step s (-1: after the reset), from the oracle's dones alone: first the
    envs whose episode ended in step s (their reset is pending), then those whose episode ends anywhere later in the run,
    then the lowest-numbered rest."""
    n = dones.shape[1]
    ended = np.nonzero(dones[s])[0] if s >= 0 else np.zeros(0, np.int64)
    later = np.nonzero(dones[s + 1:].any(axis=0))[0]
    order = list(ended) + [e for e in later if e not in set(ended)]
    order += [e for e in range(n) if e not in set(order)]
    return np.array(order[:count], np.int64)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_the_choice_of_moved_envs_holds_on_the_oracle(case):
    dones = oracle_dones(case)
    plan = snapshot_plan(case, dones)
    _check_plan(case, dones, plan)
    for s, names in sorted(plan.items()):
        chosen = chosen_envs(dones, s, FOREIGN_N)
        assert len(set(chosen)) == FOREIGN_N
        pending = int(dones[s][chosen].sum()) if s >= 0 else 0
        later = int(dones[s + 1:, chosen].sum())
        print("%s %s (after step %d): %d of the %d chosen envs carry a pending reset, %d episodes end among them later"
              % (case.id, "+".join(names), s, pending, FOREIGN_N, later))
        assert later >= 1
        if s >= 0 and set(names) & {"P1", "P2", "P3"}:
            assert pending >= 1 and pending == min(FOREIGN_N, int(dones[s].sum()))
        if set(names) & {"P0", "P3"}:  # (the first 40 are the ones loaded there)
            assert dones[s + 1:, chosen[:PARTIAL]].any()
    if case.id in REWIND_IDS:
        for name, length in (("P1", 51), ("P3", 52)):
            s = next(s for s, names in plan.items() if name in names)
            ends = int(dones[s + 1:s + 1 + length].sum())
            print("%s: %d episodes end in the %d steps after %s" % (case.id, ends, length, name))
            assert ends >= 1 and s + length < case.steps


def test_the_rewind_cases_exist():
    assert set(REWIND_IDS) <= {c.id for c in CASES}


@pytest.mark.parametrize("game", sorted(PREFETCH_GAMES))
def test_episodes_end_after_the_records_move_between_prefetch_settings(game):
    dones = oracle_dones(Case(game), n=PREFETCH_N)
    after = int(dones[PREFETCH_AT + 1:PREFETCH_GAMES[game]].sum())
    print("%s: %d episodes end in steps %d … %d" % (game, after, PREFETCH_AT + 1, PREFETCH_GAMES[game] - 1))
    assert after >= 1


def test_prototypes_and_exports(engine_lib):
    for name in RECORD_SYMBOLS:
        assert name in pglib.EXPORTED_VEC_SYMBOLS, name
        fn = getattr(engine_lib, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    import ctypes
    assert engine_lib.pgv_env_record_tag.restype is ctypes.c_uint64 and engine_lib.pgv_env_record_bytes.restype is ctypes.c_int64
    assert engine_lib.pgv_load_envs.argtypes[-1] is ctypes.c_uint64 and len(engine_lib.pgv_load_envs.argtypes) == 5
    # no env, no GPU: the calls fail with a message instead of touching anything
    assert engine_lib.pgv_env_record_bytes(None) == -1 and engine_lib.pgv_env_record_tag(None) == 0
    assert engine_lib.pgv_save_envs(None, None, 1, None) != 0 and b"NULL" in engine_lib.pgv_last_error()
    assert engine_lib.pgv_load_envs_host(None, None, 0, None, 1) != 0


def test_the_header_documents_every_record_symbol():
    text = open(os.path.join(ROOT, "include", "procgen2_vec.h")).read()
    for name in RECORD_SYMBOLS:
        assert re.search(r"PGV_API\s+u?int(32|64)_t\s+%s\s*\(" % name, text), name
    doc = text[text.index("Per-env state records"):text.index("pgv_load_envs_host")]
    for word in ("transparent", "any slot", "untouched", "byte-equal", "does NOT travel", "distinct", "marked empty", "16-byte",
                 "not synchronised", "tag"):
        assert word in doc, word


def test_vec_env_has_the_record_surface():
    from procgen2_amd import vec_env
    for name in ("env_record_bytes", "env_record_tag", "save_envs", "load_envs", "fork"):
        assert hasattr(vec_env.ProcgenVecEnv, name), name
    import torch
    rec = vec_env.EnvRecords(torch.arange(64, dtype=torch.uint8).reshape(4, 16), 77)
    assert len(rec) == 4 and rec[1:3].tag == 77 and rec[torch.tensor([3, 0])].data[0, 0] == 48 and len(rec[2]) == 1
    assert rec[-1].data[0, 0] == 48 and rec[1:3].data.data_ptr() == rec.data[1:3].data_ptr()
