"""tests/bench_replay.py's checker, without a GPU: dumps in bench.py --dump-outputs' format made by the oracle itself
(2 048 envs, more than bench.DUMP_OBS_ENVS, so that the checker replays a sample of the rows as it does at 65 536) must
pass, and each kind of damage to them must fail."""
import os
import sys

import numpy as np
import pytest

from bench_replay import check_dump, mixed_blocks, row_env
from oracle_util import OracleVec

from procgen2_amd import lib as pglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

GAME, MODE, N, STEPS = "bossfight", "easy", 2048, 48


def _run_oracle(game, n, steps, mode=None):
    """What the last of `steps` steps of a bench run of `n` envs of `game` hands its caller, by the oracle drawing every
    step as the engine does, and how many episode ends each env had on the way."""
    threads = bench.usable_cores()
    ora = OracleVec(game, n, seed_base=1, mode=pglib.mode_id(mode), threads=threads)
    ends = np.zeros(n, np.int64)
    for _ in range(steps):
        obs, reward, done = ora.step(None, run_seed=0, threads=threads)
        ends += done
    out = obs.copy(), reward.copy(), done.copy(), ends
    ora.close()
    return out


def _write(directory, obs, reward, done):
    import torch
    bench.dump_outputs(str(directory), torch.from_numpy(obs.reshape(-1, 64, 64, 3)), torch.from_numpy(reward),
                       torch.from_numpy(done))
    return str(directory)


@pytest.fixture(scope="module")
def single():
    """Envs 0 .. N of GAME in MODE: one more than a dump holds, for the dump of the envs one further on."""
    return _run_oracle(GAME, N + 1, STEPS, MODE)


@pytest.fixture(scope="module")
def mixed():
    """The mixed workload's slab of N envs: every game's block from its own oracle vector, as bench.py lays it out."""
    parts = [_run_oracle(game, count, STEPS) for game, _, count in mixed_blocks(N)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def test_mixed_blocks_are_bench_layout():
    blocks = mixed_blocks(65536)
    assert [c for _, _, c in blocks] == [9362] * 6 + [9364]
    assert [at for _, at, _ in blocks] == [9362 * k for k in range(7)]
    assert row_env("mixed", 65536, 9362 * 5 - 1) == (blocks[4][0], 9361)
    assert row_env("mixed", 65536, 65535) == ("jumper", 9363) and row_env("maze", 65536, 700) == ("maze", 700)


def test_checker_passes_a_true_dump_and_counts_its_episode_ends(single, tmp_path):
    obs, reward, done, ends = (x[:N] for x in single)
    rows = bench.dump_rows(N, bench.DUMP_OBS_ENVS)
    ended = int((ends[rows] > 0).sum())
    assert rows.size == 1024 and 0 < ended < rows.size, ended
    assert check_dump(_write(tmp_path, obs, reward, done), GAME, N, STEPS, mode=MODE) == (rows.size, ended)


def _damage(kind, single):
    """A dump of `single` with one kind of damage, and what the checker's message must name."""
    obs, reward, done = (x[:N].copy() for x in single[:3])
    rows = bench.dump_rows(N, bench.DUMP_OBS_ENVS)
    row = int(rows[rows.size // 3])  # an env whose observation is dumped
    if kind == "obs byte":
        obs[row, 4321] ^= 1
        return (obs, reward, done), "row %d .*obs \\(1 bytes\\)" % row
    if kind == "reward ulp":
        reward[row] = np.nextafter(reward[row], np.float32(np.inf))
        return (obs, reward, done), "row %d .*reward" % row
    if kind == "done flipped":
        done[row] ^= 1
        return (obs, reward, done), "row %d .*done" % row
    assert kind == "rows shifted"
    return tuple(x[1:N + 1] for x in single[:3]), "differ from the oracle"


@pytest.mark.parametrize("kind", ["obs byte", "reward ulp", "done flipped", "rows shifted"])
def test_checker_fails_a_damaged_dump(single, tmp_path, kind):
    arrays, message = _damage(kind, single)
    with pytest.raises(AssertionError, match=message):
        check_dump(_write(tmp_path, *arrays), GAME, N, STEPS, mode=MODE)


@pytest.mark.parametrize("steps,mode", [(STEPS - 1, MODE), (STEPS + 1, MODE), (STEPS, None)],
                         ids=["one step short", "one step over", "default mode"])
def test_checker_fails_a_true_dump_of_another_run(single, tmp_path, steps, mode):
    directory = _write(tmp_path, *(x[:N] for x in single[:3]))
    with pytest.raises(AssertionError, match="differ from the oracle"):
        check_dump(directory, GAME, N, steps, mode=mode)


def test_checker_passes_a_true_mixed_dump(mixed, tmp_path):
    obs, reward, done, ends = mixed
    rows = bench.dump_rows(N, bench.DUMP_OBS_ENVS)
    games = {row_env("mixed", N, int(r))[0] for r in rows}
    assert len(games) == 7  # every block has rows in the sample
    ended = int((ends[rows] > 0).sum())
    assert check_dump(_write(tmp_path, obs, reward, done), "mixed", N, STEPS) == (rows.size, ended) and ended > 0


def test_checker_fails_a_mixed_dump_with_two_blocks_swapped(mixed, tmp_path):
    (first, a, count), (second, b, count_b) = mixed_blocks(N)[:2]
    assert count == count_b
    swapped = []
    for x in mixed[:3]:
        x = x.copy()
        x[a:a + count], x[b:b + count] = x[b:b + count].copy(), x[a:a + count].copy()
        swapped.append(x)
    with pytest.raises(AssertionError, match="(%s|%s) env" % (first, second)):
        check_dump(_write(tmp_path, *swapped), "mixed", N, STEPS)
