"""The early-end protocol of tests/test_coinrun_lean_gpu.py, and its deaths counted on the oracle alone (no GPU, nothing drawn):
tests/test_coinrun_resources.py holds the protocol to its floor without a GPU, the GPU tests assert it again before they run."""
import numpy as np

from episodes_util import synthetic_actions
from oracle_util import OracleVec

DEATH_N, DEATH_STEPS, DEATH_SEED, DEATH_RUN = 512, 120, 1, 0


def death_steps(n=DEATH_N, steps=DEATH_STEPS, seed_base=DEATH_SEED, run_seed=DEATH_RUN):
    """On the oracle alone, without drawing: per step, the envs that die in it (done, reward 0)."""
    ora = OracleVec("coinrun", n, seed_base=seed_base, render=False)
    died = []
    for s in range(steps):
        _, r, d = ora.step(synthetic_actions(run_seed, s, n))
        died.append(np.nonzero((d != 0) & (r == 0.0))[0])
    ora.close()
    return died


def early_end(before, after):
    """Did the step between two state dumps of one env (oracle/pgo_coinrun.cpp dump_state: 14 floats, then x, y, vx, frame,
    anim_t per entity) end before its fourth sub-step?  An entity's anim_t gains 0.25 a sub-step and drops by its period when
    it passes it (1 for a saw, 5 for a mob; the coin's stays 0), so a whole step moves it by 0, 1 or -4 and an early end by
    something else.  (An env with no saw and no mob cannot tell: counted as not early.)"""
    d = after[14:][4::5] - before[14:][4::5]
    return bool(np.any(np.min(np.abs(d[:, None] - np.array([0.0, 1.0, -4.0], np.float32)[None, :]), axis=1) > 0.01))


def early_deaths(died, n=DEATH_N, seed_base=DEATH_SEED, run_seed=DEATH_RUN):
    """Of the deaths death_steps found, per step the envs whose step ended before its last sub-step: the redo case."""
    ora = OracleVec("coinrun", n, seed_base=seed_base, render=False)
    early = []
    for s, envs in enumerate(died):
        before = {e: ora.state(e) for e in envs}
        ora.step(synthetic_actions(run_seed, s, n))
        early.append(np.array([e for e in envs if early_end(before[e], ora.state(e))], np.int64))
    ora.close()
    return early
