"""The protocols of tests/test_variant_paths_gpu.py, stated once: the GPU half runs them on the HIP engine beside the oracle,
tests/test_variant_paths.py runs them on the oracle alone and asserts that they cover the ground (auto-resets served, maze
envs ending at the step cap together), so the GPU tests are known not to be vacuous before a GPU is touched.

Lock-step protocol: n = 131 envs (two full wavefronts and three lanes; prime, so a multiple of no gang width, of no
envs-per-block count and of no pre-pass group; env 130 sits in a wave of its own), seed_base 17, explicit actions
pgo_synthetic_action(9, step, env), masked resets after steps 60, 61 (no seeds: the env's stream goes on) and 110 (a seeds
array with a negative entry), state dumps of the envs at the wavefronts' edges after steps 0, 59, 62, 111 and the last.

maze differs in one place.  Its cases run 520 steps so that the envs no reset touched reach the 500-step cap together, and
at least 30 must do so in one step.  With resets after steps 60 and 61 the masks (i + s) % 3 == 0 name two different thirds,
35 envs stay untouched, and only 22 / 24 / 29 of them (easy / hard / memory, on the oracle) are still in their first maze
at step 499.  So in maze the second unseeded reset comes after step 63, where the same formula names the first third
again: 70 envs stay untouched and 40 / 48 / 58 end together at step 499 (184 / 140 / 120 auto-resets in all); maze is
dumped after step 64 as well.
"""
import numpy as np

from episodes_util import synthetic_actions
from test_modes import EASY, EXTREME, HARD, MEMORY, NON_DEFAULT, TABLE  # noqa: F401

PAIRS = sorted((g, m) for g, (_, ms) in TABLE.items() for m in ms)  # all 18, the defaults by their own number
N, SEED_BASE, RUN_SEED = 131, 17, 9
DUMP_ENVS = (0, 1, 63, 64, 65, 127, 128, 130)
MIN_ENDS = 10       # auto-resets a case serves, at least
MIN_CAP_ENDS = 30   # maze: envs that end at the 500-step cap in one step, at least

# pgv_set_debug bits (procgen2_amd/csrc/engine.hip pgv_set_debug)
REPLAY, NO_PREFETCH, NO_PRE_PASS, HAND_BACK, HAZARDS_LONG, ENEMIES_SERIAL = 1, 1 << 8, 1 << 21, 1 << 23, 1 << 24, 1 << 25
PATH_NAMES = {0: "default", REPLAY: "draw-list replay (bit 0)", NO_PREFETCH: "levels generated inside the step (bit 8)",
              NO_PRE_PASS: "complete render path (bit 21)", HAND_BACK: "frames the pre-pass hands back (bit 23)",
              HAZARDS_LONG: "hazards the long way (bit 24)", ENEMIES_SERIAL: "enemies one after the other (bit 25)"}


def paths(game):
    """The debug words a game's engines run with, side by side."""
    out = [0, REPLAY, NO_PREFETCH, NO_PRE_PASS]
    if game in ("coinrun", "climber", "caveflyer", "jumper"):
        out.append(HAND_BACK)
    if game == "coinrun":
        out.append(HAZARDS_LONG)
    if game == "chaser":
        out.append(ENEMIES_SERIAL)
    return out


def steps_of(game, mode):
    """maze: past the 500-step cap, so the envs no reset touched run into it together; jumper-memory ends rarely."""
    return 520 if game == "maze" else 400 if (game, mode) == ("jumper", MEMORY) else 200


def second_reset_after(game):
    return 63 if game == "maze" else 61


def dump_after(game, mode):
    return (0, 59, 62, 111, steps_of(game, mode) - 1) + ((64,) if game == "maze" else ())


def actions(step, n=N):
    return synthetic_actions(RUN_SEED, step, n)


def masked_reset_after(game, step, n=N):
    """(mask, seeds) of the masked reset that follows `step`, or None."""
    i = np.arange(n)
    if step in (60, second_reset_after(game)):
        return ((i + step) % 3 == 0).astype(np.uint8), None
    if step == 110:
        return (i % 5 == 2).astype(np.uint8), (i * 7 - 5).astype(np.int32)
    return None


def run_on_oracle(game, mode, each_step=None, each_reset=None, at_start=None, render=False, threads=1):
    """The lock-step protocol on an OracleVec.  at_start(ora) before the first step, each_step(s, ora, actions, obs, reward,
    done) after every step, each_reset(s, ora, mask, seeds, obs) after every masked reset.  Returns (auto-resets served, most
    envs ended in one step at or past step 499)."""
    from oracle_util import OracleVec
    ora = OracleVec(game, N, seed_base=SEED_BASE, render=render, mode=mode, threads=threads)
    ends = cap_ends = 0
    try:
        if at_start:
            at_start(ora)
        for s in range(steps_of(game, mode)):
            a = actions(s)
            obs, reward, done = ora.step(a, threads=threads)
            ends += int((done != 0).sum())
            if s >= 499:
                cap_ends = max(cap_ends, int((done != 0).sum()))
            if each_step:
                each_step(s, ora, a, obs, reward, done)
            m = masked_reset_after(game, s)
            if m is not None:
                obs = ora.reset(mask=m[0], seeds=m[1])
                if each_reset:
                    each_reset(s, ora, m[0], m[1], obs)
    finally:
        ora.close()
    return ends, cap_ends


def assert_covers(game, mode, ends, cap_ends):
    assert ends >= MIN_ENDS, "%s mode %d serves only %d auto-resets" % (game, mode, ends)
    assert game != "maze" or cap_ends >= MIN_CAP_ENDS, "maze mode %d: at most %d envs end at the cap in one step" % (mode, cap_ends)


# test_variants_at_one_and_65_envs: 80 steps, one unseeded masked reset of env 0 after step 40
SMALL_NS, SMALL_STEPS, SMALL_RESET_AFTER = (1, 65), 80, 40
SMALL_PATHS = (0, NO_PRE_PASS)

# test_same_step_with_a_limit_in_every_variant (tests/test_episodes_gpu.py)
EPISODE_N, EPISODE_LIMIT, EPISODE_RING, EPISODE_STEPS, EPISODE_RUN_SEED = 131, 23, 4, 70, 7


def run_limit_case(model, eng=None, check_step=None, n=EPISODE_N, steps=EPISODE_STEPS, run_seed=EPISODE_RUN_SEED):
    """Case 3 of tests/test_episodes_gpu.py as it stands — three plain steps, each followed by a masked reset of another
    third, then step_episodes — on the model alone or on an engine beside it.  Returns (terminated, truncated, steps that
    overflow the ring, the fewest endings any env had)."""
    t = 0
    for third in range(3):
        a = synthetic_actions(run_seed, t, n)
        mask = (np.arange(n) % 3 == third).astype(np.uint8)
        want = model.plain_step(a)
        if eng is not None:
            obs, reward, done = eng.plain_step(a)
            assert np.array_equal(obs, want[0]) and np.array_equal(done, want[2])
            assert np.array_equal(eng.reset(mask), model.reset(mask))
        else:
            model.reset(mask)
        t += 1
    terminated = truncated = overflows = 0
    ended = np.zeros(n, int)
    for _ in range(steps):
        a = synthetic_actions(run_seed, t, n)
        got = eng.step(a) if eng is not None else None
        model.step(a)
        if eng is not None:
            check_step(eng, model, got, t)
            c = int(got["counts"][0])
            assert int(got["counts"][1]) == min(c, model.capacity)
            assert c == 0 or got["ended_length"][:c].max() <= model.T
        terminated += int(model.terminated.sum())
        truncated += int(model.truncated.sum())
        overflows += int(model.counts[0] > model.capacity)
        ended += model.ended != 0
        t += 1
    assert model.longest <= model.T
    return terminated, truncated, overflows, int(ended.min())


def assert_limit_case_covers(terminated, truncated, overflows, fewest):
    """Every env's level is generated at least twice by the masked-reset install.  (terminated > 0 is not asked for: chaser
    cannot end a game in 23 steps.)"""
    assert truncated > 0 and overflows >= 1 and fewest >= 2, (terminated, truncated, overflows, fewest)
