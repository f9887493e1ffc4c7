#!/usr/bin/env python3
"""What the lock-step protocols reach, counted on the CPU oracle alone (no GPU, no frames):

    python tools/event_census.py [--out profiles/scripted_play/event_census.md]

Random play: the protocol of tests/variant_paths_util.py without its masked resets — 131 envs, seed_base 17,
pgo_synthetic_action(9, step, env), 200 steps (maze 520, jumper-memory 400) — for all 18 (game, mode) pairs: episodes ended,
how many of them with a positive reward in their last step, the rewards seen.  Scripted play: the protocol of
tests/scripted_play_util.py for bossfight, chaser and climber, with the counts its floors are set on.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scripted_play_util as sp  # noqa: E402
import variant_paths_util as vp  # noqa: E402
from oracle_util import OracleVec  # noqa: E402


def rewards_seen(values):
    values = sorted(values)
    shown = ", ".join("%g" % v for v in values[:6])
    return shown + (", … (%d values)" % len(values) if len(values) > 6 else "")


def random_play(game, mode):
    """(steps, ended, ended with a positive reward, the non-zero rewards seen, bossfight's phases or None)."""
    steps = vp.steps_of(game, mode)
    ora = OracleVec(game, vp.N, seed_base=vp.SEED_BASE, render=False, mode=mode)
    resetting = np.zeros(vp.N, bool)
    ended = won = 0
    seen, phases = set(), set()
    column = sp.columns(game, mode).f["phase_index"] if game == "bossfight" else None
    for s in range(steps):
        _, reward, done = ora.step(vp.actions(s))
        fresh = (done != 0) & ~resetting  # (an env's step after its last is its reset step: the engine's auto-reset)
        ended += int(fresh.sum())
        won += int((fresh & (reward > 0)).sum())
        seen |= set(np.unique(reward[~resetting & (reward != 0)]).tolist())
        resetting = done != 0
        if column is not None and s % 4 == 0:
            phases |= {int(ora.state(e, column + 1)[column]) for e in range(vp.N)}
    ora.close()
    return steps, ended, won, seen, phases or None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the tables to this file")
    args = ap.parse_args()
    lines = ["# Event census: what the lock-step protocols reach on the oracle", "",
             "## Random play (tests/variant_paths_util.py: %d envs, seed_base %d, pgo_synthetic_action(%d, step, env), no masked resets)" %
             (vp.N, vp.SEED_BASE, vp.RUN_SEED), "",
             "| game | mode | steps | episodes ended | ended with a positive reward | non-zero rewards seen | bossfight phases |", "|---|---|---|---|---|---|---|"]
    for game, mode in vp.PAIRS:
        steps, ended, won, seen, phases = random_play(game, mode)
        lines.append("| %s | %d | %d | %d | %d | %s | %s |" % (game, mode, steps, ended, won, rewards_seen(seen) or "none",
                                                             "" if phases is None else sorted(phases)))
        print(lines[-1], flush=True)
    lines += ["", "## Scripted play (tests/scripted_play_util.py: %d envs, seed_base %d, the agents' actions, no masked resets)" % (sp.N, sp.SEED_BASE), "",
              "| game | mode | steps | episodes ended | won | lost | the rest of the counts | seconds |", "|---|---|---|---|---|---|---|---|"]
    for game, mode in sp.PAIRS:
        t = time.time()
        k = sp.run_on_oracle(game, mode)
        rest = ", ".join("%s %s" % (name, sorted(v) if isinstance(v, set) else ("%.3f" % v if isinstance(v, float) else v))
                         for name, v in k.items() if name not in ("wins", "deaths", "ends"))
        lines.append("| %s | %d | %d | %d | %d | %d | %s | %.1f |" % (game, mode, sp.STEPS[(game, mode)], k["ends"], k["wins"], k["deaths"], rest, time.time() - t))
        print(lines[-1], flush=True)
        sp.assert_covers(game, mode, k)
    lines += ["", "The next hole: caveflyer's target reward (3.0) is rare in the random census above and absent from easy mode; no agent",
              "plays caveflyer yet.", ""]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
