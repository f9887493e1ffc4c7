#!/usr/bin/env python3
"""What the lock-step protocols reach, counted on the CPU oracle alone (no GPU, no frames):

    python tools/event_census.py [--out profiles/scripted_play/event_census.md]

Random play: the protocol of tests/variant_paths_util.py without its masked resets — 131 envs, seed_base 17,
pgo_synthetic_action(9, step, env), 200 steps (maze 520, jumper-memory 400) — for all 18 (game, mode) pairs: episodes ended,
how many of them with a positive reward in their last step, the rewards seen; for caveflyer the most live bullets and the
env-steps that draw more things than the render wave has lanes, for coinrun the median and the 90th percentile of
agent_x / coin_x over the env-steps and the deaths in lava, for every game the most episodes one env ended.  Scripted play:
the protocol of tests/scripted_play_util.py for all seven games, with the counts its floors are set on.
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
    """(steps, ended, ended with a positive reward, the non-zero rewards seen, bossfight's phases or None, caveflyer's
    (most live bullets, env-steps with more draws than lanes) or None, coinrun's (median progress, its 90th percentile, deaths
    in lava) or None, the most episodes one env ended)."""
    steps = vp.steps_of(game, mode)
    ora = OracleVec(game, vp.N, seed_base=vp.SEED_BASE, render=False, mode=mode)
    resetting = np.zeros(vp.N, bool)
    ended = won = 0
    seen, phases = set(), set()
    column = sp.columns(game, mode).f["phase_index"] if game == "bossfight" else None
    cave = sp.Counter(game, mode, vp.N) if game == "caveflyer" else None
    coin = sp.Counter(game, mode, vp.N) if game == "coinrun" else None
    most_shots = overflows = lava = 0
    progress, env_ends = [], np.zeros(vp.N, int)
    for s in range(steps):
        _, reward, done = ora.step(vp.actions(s))
        fresh = (done != 0) & ~resetting  # (an env's step after its last is its reset step: the engine's auto-reset)
        ended += int(fresh.sum())
        env_ends += fresh
        if coin is not None:
            dumps = sp.Dumps(ora, coin.c)
            progress += coin.coinrun_progress(dumps)[~resetting].tolist()
            lava += sum(coin.coinrun_death(dumps.states[e], dumps.tiles[e]) == "lava" for e in np.nonzero(fresh & (reward < 10))[0])
        won += int((fresh & (reward > 0)).sum())
        seen |= set(np.unique(reward[~resetting & (reward != 0)]).tolist())
        if cave is not None:
            dumps = sp.Dumps(ora, cave.c)
            most_shots = max([most_shots] + dumps.states[~resetting, cave.c.f["s_count"]].astype(int).tolist())
            overflows += int((cave.caveflyer_overflow(dumps) & ~resetting).sum())
        resetting = done != 0
        if column is not None and s % 4 == 0:
            phases |= {int(ora.state(e, column + 1)[column]) for e in range(vp.N)}
    ora.close()
    return (steps, ended, won, seen, phases or None, (most_shots, overflows) if cave is not None else None,
            ("%.2f" % np.median(progress), "%.2f" % np.percentile(progress, 90), lava) if coin is not None else None, int(env_ends.max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the tables to this file")
    args = ap.parse_args()
    lines = ["# Event census: what the lock-step protocols reach on the oracle", "",
             "## Random play (tests/variant_paths_util.py: %d envs, seed_base %d, pgo_synthetic_action(%d, step, env), no masked resets)" %
             (vp.N, vp.SEED_BASE, vp.RUN_SEED), "",
             "| game | mode | steps | episodes ended | ended with a positive reward | non-zero rewards seen | bossfight phases "
             "| caveflyer: most live bullets | caveflyer: overflow env-steps | coinrun: median agent_x / coin_x | coinrun: its 90th percentile "
             "| coinrun: deaths in lava | most episodes ended in one env |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for game, mode in vp.PAIRS:
        steps, ended, won, seen, phases, cave, coin, deepest = random_play(game, mode)
        lines.append("| %s | %d | %d | %d | %d | %s | %s | %s | %s | %s | %s | %s | %d |" %
                     ((game, mode, steps, ended, won, rewards_seen(seen) or "none", "" if phases is None else sorted(phases))
                      + (("", "") if cave is None else cave) + (("", "", "") if coin is None else coin) + (deepest,)))
        print(lines[-1], flush=True)
    lines += ["", "## Scripted play (tests/scripted_play_util.py: %d envs, seed_base %d, the agents' actions, no masked resets)" % (sp.N, sp.SEED_BASE), "",
              "| game | mode | steps | episodes ended | won | lost | the rest of the counts |", "|---|---|---|---|---|---|---|"]
    for game, mode in sp.PAIRS:
        t = time.time()
        k = sp.run_on_oracle(game, mode)
        rest = ", ".join("%s %s" % (name, sorted(v) if isinstance(v, set) else ("%.3f" % v if isinstance(v, float) else v))
                         for name, v in k.items() if name not in ("wins", "deaths", "ends"))
        lines.append("| %s | %d | %d | %d | %d | %d | %s |" % (game, mode, sp.STEPS[(game, mode)], k["ends"], k["wins"], k["deaths"], rest))
        print(lines[-1], "%.1f s" % (time.time() - t), flush=True)  # (the seconds stay out of the file: it is reproduced byte for byte)
        sp.assert_covers(game, mode, k)
        if (game, mode) == ("jumper", sp.MEMORY):
            memory = k
        assert game != "caveflyer" or not (k["double_target_steps"] or k["goal_with_target_steps"]), "rewrite the closing lines"
    lines += ["", "coinrun, jumper and maze are played now.  The holes still open: no caveflyer step destroys two targets (a reward of 6) or",
              "reaches the goal with a target (13), and no bullet of the cast meets an enemy and a target at once, so the hazard order that",
              "decides between them is held by no run; chaser extreme clears no board (`available == 0`).  jumper's memory mode ending",
              "\"never by a spike\" was named a hole and is none: `spike_prob` is 0 in memory mode (`oracle/pgo_jumper.cpp`), the mode has no",
              "spikes, and the scripted run asserts exactly 0 such deaths.  What the new casts do not reach: coinrun's entity sets keep",
              "their bucket arrays from level to level, and an oracle changed to start every level with fresh sets draws the same frames",
              "as the good one for the whole 300 steps of the cast — under the same agents it first parts at step 631 (env 26, frames only:",
              "the order of overlapping sprites), past the 600-step cap, and in five envs of 65 within 1 500 steps; in jumper's memory mode",
              "%d of 65 envs end no episode within the run and %d first steps of a fourth or later level are met; maze's 500-step cap is" %
              (memory["envs_with_no_end"], memory["deep_starts"]),
              "left to the variant-path protocol.", ""]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
