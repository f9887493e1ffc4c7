#!/usr/bin/env python3
"""Where the protocol "churn, then play" (tests/chain_util.py) tells carried containers from fresh ones, counted on the CPU
oracle alone (no GPU):

    python tools/chain_census.py [--rounds R] [--play P] [--games coinrun,jumper] [--out profiles/chain/census.md]

For every (game, mode) pair the protocol runs on the good oracle and on the fresh-containers one
(OracleVec.set_fresh_containers) side by side, 65 envs, frames drawn.  Per pair: the depth the churn reaches, the call at
which anything first differs, the env-steps that differ split into frames, state rows, rewards and dones, the envs they lie
in, and the call at which 20 differing env-steps in 5 envs are first met — what the R and P in chain_util.CASES are set on.
Without --rounds / --play a pair that is in CASES runs at its own R and P, every other at the defaults below.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chain_util as cu  # noqa: E402
import variant_paths_util as vp  # noqa: E402

DEFAULT_R, DEFAULT_P = 44, 200
NAMES = {1: "easy", 2: "hard", 3: "memory", 4: "extreme"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int)
    ap.add_argument("--play", type=int)
    ap.add_argument("--games", default="")
    ap.add_argument("--cast", action="store_true", help="play under the agents of tests/scripted_play_util.py")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out")
    args = ap.parse_args()
    games = set(args.games.split(",")) if args.games else None
    lines = ["| game, mode | kept | R | P | depth after churn: min / median / max | reseeding resets | auto-resets | first difference | "
             "frames | state | reward | done | env-steps that differ | envs | 20 in 5 envs met at | s |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for game, mode in vp.PAIRS:
        if games and game not in games:
            continue
        R, P, cast = cu.CASES.get((game, mode), (DEFAULT_R, DEFAULT_P, False))
        R, P, cast = args.rounds or R, args.play or P, cast or args.cast
        t0 = time.time()
        w, churned, end, ends = cu.compare_oracles(game, mode, R, P, threads=args.threads, cast=cast)
        firsts = [v for v in w.first.values() if v is not None]
        first = "none" if not firsts else "%s (env %d)" % min(firsts, key=lambda f: (f[0].startswith("step"), int(f[0].split()[1])))
        line = "| %s %s | %s | %d | %d%s | %d / %g / %d | %d | %d | %s | %d | %d | %d | %d | %d | %d | %s | %.1f |" % (
            game, NAMES[mode], "yes" if (game, mode) in cu.CASES else "no", R, P, ", cast" if cast else "", churned.depth.min(), churned.median(),
            churned.depth.max(), churned.reseeding, ends, first, w.count["frames"], w.count["state"], w.count["reward"],
            w.count["done"], w.env_steps, w.envs, w.met_at or "never", time.time() - t0)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
