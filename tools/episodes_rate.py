#!/usr/bin/env python
"""What the episode bookkeeping on the device costs a step (include/procgen2_vec.h pgv_step_episodes).

Per game, at --envs envs (65 536), after --warmup steps (>= 64: levels prefetched, episodes spread out), milliseconds a
step of
    (a) pgv_step_synthetic                                        the engine as it was
    (b) pgv_step_episodes_synthetic, NEXT_STEP                    + the three episode launches
    (c) … SAME_STEP, no limit                                     + the masked reset, pre-pass and render of the ended envs
    (d) … SAME_STEP, max_episode_steps 1000, final_capacity 1024
each in an engine of its own (episodes are enabled once per engine), measured the same way: two HIP events on the env's
stream round --steps back-to-back calls with nothing else in the region, --repeats times, the median.  Beside them `episode_us`:
the two episode launches behind the step alone, bracketed by events inside the step (pgv_step_episodes_times; the median
over the steps) — events inside a region slow it, so this run is separate and is not part of (b) .. (d).

    python tools/episodes_rate.py [--games coinrun chaser] [--json out.json]
    python tools/episodes_rate.py --baseline-only      # (a) alone: needs nothing but the entry points the parent commit has
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("a_step", None, 0, 0), ("b_next_step", "next_step", 0, 0), ("c_same_step", "same_step", 0, 0),
            ("d_same_step_limit", "same_step", 1000, 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", nargs="*", default=None)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=96)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--order", default="abcd", help="the variants to run and their order, e.g. adcb (the table needs all four)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.warmup < 64:
        ap.error("--warmup must be at least 64")
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import GAMES, ProcgenVecEnv

    rows = []
    for game in a.games or GAMES:
        row = {"game": game, "envs": a.envs, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup}
        for name, mode, limit, capacity in VARIANTS[:1] if a.baseline_only else [VARIANTS["abcd".index(c)] for c in a.order]:
            more = {} if mode is None else {"autoreset_mode": mode, "max_episode_steps": limit, "final_obs_capacity": capacity}
            env = ProcgenVecEnv(game, a.envs, seed_base=1, **more)
            L, h, st = env.L, env._h, env._stream
            call = L.pgv_step_synthetic if mode is None else L.pgv_step_episodes_synthetic
            what = "pgv_step_synthetic" if mode is None else "pgv_step_episodes_synthetic"
            env.reset()
            for _ in range(a.warmup):
                pglib.check(L, call(h, a.run_seed), what)
            env.sync()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.steps):
                    pglib.check(L, call(h, a.run_seed), what)
                e1.record(st)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.steps)
            row[name + "_ms"] = statistics.median(ms)
            row[name + "_ms_min"], row[name + "_ms_max"] = min(ms), max(ms)
            if mode is not None:
                step_ms, episode_ms = env.step_episodes_times(a.steps, a.run_seed)
                row[name + "_episode_us"] = 1e3 * float(statistics.median(episode_ms.tolist()))
                row[name + "_ended_per_step"] = float(env.episode.counts[0])  # (of the last step: the order of magnitude)
            env.close()
            del env
            torch.cuda.empty_cache()
        if not a.baseline_only and sorted(a.order) == list("abcd"):
            base = row["a_step_ms"]
            for name in ("b_next_step", "c_same_step", "d_same_step_limit"):
                row[name + "_over_a_pct"] = 100.0 * (row[name + "_ms"] - base) / base
            print("%-9s (a) %.4f ms  (b) %.4f (%+.2f %%)  (c) %.4f (%+.2f %%)  (d) %.4f (%+.2f %%)  | episode launches alone %.1f / %.1f / %.1f us"
                  % (game, base, row["b_next_step_ms"], row["b_next_step_over_a_pct"], row["c_same_step_ms"], row["c_same_step_over_a_pct"],
                     row["d_same_step_limit_ms"], row["d_same_step_limit_over_a_pct"], row["b_next_step_episode_us"],
                     row["c_same_step_episode_us"], row["d_same_step_limit_episode_us"]), flush=True)
        else:
            print("%-9s %s" % (game, "  ".join("(%s) %.4f ms [%.4f .. %.4f]" % (k[0], row[k + "_ms"], row[k + "_ms_min"], row[k + "_ms_max"])
                                                for k, _, _, _ in VARIANTS if k + "_ms" in row)), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
