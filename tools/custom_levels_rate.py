#!/usr/bin/env python
"""Cost of caller-made levels (pgv_get_levels / pgv_set_levels, include/procgen2_vec.h) beside pgv_reset of the same envs
and beside the game's own step.

Maze, at --envs envs (65 536), per mode: the HIP-event time, on the env's stream, of
  * pgv_set_levels of EVERY env (the levels read from the engine itself with pgv_get_levels, their goals moved off the
    agent's cell where the generator had put them there, so that every row is installed);
  * pgv_set_levels of the envs that ended in a step — the fixed-size call, indices = where(done, arange, -1) — and how many
    those were;
  * pgv_reset of all envs and pgv_reset under the same `done` mask, in the same process on the same device: a reset builds
    or copies a level where an install takes the caller's, and launches the generator behind it;
  * pgv_get_levels of every env;
  * the game's own step from pgv_timed_steps (no per-launch events),
`--repeats` times after `--warmups`, the median.  Only ratios taken inside one run mean anything.

    python tools/custom_levels_rate.py [--modes easy hard memory] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="*", default=["easy", "hard", "memory"])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64, help="synthetic steps before the measurement, and steps of the timed run")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv

    def timed(stream, fn, before=None):
        """Median milliseconds of fn() between two events on `stream`; before() runs outside the region."""
        ms = []
        for k in range(a.warmups + a.repeats):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if k >= a.warmups:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    out = []
    for mode in a.modes:
        env = ProcgenVecEnv("maze", a.envs, seed_base=1, distribution_mode=mode)
        n, st = a.envs, env._stream
        env.reset()
        with torch.cuda.stream(st):  # (the calls' own stream: the regions hold the calls and nothing else)
            levels = env.get_levels()
            # the generator may put the goal on the agent's cell; an install refuses that: move such a goal to another open cell
            same = levels.goal_cell == levels.agent_cell
            other = (levels.tiles == 0) & (torch.arange(levels.tiles.shape[1], device=env.device)[None, :] != levels.agent_cell[:, None].long())
            levels = levels._replace(goal_cell=torch.where(same, other.int().argmax(dim=1).int(), levels.goal_cell))
            ids = torch.arange(n, dtype=torch.int32, device=env.device)
            arange = torch.arange(n, dtype=torch.int32, device=env.device)
            status = env.set_levels(levels, ids=ids)
            installed = int((status == 0).sum())
            for _ in range(a.steps):
                env.step_synthetic(3)
            done = env.done.clone()
            ended = torch.where(done != 0, arange, torch.full_like(arange, -1))
            torch.cuda.synchronize()
            r = {"mode": env.distribution_mode, "envs": n, "cells": env.level_layout.cells, "installed_of_all": installed,
                 "ended": int((done != 0).sum()),
                 "get_all_ms": timed(st, lambda: env.get_levels()),
                 "set_all_ms": timed(st, lambda: env.set_levels(levels, ids=ids)),
                 "reset_all_ms": timed(st, lambda: env.reset()),
                 "set_ended_ms": timed(st, lambda: env.set_levels(levels, ids=ids, indices=ended)),
                 "reset_ended_ms": timed(st, lambda: env.reset(mask=done))}
        total, _ = env.timed_steps(a.steps, run_seed=3, render_events=False)
        r["step_ms"] = total / a.steps
        r["set_all_of_reset"] = r["set_all_ms"] / r["reset_all_ms"]
        r["set_ended_of_reset"] = r["set_ended_ms"] / r["reset_ended_ms"]
        r["set_ended_of_step"] = r["set_ended_ms"] / r["step_ms"]
        print("maze %-6s %4d cells  step %6.3f ms | all %d envs: set %6.3f ms = %4.2f x reset (%6.3f), get %6.3f ms | the %d envs that ended: "
              "set %6.3f ms = %4.2f x reset (%6.3f), %4.2f of a step"
              % (r["mode"], r["cells"], r["step_ms"], n, r["set_all_ms"], r["set_all_of_reset"], r["reset_all_ms"], r["get_all_ms"], r["ended"],
                 r["set_ended_ms"], r["set_ended_of_reset"], r["reset_ended_ms"], r["set_ended_of_step"]), flush=True)
        out.append(r)
        env.close()
        del levels
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
