#!/usr/bin/env python
"""What assigning levels costs a rollout (pgv_assign_levels, include/procgen2_vec.h): env-steps/s of

  (a) an engine in level-seed mode (--num-levels levels) that is never assigned anything, and
  (b) the same engine with EVERY finished env assigned its next level after every step, from a table on the device:
          assign_levels(table[torch.randint(...)], <the envs with done != 0>)
      with no host synchronisation in the loop,

per game (maze, coinrun) at --envs envs (65 536), in one process, seconds apart: boxes differ, a pair taken on one does
not.  Both loops enqueue --steps synthetic steps after --warmup and are timed by events on torch's current stream; the
level generator's launches (pgv_generator_launches) are counted over the timed steps.  An assignment call costs one small
launch over its indices and ONE forced launch of the generator on the side stream, where (a) launches it every
pregen_every()-th step only — the launch counts show which of the two a difference comes from; the levels themselves are
generated an episode ahead on the side stream either way (an assignment made at `done` is the late case: the env resets in
the very next step, so its level is generated inside that step or waited for).

--select where (default): the indices are torch.where(done != 0, arange, -1) — an index outside the batch is skipped, and
nothing on the host waits for a count.  --select nonzero: done.nonzero(), which torch cannot size without reading the
count back: one host synchronisation per step, shown for what it costs.  Between (a) and (b) a line gives the loop of (b)
with its torch ops (randint, the table gather, where) and WITHOUT the assignment call: what of the difference is torch's.

    python tools/assign_levels_rate.py [--games maze coinrun] [--select where nonzero] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", nargs="*", default=["maze", "coinrun"])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--num-levels", type=int, default=200)
    ap.add_argument("--select", nargs="*", default=["where"], choices=["where", "nonzero"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd.vec_env import ProcgenVecEnv

    def run(game, select):
        """select None: no assignments.  Returns (env-steps/s, generator launches over the timed steps)."""
        env = ProcgenVecEnv(game, a.envs, seed_base=1, num_levels=a.num_levels, start_level=0)
        n = a.envs
        gen = torch.Generator(device=env.device)
        gen.manual_seed(1)
        table = torch.arange(a.num_levels, device=env.device, dtype=torch.int32)
        everyone = torch.arange(n, device=env.device, dtype=torch.int32)
        nobody = torch.full((n,), -1, device=env.device, dtype=torch.int32)
        env.reset()

        def one():
            _, _, done = env.step_synthetic(3)
            if select in ("where", "ops"):
                levels = table[torch.randint(0, a.num_levels, (n,), device=env.device, generator=gen)]
                indices = torch.where(done != 0, everyone, nobody)
                if select == "where":
                    env.assign_levels(levels, indices)
            elif select == "nonzero":
                idx = done.nonzero().reshape(-1)
                env.assign_levels(table[torch.randint(0, a.num_levels, (idx.numel(),), device=env.device, generator=gen)], idx)

        for _ in range(a.warmup):
            one()
        torch.cuda.synchronize()
        launches = env.L.pgv_generator_launches(env._h)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            one()
        e1.record()
        e1.synchronize()
        torch.cuda.synchronize()
        rate = n * a.steps / (e0.elapsed_time(e1) * 1e-3)
        launches = env.L.pgv_generator_launches(env._h) - launches
        env.close()
        return rate, launches

    rows = []
    for game in a.games:
        base_rate, base_launches = run(game, None)
        row = {"game": game, "envs": a.envs, "steps": a.steps, "num_levels": a.num_levels, "plain_env_steps_per_s": base_rate,
               "plain_generator_launches": base_launches}
        print("%-8s (a) no assignments        %7.1f M env-steps/s   %4d generator launches in %d steps"
              % (game, base_rate / 1e6, base_launches, a.steps), flush=True)
        ops_rate, _ = run(game, "ops")  # the torch ops that choose levels and indices, and no assignment call
        row["ops_only_env_steps_per_s"] = ops_rate
        print("%-8s     torch ops of (b) alone  %7.1f M env-steps/s   (randint, gather, where; nothing assigned)"
              % (game, ops_rate / 1e6), flush=True)
        for select in a.select:
            rate, launches = run(game, select)
            row[select + "_env_steps_per_s"], row[select + "_generator_launches"] = rate, launches
            print("%-8s (b) assigned, %-8s    %7.1f M env-steps/s   %4d generator launches   (b)/(a) %.3f"
                  % (game, select, rate / 1e6, launches, rate / base_rate), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
