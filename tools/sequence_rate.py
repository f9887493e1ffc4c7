#!/usr/bin/env python
"""What a step without a frame costs (include/procgen2_vec.h pgv_step_sequence).

Per game, at --envs envs (65 536), in ONE engine and one process, after --warmup synthetic steps (>= 64: levels prefetched,
episodes spread out), milliseconds a sub-step and env-steps/s of
    step_a / step_b     pgv_step_synthetic, twice in every repeat: their difference is the spread (a) is held to
    T{1,4,16,64}_last   pgv_step_sequence, synthetic actions, PGV_FRAMES_LAST
    T{1,4,16,64}_none   … PGV_FRAMES_NONE
each measured the same way: two HIP events on the env's stream round --steps sub-steps (steps / T back-to-back calls) with
nothing else in the region, --repeats times, the median.  The sequences write every output (rewards, dones, the summary);
`bare` repeats T = 1 last and T = 64 none with every output pointer NULL: the launches of the steps alone.
The variants are INTERLEAVED: every repeat measures one region of each variant of a group in turn, so what an engine's
rollout does to its step time over a run (episodes go out of phase) is shared by all of them.  Group 1 holds what draws every
step — step_a, T1_last_bare, T1_last, step_b — and nothing else, so that frameless sub-steps, which empty the level
prefetch, do not come between the two sides of comparison (a); group 2 holds the rest.
Then one run of pgv_step_phases over --steps steps (events inside the step: a run of its own): the logic and late phases'
medians, which a frameless sub-step is held to (b): ratio = T64_none_bare / (logic + late).

    python tools/sequence_rate.py [--games coinrun chaser] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTHS = (1, 4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", nargs="*", default=None)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=96)
    ap.add_argument("--steps", type=int, default=64, help="sub-steps a region (a multiple of 64)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.warmup < 64 or a.steps % 64:
        ap.error("--warmup must be at least 64, --steps a multiple of 64")
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import GAMES, ProcgenVecEnv, SequenceResult

    rows = []
    for game in a.games or GAMES:
        env = ProcgenVecEnv(game, a.envs, seed_base=1)
        L, h, st = env.L, env._h, env._stream
        env.reset()
        for _ in range(a.warmup):
            pglib.check(L, L.pgv_step_synthetic(h, a.run_seed), "pgv_step_synthetic")
        env.sync()

        def interleaved(group):
            """group: (name, call, calls a region).  One region of each in turn, --repeats times; the medians into `row`."""
            ms = {name: [] for name, _, _ in group}
            for _ in range(a.repeats):
                for name, call, calls in group:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    for _ in range(calls):
                        call()
                    e1.record(st)
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / a.steps)
            for name in ms:
                row[name + "_ms"] = statistics.median(ms[name])
                row[name + "_regions"] = [min(ms[name]), max(ms[name])]  # the scatter of the variant's own regions

        def plain():
            pglib.check(L, L.pgv_step_synthetic(h, a.run_seed), "pgv_step_synthetic")

        def sequence(T, frames, outputs):
            ptr = {}
            if outputs:
                out = {k: torch.zeros(shape, dtype=dtype, device=env.device) for k, (shape, dtype) in SequenceResult.layout(T, a.envs).items()}
                ptr = {k: ctypes.c_void_p(v.data_ptr()) for k, v in out.items()}
                keep.append(out)
            q = pglib.sequence(T, None, 0, a.run_seed, frames, **ptr)
            return lambda: pglib.check(L, L.pgv_step_sequence(h, ctypes.byref(q)), "pgv_step_sequence")

        keep = []
        row = {"game": game, "envs": a.envs, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup}
        interleaved([("step_a", plain, a.steps), ("T1_last_bare", sequence(1, "last", False), a.steps),
                     ("T1_last", sequence(1, "last", True), a.steps), ("step_b", plain, a.steps)])
        interleaved([("T%d_%s" % (T, frames), sequence(T, frames, True), a.steps // T)
                     for T in LENGTHS for frames in ("last", "none") if (T, frames) != (1, "last")]
                    + [("T64_none_bare", sequence(64, "none", False), a.steps // 64)])
        phases = env.step_phases(a.steps, a.run_seed)
        for k in ("step", "logic", "prepass", "render", "late"):
            row["phase_%s_ms" % k] = float(statistics.median(phases[k].tolist()))
        env.close()
        del env, keep
        torch.cuda.empty_cache()

        step = min(row["step_a_ms"], row["step_b_ms"])
        row["step_spread_pct"] = 100.0 * abs(row["step_a_ms"] - row["step_b_ms"]) / step
        row["step_regions_pct"] = 100.0 * (max(row["step_a_regions"][1], row["step_b_regions"][1]) - min(row["step_a_regions"][0], row["step_b_regions"][0])) / step
        row["T1_last_over_step_pct"] = 100.0 * (row["T1_last_ms"] - step) / step
        row["T1_last_bare_over_step_pct"] = 100.0 * (row["T1_last_bare_ms"] - step) / step
        row["logic_late_ms"] = row["phase_logic_ms"] + row["phase_late_ms"]
        row["frameless_over_logic_late"] = row["T64_none_bare_ms"] / row["logic_late_ms"]
        for k in [k for k in row if k.endswith("_ms")]:
            row[k[:-3] + "_Msteps"] = 1e-3 * a.envs / row[k]
        print("%-9s step %.4f / %.4f ms (spread %.2f %%, regions within %.2f %%) | T=1 last %+.2f %% (bare %+.2f %%) | last " % (
            game, row["step_a_ms"], row["step_b_ms"], row["step_spread_pct"], row["step_regions_pct"], row["T1_last_over_step_pct"], row["T1_last_bare_over_step_pct"])
            + " ".join("%.0f" % row["T%d_last_Msteps" % T] for T in LENGTHS) + " | none "
            + " ".join("%.0f" % row["T%d_none_Msteps" % T] for T in LENGTHS)
            + " M env-steps/s | frameless %.1f us (bare %.1f), logic + late %.1f us, ratio %.2f" % (
                1e3 * row["T64_none_ms"], 1e3 * row["T64_none_bare_ms"], 1e3 * row["logic_late_ms"], row["frameless_over_logic_late"]), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
