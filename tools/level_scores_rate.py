#!/usr/bin/env python
"""What the level replay scores cost (include/procgen2_vec.h pgv_level_scores_enable): an update beside V-trace over the same
rows, on both of its atomic paths, and the level-word launch on a recorded step.

In one process, at --shape (envs x L), engines of --game with a gray ring of L + 1 slots, stepped L + 8 times; each region two
HIP events on the env's stream round its calls, --repeats times, the median with its minimum and maximum, the regions of a group
INTERLEAVED (every repeat measures one region of each in turn).
    step, step+levels    pgv_step_synthetic with history + transitions, without and with level scores (two engines side by side).
    vtrace               transition_vtrace with ratios and advantages on the engine without: the yardstick — it reads a similar
                         number of ring bytes.
    update K lds|global  level_scores_update over the L rows, kind abs, partial segments included, per capacity K of
                         --capacities on an engine with num_levels = K: through the workgroups' own tables (K <= 1024 only),
                         and with pgv_set_debug bit 28, straight into device memory.
Bytes a cell: an update reads flags 1, began 1, reward 4, level 4, known 1 and the signal 4: 15.

--episode-steps M > 0: same-step episodes with a time limit of M steps (pgv_step_episodes_synthetic) in place of plain steps,
so that a stretch holds L / M segments an env: the closes at their densest.

    python tools/level_scores_rate.py [--json out.json] [--shape 16384x256] [--capacities 200,1024,100000] [--episode-steps 8]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="coinrun")
    ap.add_argument("--shape", default="16384x256", help="envs x L")
    ap.add_argument("--capacities", default="200,1024,100000")
    ap.add_argument("--episode-steps", type=int, default=0, help="0: plain steps; M: same-step episodes truncated at M steps")
    ap.add_argument("--calls", type=int, default=32, help="calls a region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    def regions(group):
        """group: (name, stream, before, call).  One region of each in turn, --repeats times → {name: (median, min, max)} ms a call."""
        ms = {name: [] for name, _, _, _ in group}
        for _ in range(a.repeats):
            for name, st, before, call in group:
                before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.calls):
                    call()
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.calls)
        return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}

    def show(name, r, more=""):
        print("%-22s %.4f ms [%.4f .. %.4f] (spread %.1f %%)%s" % (name, *r, 100.0 * (r[2] - r[1]) / r[0], more), flush=True)

    n, L = (int(x) for x in a.shape.split("x"))
    capacities = [int(x) for x in a.capacities.split(",")]

    def engine(levels):
        more = dict(num_levels=levels, level_scores=dict(first_level=0, capacity=levels)) if levels else {}
        if a.episode_steps:
            more.update(autoreset_mode="same_step", max_episode_steps=a.episode_steps)
        v = ProcgenVecEnv(a.game, n, seed_base=1, history=dict(capacity=L + 1, gray=True), transitions=True, **more)
        v.reset()
        for _ in range(L + 8):
            stepper(v)()
        v.sync()
        return v

    def nothing():
        pass

    def stepper(v):
        if a.episode_steps:
            return lambda: pglib.check(v.L, v.L.pgv_step_episodes_synthetic(v._h, a.run_seed), "pgv_step_episodes_synthetic")
        return lambda: pglib.check(v.L, v.L.pgv_step_synthetic(v._h, a.run_seed), "pgv_step_synthetic")

    result = {"game": a.game, "episode_steps": a.episode_steps, "envs": n, "L": L, "calls": a.calls, "repeats": a.repeats, "lds_levels": pglib.LEVEL_SCORE_LDS_LEVELS, "ms": {}}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(6)
    V = torch.randn((L + 1, n), generator=gen, device="cuda")
    rho = torch.exp(0.5 * torch.randn((L, n), generator=gen, device="cuda"))
    signal = torch.randn((L, n), generator=gen, device="cuda")
    plain = engine(0)
    for k, K in enumerate(capacities):
        v = engine(K)
        if k == 0:  # the step, on both engines; their rings have moved on afterwards, so the stretch is taken behind it
            r = regions([("step", plain._stream, nothing, stepper(plain)), ("step+levels", v._stream, nothing, stepper(v))])
            result["ms"].update(r)
            show("step", r["step"]), show("step+levels", r["step+levels"], " | + %.4f ms" % (r["step+levels"][0] - r["step"][0]))
        first = v.history.head - 1 - L

        def on(env, f):
            def call():
                with torch.cuda.stream(env._stream):
                    f()
            return call

        def path(flag):
            return lambda: pglib.check(v.L, v.L.pgv_set_debug(v._h, flag), "pgv_set_debug")

        update = on(v, lambda: v.level_scores_update(first, L, signal, "abs", 0.5, True, 1))
        group = [("update %d global" % K, v._stream, path(pglib.DEBUG_LEVEL_SCORES_GLOBAL), update)]
        if K <= pglib.LEVEL_SCORE_LDS_LEVELS:
            group.insert(0, ("update %d lds" % K, v._stream, path(0), update))
        if k == 0:
            plain_first = plain.history.head - 1 - L
            group.append(("vtrace", plain._stream, nothing, on(plain, lambda: plain.transition_vtrace(plain_first, L, V, rho, 0.999, 0.95))))
        tables = []
        for _, _, before, call in group:  # every region warm, and the paths held to each other
            v.level_scores.score.zero_(), v.level_scores.episodes.zero_()
            before(), call(), call()
            torch.cuda.synchronize()
            tables.append((v.level_scores.score.clone(), v.level_scores.episodes.clone(), v.level_scores.max_return.clone()))
        assert all(torch.equal(x, y) for t in tables[1:2] for x, y in zip(tables[0], t)), "the two paths disagree"
        r = regions(group)
        result["ms"].update(r)
        segments, steps = (int(x) for x in v.level_scores_update(first, L, signal, "abs", 0.5, True, 1, totals=True))
        result["segments %d" % K], result["steps %d" % K] = segments, steps
        yard = result["ms"]["vtrace"][0]
        for name, _, _, _ in group:
            show(name, r[name], "" if name == "vtrace" else " | %.0f GB/s | / vtrace %.2f | %d segments" % (1e-6 * 15 * L * n / r[name][0], r[name][0] / yard, segments))
        path(0)()
        v.close()
        del v
        torch.cuda.empty_cache()
    plain.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
