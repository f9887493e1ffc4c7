#!/usr/bin/env python
"""What the frame history on the device costs (include/procgen2_vec.h pgv_history_enable).

Per game, at --envs envs (65 536), in one process, engines made alike and stepped alike — the same seeds, the same synthetic
actions, the same number of steps — after --warmup steps, each measured the same way: two HIP events on the env's stream
round --steps calls, --repeats times, the median, the variants INTERLEAVED (every repeat measures one region of each in turn).
    steps    milliseconds a step of pgv_step_synthetic with the feature off (a), with the history RGB and gray (b: the step
             ends with a push of one frame per env into a ring of --capacity slots), and with the policy observations
             K = 4, RGB, f16 (c: the step ends with a push that moves the whole stack);
    push     pgv_history_push alone, RGB, beside pgv_policy_obs_push of K = 1, RGB, u8 — the same bytes: 12 288 read and
             12 288 written per env — and a device-to-device copy that moves as many;
    gather   pgv_history_gather of every env at head - 1, K = 4, f16, and of a --minibatch (16 384) of random (push, env)
             pairs over the held pushes of the ring, each beside a device-to-device copy that moves as many bytes as the
             gather (per entry K*C*4096 read and K*C*4096 elements written; half of the copy's bytes are read, half
             written).  --gather-dtype names another element type.
--other-lib PATH: the gather regions once more on an engine of that library (one built with another store form), interleaved
with the tree's own.
--parent-lib PATH: the off path against the parent commit's library is tools/policy_obs_rate.py --off-path-only's job.

    python tools/history_rate.py [--games coinrun maze] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", nargs="*", default=["coinrun", "maze"])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=96)
    ap.add_argument("--steps", type=int, default=32, help="calls a region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--gather-dtype", default="float16", choices=["uint8", "float16", "bfloat16", "float32"])
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    def regions(group):
        """group: (name, stream, call).  One region of each in turn, --repeats times → {name: (median, min, max)} ms a call."""
        ms = {name: [] for name, _, _ in group}
        for _ in range(a.repeats):
            for name, st, call in group:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.steps):
                    call()
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.steps)
        return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}

    def stepper(env):
        return lambda: pglib.check(env.L, env.L.pgv_step_synthetic(env._h, a.run_seed), "pgv_step_synthetic")

    def warm(env):
        env.reset()
        for _ in range(a.warmup):
            stepper(env)()
        env.sync()

    def copier(stream, moved):
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        return copy

    def spread(r):
        return 100.0 * (r[2] - r[1]) / r[0]

    K, T, n = 4, a.capacity, a.envs
    dtype_number, es = pglib.POLICY_DTYPES[a.gather_dtype]
    row_bytes = K * 3 * 4096 * (1 + es)  # a gathered row: K*C*4096 bytes read, K*C*4096 elements written
    rows = []
    for game in a.games:
        # -- steps ---------------------------------------------------------------------------------
        engines = {"off": ProcgenVecEnv(game, n, seed_base=1),
                   "history_rgb": ProcgenVecEnv(game, n, seed_base=1, history=dict(capacity=T, gray=False)),
                   "history_gray": ProcgenVecEnv(game, n, seed_base=1, history=dict(capacity=T, gray=True)),
                   "policy_k4_rgb_f16": ProcgenVecEnv(game, n, seed_base=1, policy_obs=dict(stack=K, gray=False, dtype="float16"))}
        torch.cuda.synchronize()
        for e in engines.values():
            warm(e)
        r = regions([(name, e._stream, stepper(e)) for name, e in engines.items()])
        assert all(bool((e.obs == engines["off"].obs).all()) for e in engines.values()), "the engines left the same rollout"
        row = {"game": game, "envs": n, "capacity": T, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup, "step_ms": r,
               "adds_ms": {k: r[k][0] - r["off"][0] for k in r if k != "off"}}
        print("%-8s step: off %.4f ms (spread %.1f %%) | history RGB %.4f (+%.4f) | history gray %.4f (+%.4f) | policy K=4 RGB f16 %.4f (+%.4f)" % (
            game, r["off"][0], spread(r["off"]), r["history_rgb"][0], row["adds_ms"]["history_rgb"], r["history_gray"][0],
            row["adds_ms"]["history_gray"], r["policy_k4_rgb_f16"][0], row["adds_ms"]["policy_k4_rgb_f16"]), flush=True)
        engines["policy_k4_rgb_f16"].close(), engines["history_gray"].close(), engines["off"].close()
        hist = engines["history_rgb"]
        del engines
        torch.cuda.empty_cache()
        # -- the push alone, beside the policy push that moves the same bytes ----------------------------
        pol = ProcgenVecEnv(game, n, seed_base=1, policy_obs=dict(stack=1, gray=False, dtype="uint8"))
        warm(pol)
        moved = n * 2 * 12288
        p = regions([("history_push", hist._stream, lambda: pglib.check(hist.L, hist.L.pgv_history_push(hist._h), "pgv_history_push")),
                     ("policy_push_k1_rgb_u8", pol._stream, lambda: pglib.check(pol.L, pol.L.pgv_policy_obs_push(pol._h, None), "pgv_policy_obs_push")),
                     ("copy", hist._stream, copier(hist._stream, moved))])
        row.update({"push_ms": p, "push_bytes": moved, "push_GBps": {k: 1e-6 * moved / v[0] for k, v in p.items()},
                    "push_spread_pct": {k: spread(v) for k, v in p.items()}})
        print("%-8s push: history %.4f ms %.0f GB/s (spread %.1f %%) | policy K=1 RGB u8 %.4f ms %.0f GB/s (spread %.1f %%) | copy %.4f ms %.0f GB/s" % (
            game, p["history_push"][0], row["push_GBps"]["history_push"], spread(p["history_push"]), p["policy_push_k1_rgb_u8"][0],
            row["push_GBps"]["policy_push_k1_rgb_u8"], spread(p["policy_push_k1_rgb_u8"]), p["copy"][0], row["push_GBps"]["copy"]), flush=True)
        pol.close()
        del pol
        torch.cuda.empty_cache()
        # -- gather ----------------------------------------------------------------------------------
        gen = torch.Generator(device="cuda")
        gen.manual_seed(5)
        group, keep = [], []
        libs = [("", hist)]
        if a.other_lib:
            other = ProcgenVecEnv(game, n, seed_base=1, lib_path=a.other_lib, history=dict(capacity=T, gray=False))
            warm(other)
            libs.append(("other_", other))
        for tag, e in libs:
            head = e.history.head
            for name, count in (("all_envs", n), ("minibatch", a.minibatch)):
                if name == "all_envs":
                    pushes = torch.full((n,), head - 1, dtype=torch.int64, device="cuda")
                    envs = torch.arange(n, dtype=torch.int32, device="cuda")
                else:
                    pushes = torch.randint(max(0, head - T), head, (count,), generator=gen, device="cuda", dtype=torch.int64)
                    envs = torch.randint(0, n, (count,), generator=gen, device="cuda", dtype=torch.int32)
                out = torch.empty((count, K * 3, 64, 64), dtype=getattr(torch, a.gather_dtype), device="cuda")
                keep.append((pushes, envs, out))

                def gather(e=e, pushes=pushes, envs=envs, out=out, count=count):
                    pglib.check(e.L, e.L.pgv_history_gather(e._h, pushes.data_ptr(), envs.data_ptr(), count, K, dtype_number, out.data_ptr()), "pgv_history_gather")
                group.append((tag + "gather_" + name, e._stream, gather))
                if not tag:
                    group.append(("copy_" + name, e._stream, copier(e._stream, count * row_bytes)))
        torch.cuda.synchronize()
        g = regions(group)
        row.update({"gather_ms": g, "minibatch": a.minibatch, "stack": K, "dtype": a.gather_dtype,
                    "gather_bytes": {"all_envs": n * row_bytes, "minibatch": a.minibatch * row_bytes}})
        for name, count in (("all_envs", n), ("minibatch", a.minibatch)):
            moved = count * row_bytes
            line = "%-8s gather %-9s %6d rows: %.4f ms %.0f GB/s (spread %.1f %%) | copy %.4f ms %.0f GB/s, fraction %.2f" % (
                game, name, count, g["gather_" + name][0], 1e-6 * moved / g["gather_" + name][0], spread(g["gather_" + name]),
                g["copy_" + name][0], 1e-6 * moved / g["copy_" + name][0], g["copy_" + name][0] / g["gather_" + name][0])
            if a.other_lib:
                line += " | other lib %.4f ms (spread %.1f %%)" % (g["other_gather_" + name][0], spread(g["other_gather_" + name]))
            print(line, flush=True)
        rows.append(row)
        for _, e in libs:
            e.close()
        del libs, hist, keep, group
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
