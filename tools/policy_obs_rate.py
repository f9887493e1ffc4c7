#!/usr/bin/env python
"""What policy-ready observations on the device cost (include/procgen2_vec.h pgv_policy_obs_enable).

Per game and configuration (K, gray | RGB, dtype), at --envs envs (65 536), in one process, three engines made alike and
stepped alike — the same seeds, the same synthetic actions, the same number of steps, so all three walk through the same
rollout — after --warmup steps, milliseconds a step of
    a   pgv_step_synthetic, the feature off;
    b   pgv_step_synthetic, the feature on (the step ends with the push);
    c   pgv_step_synthetic, the feature off, plus the torch expression that makes the same tensor on the same stream, written
        the way a user writes it: keep the done row, permute(0, 3, 1, 2).contiguous(), .to(dtype) / 255 (gray: the integer
        rule first), torch.cat over the stack, torch.where on the envs whose episode just began;
each measured the same way: two HIP events on the env's stream round --steps steps, --repeats times, the median, the variants
INTERLEAVED (every repeat measures one region of each in turn).  The feature exists to make b - a smaller than c - a.
Before anything is timed, c's tensor is compared with b's: `same` says whether they are equal bit for bit (a user's
.to(float16) / 255 divides in half precision — one rounding where the engine's table has two — so some values may differ
by one unit in the last place; the count is reported, nothing is tuned).
Then, on engine b alone: `push`, --steps calls of pgv_policy_obs_push(NULL) in a region (no flag is pending: every env
moves its stack) — the bytes it moves (12 288 read, the K - 1 slots it moves read, K slots written, per env) over its time —
`push_strided`, the same with each lane storing its own values as they lie (pgv_set_debug bit 26), and `copy`, a
device-to-device copy that moves as many bytes (half of them read, half written), timed in the same run; copy_fraction =
the push's bytes/s over the copy's.
--parent-lib PATH: two engines of the parent commit's library and one of the tree's own between them, all with the feature
off and stepped alike, regions parent_a, now, parent_b interleaved — the off path's one host branch against the spread between
two runs of the parent — then the other way round (now_a, parent, now_b), and then three engines of the parent's library
(parent_a, parent_m, parent_b): an excess that the engine in the middle shows whichever library it is of comes from its place,
not from the code.  --arrangements pnp,npn,ppp names them and their order: the second coinrun engine made in a fresh process
steps 11 % slower whichever library it is of (docs/OPTLOG.md), so read no arrangement that came first without one that did not.

    python tools/policy_obs_rate.py [--games coinrun maze] [--parent-lib procgen2_amd/lib_ref/libprocgen2_hip_parent.so] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ((4, True, "float16"), (4, False, "float16"), (1, False, "uint8"), (4, False, "float32"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", nargs="*", default=["coinrun", "maze"])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=96)
    ap.add_argument("--steps", type=int, default=32, help="steps a region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--arrangements", default="pnp,npn,ppp", help="with --parent-lib: which arrangements, in which order (the first "
                    "one of a process is made on a fresh heap)")
    ap.add_argument("--off-path-only", action="store_true", help="with --parent-lib: that comparison and nothing else")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    def regions(group):
        """group: (name, stream, call).  One region of each in turn, --repeats times → {name: (median, min, max)} ms a step."""
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

    class RawEngine:
        """An engine of any library that has the calls a step needs (the parent commit's lacks the new ones, which
        pglib.load would insist on): made, reset and stepped through ctypes on a torch stream of its own."""

        def __init__(self, path, game, n):
            import ctypes
            self.L = L = ctypes.CDLL(os.path.abspath(path))
            P = ctypes.c_void_p
            L.pgv_last_error.restype = ctypes.c_char_p
            L.pgv_make_config.argtypes = [ctypes.POINTER(pglib.Config), ctypes.POINTER(P)]
            L.pgv_reset.argtypes, L.pgv_step_synthetic.argtypes, L.pgv_sync.argtypes, L.pgv_close.argtypes = [P, P, P], [P, ctypes.c_uint32], [P], [P]
            self._stream = torch.cuda.Stream()
            self._h = pglib.make(L, game, n, seed_base=1, stream=P(self._stream.cuda_stream))

        def reset(self):
            pglib.check(self.L, self.L.pgv_reset(self._h, None, None), "pgv_reset")

        def sync(self):
            pglib.check(self.L, self.L.pgv_sync(self._h), "pgv_sync")

        def close(self):
            self.L.pgv_close(self._h)

    rows = []
    for game in a.games:
        if a.parent_lib:
            # Three engines stepped alike, three times: two of the parent's library — their difference is what two runs of the
            # same code differ by — with one of the tree's own between them, then the other way round, then all three of the
            # parent's (what the place in the middle does to a figure shows as the same excess in every arrangement).
            orders = {"pnp": ("parent_a", "now", "parent_b"), "npn": ("now_a", "parent", "now_b"), "ppp": ("parent_a", "parent_m", "parent_b")}
            for names in [orders[k] for k in a.arrangements.split(",")]:
                engines = [RawEngine(a.parent_lib if name.startswith("parent") else pglib.DEFAULT_LIB, game, a.envs) for name in names]
                for e in engines:
                    warm(e)
                r = regions([(name, e._stream, stepper(e)) for name, e in zip(names, engines)])
                outer = 0.5 * (r[names[0]][0] + r[names[2]][0])
                row = {"game": game, "envs": a.envs, "off_path": {k: v for k, v in r.items()}, "order": names,
                       "outer_spread_pct": 100.0 * abs(r[names[0]][0] - r[names[2]][0]) / min(r[names[0]][0], r[names[2]][0]),
                       "middle_over_outer_pct": 100.0 * (r[names[1]][0] - outer) / outer}
                print("%-8s off path: %s %.4f / %s %.4f ms (spread %.2f %%), %s between them %.4f ms (%+.2f %% against their mean)" % (
                    game, names[0], r[names[0]][0], names[2], r[names[2]][0], row["outer_spread_pct"], names[1], r[names[1]][0],
                    row["middle_over_outer_pct"]), flush=True)
                rows.append(row)
                for e in engines:
                    e.close()
                del engines
                torch.cuda.empty_cache()
        if a.off_path_only:
            continue
        for K, gray, dtype in CONFIGS:
            C, es = 1 if gray else 3, pglib.POLICY_DTYPES[dtype][1]
            tdtype = getattr(torch, dtype)
            off = ProcgenVecEnv(game, a.envs, seed_base=1)
            on = ProcgenVecEnv(game, a.envs, seed_base=1, policy_obs=dict(stack=K, gray=gray, dtype=dtype))
            user = ProcgenVecEnv(game, a.envs, seed_base=1)
            state = {"stack": torch.zeros((a.envs, K * C, 64, 64), dtype=tdtype, device=user.device), "first": True}

            def convert(obs):
                if gray:
                    o = obs.to(torch.int32)
                    x = ((77 * o[..., 0] + 150 * o[..., 1] + 29 * o[..., 2] + 128) >> 8).unsqueeze(1)
                else:
                    x = obs.permute(0, 3, 1, 2).contiguous()
                return x.to(tdtype) if dtype == "uint8" else x.to(tdtype) / 255

            def user_step():
                """What the caller writes today, on the env's own stream."""
                with torch.cuda.stream(user._stream):
                    began = (user.done != 0) if not state["first"] else torch.ones_like(user.done, dtype=torch.bool)
                    state["first"] = False
                    stepper(user)()
                    new = convert(user.obs)
                    stack = torch.cat([state["stack"][:, C:], new], 1) if K > 1 else new
                    state["stack"] = torch.where(began[:, None, None, None], new.repeat(1, K, 1, 1), stack)

            torch.cuda.synchronize()
            warm(off), warm(on)
            user.reset()
            for _ in range(a.warmup):
                user_step()
            user.sync()
            torch.cuda.synchronize()
            differ = None
            same = bool(torch.equal(state["stack"], on.policy_obs))
            if not same:
                differ = int((state["stack"] != on.policy_obs).sum())
            r = regions([("a", off._stream, stepper(off)), ("b", on._stream, stepper(on)), ("c", user._stream, user_step)])
            assert bool((off.obs == on.obs).all()) and bool((off.obs == user.obs).all()), "the three engines left the same rollout"

            def push():
                pglib.check(on.L, on.L.pgv_policy_obs_push(on._h, None), "pgv_policy_obs_push")

            per_env = 12288 + (K - 1) * C * 4096 * es + K * C * 4096 * es
            moved = a.envs * per_env
            src = torch.empty(moved // 2, dtype=torch.uint8, device=on.device)
            dst = torch.empty_like(src)

            def copy():
                with torch.cuda.stream(on._stream):
                    dst.copy_(src)

            p = regions([("push", on._stream, push), ("copy", on._stream, copy)])
            pglib.check(on.L, on.L.pgv_set_debug(on._h, 1 << 26), "pgv_set_debug")
            p.update(regions([("push_strided", on._stream, push)]))
            row = {"game": game, "envs": a.envs, "stack": K, "gray": gray, "dtype": dtype, "steps": a.steps, "repeats": a.repeats,
                   "warmup": a.warmup, "a_ms": r["a"], "b_ms": r["b"], "c_ms": r["c"], "engine_adds_ms": r["b"][0] - r["a"][0],
                   "torch_adds_ms": r["c"][0] - r["a"][0], "same": same, "values_that_differ": differ, "push_ms": p["push"],
                   "push_strided_ms": p["push_strided"], "copy_ms": p["copy"], "push_bytes": moved,
                   "push_GBps": 1e-6 * moved / p["push"][0], "push_strided_GBps": 1e-6 * moved / p["push_strided"][0],
                   "copy_GBps": 1e-6 * moved / p["copy"][0], "copy_fraction": p["copy"][0] / p["push"][0]}
            print("%-8s K=%d %-4s %-8s a %.4f  b %.4f  c %.4f ms | b-a %.4f  c-a %.4f ms (x%.1f) | same %s%s | push %.4f ms %.0f GB/s"
                  " (strided %.4f ms), copy %.4f ms %.0f GB/s, fraction %.2f" % (
                      game, K, "gray" if gray else "RGB", dtype, r["a"][0], r["b"][0], r["c"][0], row["engine_adds_ms"], row["torch_adds_ms"],
                      row["torch_adds_ms"] / max(row["engine_adds_ms"], 1e-9), same, "" if same else " (%d values differ)" % differ,
                      p["push"][0], row["push_GBps"], p["push_strided"][0], p["copy"][0], row["copy_GBps"], row["copy_fraction"]), flush=True)
            rows.append(row)
            off.close(), on.close(), user.close()
            del off, on, user, state, src, dst
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
