#!/usr/bin/env python
"""What the transitions on the device cost (include/procgen2_vec.h pgv_transitions_enable), and what they replace.

In one process, engines made alike and stepped alike — the same seeds, the same synthetic actions — after --warmup steps, each
region measured the same way: two HIP events on the env's stream round --steps calls, --repeats times, the median with its
minimum and maximum, the variants INTERLEAVED (every repeat measures one region of each in turn).
    step     milliseconds a step of pgv_step_synthetic of --game at --envs envs (65 536) with the frame history alone (off)
             and with the record ring beside it (on: one more launch a step, 9 bytes written and 6 read per env); with
             --parent-lib PATH the same history-only step on the parent commit's library, interleaved with both.
    gather   transition_gather of --entries (4 096) random (push, env) pairs, n = 3, K = 4, f16, beside what a learner does
             without it: two history_gather calls (the second at push + n) plus the n-step fold in torch over its own [T, N]
             reward and done tensors — a loop of n steps of small launches; and the gather's scalars alone beside that fold alone.
    gae      transition_gae over L = --gae-steps (256) rows at --gae-envs envs beside the recurrence as L dependent torch
             steps over the same [L, N] tensors.  Both results are compared before they are timed.

    python tools/transitions_rate.py [--json out.json] [--parent-lib PATH]
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
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--entries", type=int, default=4096)
    ap.add_argument("--gae-envs", type=int, default=16384)
    ap.add_argument("--gae-steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=96)
    ap.add_argument("--steps", type=int, default=32, help="calls a region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    def regions(group, calls=None):
        """group: (name, stream, call).  One region of each in turn, --repeats times → {name: (median, min, max)} ms a call."""
        calls = calls or a.steps
        ms = {name: [] for name, _, _ in group}
        for _ in range(a.repeats):
            for name, st, call in group:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(calls):
                    call()
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / calls)
        return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}

    def stepper(env):
        return lambda: pglib.check(env.L, env.L.pgv_step_synthetic(env._h, a.run_seed), "pgv_step_synthetic")

    def warm(env, steps):
        env.reset()
        for _ in range(steps):
            stepper(env)()
        env.sync()

    def spread(r):
        return 100.0 * (r[2] - r[1]) / r[0]

    def on_stream(env, f):
        def call():
            with torch.cuda.stream(env._stream):
                f()
        return call

    class RawEngine:
        """A history-only engine of any library that has the calls a step needs (the parent commit's lacks the new ones, which
        pglib.load would insist on): made, reset and stepped through ctypes on a torch stream of its own, the ring the engine's."""

        def __init__(self, path, game, n, capacity):
            import ctypes
            self.L = L = ctypes.CDLL(os.path.abspath(path))
            P = ctypes.c_void_p
            L.pgv_last_error.restype = ctypes.c_char_p
            L.pgv_make_config.argtypes = [ctypes.POINTER(pglib.Config), ctypes.POINTER(P)]
            L.pgv_reset.argtypes, L.pgv_step_synthetic.argtypes, L.pgv_sync.argtypes, L.pgv_close.argtypes = [P, P, P], [P, ctypes.c_uint32], [P], [P]
            L.pgv_history_enable.argtypes = [P, ctypes.POINTER(pglib.HistoryConfig)]
            self._stream = torch.cuda.Stream()
            self._h = pglib.make(L, game, n, seed_base=1, stream=P(self._stream.cuda_stream))
            pglib.history_enable(L, self._h, capacity, True, None)

        def reset(self):
            pglib.check(self.L, self.L.pgv_reset(self._h, None, None), "pgv_reset")

        def sync(self):
            pglib.check(self.L, self.L.pgv_sync(self._h), "pgv_sync")

        def close(self):
            self.L.pgv_close(self._h)

    result = {"game": a.game, "envs": a.envs, "capacity": a.capacity, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup}
    T, n = a.capacity, a.envs
    # -- the step ----------------------------------------------------------------------------------------
    ring = dict(capacity=T, gray=True)
    engines = {"off": ProcgenVecEnv(a.game, n, seed_base=1, history=ring), "on": ProcgenVecEnv(a.game, n, seed_base=1, history=ring, transitions=True)}
    if a.parent_lib:
        engines["parent_off"] = RawEngine(a.parent_lib, a.game, n, T)
    for e in engines.values():
        warm(e, a.warmup)
    r = regions([(name, e._stream, stepper(e)) for name, e in engines.items()])
    assert bool((engines["on"].obs == engines["off"].obs).all()), "the engines left the same rollout"
    result["step_ms"] = r
    result["step_adds_ms"] = r["on"][0] - r["off"][0]
    print("%-8s step, history gray T=%d: off %.4f ms (spread %.1f %%) | ring on %.4f ms (spread %.1f %%), +%.4f ms%s" % (
        a.game, T, r["off"][0], spread(r["off"]), r["on"][0], spread(r["on"]), result["step_adds_ms"],
        " | parent, off %.4f ms (spread %.1f %%)" % (r["parent_off"][0], spread(r["parent_off"])) if a.parent_lib else ""), flush=True)
    v = engines["on"]
    for name, e in engines.items():
        if e is not v:
            e.close()
    del engines
    torch.cuda.empty_cache()
    # -- the n-step gather -------------------------------------------------------------------------------
    steps_n, K, gamma, B = 3, 4, 0.99, a.entries
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    head = v.history.head
    pushes = torch.randint(head - T, head - 1, (B,), generator=gen, device="cuda", dtype=torch.int64)
    envs = torch.randint(0, n, (B,), generator=gen, device="cuda", dtype=torch.int32)
    # the learner's own copies of the rollout's other half, as it would keep them without the feature
    flags = v.transitions.flags.clone()
    own_reward = v.transitions.reward.clone()
    own_done = ((flags & (pglib.TR_TERMINATED | pglib.TR_TRUNCATED)) != 0)
    own_void = ((flags & pglib.TR_VOID) != 0) | ((flags & pglib.TR_RECORDED) == 0)
    own_action = v.transitions.action.clone()
    envs_l = envs.long()

    def torch_fold():
        """The n-step fold over [T, N] tensors: n rounds of indexing and arithmetic, each a handful of launches."""
        ret = torch.zeros(B, device="cuda")
        disc = torch.ones(B, device="cuda")
        m = torch.zeros(B, dtype=torch.int64, device="cuda")
        alive = torch.ones(B, dtype=torch.bool, device="cuda")
        ended = torch.zeros(B, dtype=torch.bool, device="cuda")
        for k in range(steps_n):
            q = pushes + k
            slot = q % T
            alive = alive & (q + 1 < head) & ~own_void[slot, envs_l]
            ret = torch.where(alive, ret + disc * own_reward[slot, envs_l], ret)
            disc = torch.where(alive, disc * gamma, disc)
            m = m + alive
            ended = ended | (alive & own_done[slot, envs_l])
            alive = alive & ~ended
        return own_action[pushes % T, envs_l], ret, torch.where(ended, torch.zeros_like(disc), disc), m

    def torch_way():
        act, ret, disc, m = torch_fold()
        obs = v.history_gather(pushes, envs, stack=K, dtype="float16")
        nxt = v.history_gather(pushes + m, envs, stack=K, dtype="float16")
        return obs, nxt, act, ret, disc, m

    with torch.cuda.stream(v._stream):
        got = v.transition_gather(pushes, envs, n=steps_n, gamma=gamma, stack=K, dtype="float16")
        ref = torch_way()
        plain = (got.status & pglib.TR_CUT) == 0  # (the torch fold above knows no began bytes)
        valid = (got.status & 1) != 0
        agree = bool((got.steps[plain & valid] == ref[5][plain & valid]).all()) and bool(torch.allclose(got.nstep_return[plain & valid], ref[3][plain & valid], rtol=1e-5, atol=1e-6))
    v._stream.synchronize()
    assert agree, "the torch fold and the gather disagree on entries no reset cut"
    g = regions([("transition_gather", v._stream, on_stream(v, lambda: v.transition_gather(pushes, envs, n=steps_n, gamma=gamma, stack=K, dtype="float16"))),
                 ("two_gathers_and_torch_fold", v._stream, on_stream(v, torch_way)),
                 ("transition_gather_scalars", v._stream, on_stream(v, lambda: v.transition_gather(pushes, envs, n=steps_n, gamma=gamma, frames=False))),
                 ("torch_fold", v._stream, on_stream(v, torch_fold))])
    result.update({"entries": B, "n": steps_n, "stack": K, "dtype": "float16", "gather_ms": g,
                   "gather_valid_fraction": float(valid.float().mean())})
    print("gather   %d entries, n=%d, K=%d f16 gray: transition_gather %.4f ms (spread %.1f %%) | two history_gather + torch fold %.4f ms (spread %.1f %%) | "
          "scalars alone %.4f ms | torch fold alone %.4f ms" % (B, steps_n, K, g["transition_gather"][0], spread(g["transition_gather"]),
                                                            g["two_gathers_and_torch_fold"][0], spread(g["two_gathers_and_torch_fold"]),
                                                            g["transition_gather_scalars"][0], g["torch_fold"][0]), flush=True)
    v.close()
    del v, flags, own_reward, own_done, own_void, own_action
    torch.cuda.empty_cache()
    # -- GAE ------------------------------------------------------------------------------------------------
    L, n = a.gae_steps, a.gae_envs
    v = ProcgenVecEnv(a.game, n, seed_base=1, history=dict(capacity=L + 1, gray=True), transitions=True)
    warm(v, L + 8)
    gamma, lam = 0.999, 0.95
    first = v.history.head - 1 - L
    gen.manual_seed(6)
    V = torch.randn((L + 1, n), generator=gen, device="cuda")
    order = [(first + t) % (L + 1) for t in range(L)]
    rew = v.transitions.reward[order].clone()
    fl = v.transitions.flags[order]
    term = ((fl & pglib.TR_TERMINATED) != 0).float()
    skip = (fl & pglib.TR_VOID) != 0

    def torch_gae():
        adv = torch.empty((L, n), device="cuda")
        last = torch.zeros(n, device="cuda")
        for t in range(L - 1, -1, -1):
            live = 1.0 - term[t]
            delta = rew[t] + gamma * V[t + 1] * live - V[t]
            last = torch.where(skip[t], torch.zeros_like(last), delta + gamma * lam * live * last)
            adv[t] = last
        return adv, adv + V[:L]

    with torch.cuda.stream(v._stream):
        adv, ret = v.transition_gae(first, L, V, gamma=gamma, lam=lam)
        ref_adv, _ = torch_gae()
        close = bool(torch.allclose(adv, ref_adv, rtol=1e-3, atol=1e-3))  # (no reset from outside in this run: no row is CUT)
    v._stream.synchronize()
    assert close, "the torch loop and transition_gae disagree"
    e = regions([("transition_gae", v._stream, on_stream(v, lambda: v.transition_gae(first, L, V, gamma=gamma, lam=lam))),
                 ("torch_loop", v._stream, on_stream(v, torch_gae))], calls=4)
    moved = L * n * (4 + 1 + 1 + 4 + 4 + 4) + n * 4  # reward, flags, began and values read, advantages and returns written
    result.update({"gae_envs": n, "gae_steps": L, "gae_ms": e, "gae_bytes": moved, "gae_GBps": 1e-6 * moved / e["transition_gae"][0]})
    print("gae      L=%d, %d envs: transition_gae %.4f ms (spread %.1f %%), %.0f GB/s | torch loop %.4f ms (spread %.1f %%)" % (
        L, n, e["transition_gae"][0], spread(e["transition_gae"]), result["gae_GBps"], e["torch_loop"][0], spread(e["torch_loop"])), flush=True)
    v.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
