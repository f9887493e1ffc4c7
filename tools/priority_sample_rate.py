#!/usr/bin/env python
"""What prioritised sampling over the transition ring costs (include/procgen2_vec.h pgv_priorities_enable), and what it replaces.

In one process, after --warmup steps that fill the ring, each region measured the same way: two HIP events on the env's stream
round --calls calls, --repeats times, the median with its minimum and maximum, the variants INTERLEAVED (every repeat measures
one region of each in turn).
    sample   transition_sample of --count (4 096) rows over a ring of --capacity x --envs (128 x 16 384) rows: three launches —
             beside the torch expression a learner writes without it: a validity mask from `flags` and head, a masked float64
             cumsum over T*N elements, searchsorted, and the pushes and envs of the rows found.
    set      transition_priorities of --count entries: one launch.
    step     milliseconds a step of pgv_step_synthetic of --game with the record ring alone (off) and with the priorities
             beside it (on: one more launch a step, 4 bytes written per env).
Before anything is timed the sample is held to the torch mask: every row drawn is one the mask calls valid, and the totals are
the mask's sums.

    python tools/priority_sample_rate.py [--json out.json]
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
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--capacity", type=int, default=128)
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=136)
    ap.add_argument("--calls", type=int, default=256, help="calls a region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
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
                for _ in range(a.calls):
                    call()
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.calls)
        return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}

    def stepper(env):
        return lambda: pglib.check(env.L, env.L.pgv_step_synthetic(env._h, a.run_seed), "pgv_step_synthetic")

    def on_stream(env, f):
        def call():
            with torch.cuda.stream(env._stream):
                f()
        return call

    def spread(r):
        return 100.0 * (r[2] - r[1]) / r[0]

    T, n, B = a.capacity, a.envs, a.count
    ring = dict(capacity=T, gray=True)
    engines = {"off": ProcgenVecEnv(a.game, n, seed_base=1, history=ring, transitions=True),
               "on": ProcgenVecEnv(a.game, n, seed_base=1, history=ring, transitions=True, priorities=True)}
    for e in engines.values():
        e.reset()
        for _ in range(a.warmup):
            stepper(e)()
        e.sync()
    result = {"game": a.game, "envs": n, "capacity": T, "count": B, "calls": a.calls, "repeats": a.repeats, "warmup": a.warmup}
    r = regions([(name, e._stream, stepper(e)) for name, e in engines.items()])
    assert bool((engines["on"].obs == engines["off"].obs).all()), "the engines left the same rollout"
    result["step_ms"] = r
    result["step_adds_ms"] = r["on"][0] - r["off"][0]
    print("%-8s step, %d envs, T=%d: ring alone %.4f ms (spread %.1f %%) | priorities on %.4f ms (spread %.1f %%), +%.4f ms" % (
        a.game, n, T, r["off"][0], spread(r["off"]), r["on"][0], spread(r["on"]), result["step_adds_ms"]), flush=True)
    engines.pop("off").close()
    v = engines["on"]
    torch.cuda.empty_cache()

    head = v.history.head
    flags, priority = v.transitions.flags, v.transitions.priority
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    with torch.cuda.stream(v._stream):
        first = v.transition_sample(B, 1)
        v.transition_priorities(first.pushes, first.envs, torch.rand(B, generator=gen, device="cuda") * 4.0)  # some spread of weights
    slots = torch.arange(T, device="cuda")
    rows = head - 1 - (head - 1 - slots) % T  # the row living in every slot (head >= T here)
    held = (rows >= 0) & (rows + 1 < head)

    def torch_way():
        """The same draw in torch: mask, masked cumsum in float64 (exact below 2^53), search, the rows' pushes and envs."""
        ok = held[:, None] & ((flags & pglib.TR_RECORDED) != 0) & ((flags & pglib.TR_VOID) == 0)
        w = torch.where(ok, priority, torch.zeros_like(priority)).reshape(-1).to(torch.float64)
        cum = torch.cumsum(w, 0)
        total = cum[-1]
        strata = (torch.arange(B, device="cuda", dtype=torch.float64) + torch.rand(B, generator=gen, device="cuda", dtype=torch.float64)) / B
        j = torch.searchsorted(cum, strata * total, right=True).clamp_(max=T * n - 1)
        return rows[j // n], (j % n).to(torch.int32), w[j] / total, total, ok.sum()

    with torch.cuda.stream(v._stream):
        got = v.transition_sample(B, 2)
        ref = torch_way()
        ok = held[:, None] & ((flags & pglib.TR_RECORDED) != 0) & ((flags & pglib.TR_VOID) == 0)
        agree = (bool(ok[got.pushes % T, got.envs.long()].all()) and int(got.total) == int(ref[3]) and int(got.eligible) == int(ref[4])
                 and bool((priority[got.pushes % T, got.envs.long()] == got.priority).all()))
    v._stream.synchronize()
    assert agree, "the sample and the torch mask disagree"
    values = torch.rand(B, generator=gen, device="cuda") * 4.0
    g = regions([("transition_sample", v._stream, on_stream(v, lambda: v.transition_sample(B, 2))),
                 ("torch_mask_cumsum_search", v._stream, on_stream(v, torch_way)),
                 ("transition_priorities", v._stream, on_stream(v, lambda: v.transition_priorities(got.pushes, got.envs, values)))])
    moved = T * n * 5  # priority and flags, read once by the chunk sums
    result.update({"sample_ms": g, "ring_rows": T * n, "eligible": int(got.eligible), "scan_bytes": moved})
    print("sample   %d of %d x %d rows (%d eligible): transition_sample %.4f ms (spread %.1f %%) | torch mask + cumsum + searchsorted %.4f ms "
          "(spread %.1f %%) | transition_priorities of %d %.4f ms (spread %.1f %%)" % (
              B, T, n, int(got.eligible), g["transition_sample"][0], spread(g["transition_sample"]), g["torch_mask_cumsum_search"][0],
              spread(g["torch_mask_cumsum_search"]), B, g["transition_priorities"][0], spread(g["transition_priorities"])), flush=True)
    v.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
