#!/usr/bin/env python
"""What V-trace over the transition ring costs (include/procgen2_vec.h pgv_transitions_vtrace), beside GAE and beside torch.

In one process, per shape (envs x L) an engine of --game with a gray ring of L + 1 slots, stepped L + 8 times; each region two HIP
events on the env's stream round --calls calls, --repeats times, the median with its minimum and maximum, the regions
INTERLEAVED (every repeat measures one region of each in turn).
    gae      transition_gae: the lane-per-env kernel as it stands.  The yardstick.
    vtrace   transition_vtrace with ratios and advantages.
    torch    the same recurrence as L dependent torch steps over [L, N] tensors (first shape only); held to `vtrace` within
             1e-3 before it is timed.
Bytes a cell: gae reads flags 1, began 1, reward 4, value 4 and writes two floats: 18; vtrace reads the ratio as well: 22.

    python tools/vtrace_rate.py [--json out.json] [--shapes 16384x256,1024x256,65536x64]
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
    ap.add_argument("--shapes", default="16384x256,1024x256,65536x64", help="envs x L, the first one also in torch")
    ap.add_argument("--calls", type=int, default=32, help="calls a region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    def regions(group):
        """group: (name, stream, call, calls).  One region of each in turn, --repeats times → {name: (median, min, max)} ms a call."""
        ms = {name: [] for name, _, _, _ in group}
        for _ in range(a.repeats):
            for name, st, call, calls in group:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(calls):
                    call()
                e1.record(st)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / calls)
        return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}

    def spread(r):
        return 100.0 * (r[2] - r[1]) / r[0]

    gamma, lam, bars = 0.999, 0.95, (1.0, 1.0, 1.0)
    result = {"game": a.game, "calls": a.calls, "repeats": a.repeats, "gamma": gamma, "lam": lam, "rows_a_chunk": pglib.VTRACE_ROWS, "shapes": []}
    gen = torch.Generator(device="cuda")
    for k, shape in enumerate(a.shapes.split(",")):
        n, L = (int(x) for x in shape.split("x"))
        v = ProcgenVecEnv(a.game, n, seed_base=1, history=dict(capacity=L + 1, gray=True), transitions=True)
        v.reset()
        for _ in range(L + 8):
            pglib.check(v.L, v.L.pgv_step_synthetic(v._h, a.run_seed), "pgv_step_synthetic")
        v.sync()
        first = v.history.head - 1 - L
        gen.manual_seed(6)
        V = torch.randn((L + 1, n), generator=gen, device="cuda")
        rho = torch.exp(0.5 * torch.randn((L, n), generator=gen, device="cuda"))

        def on_stream(f):
            def call():
                with torch.cuda.stream(v._stream):
                    f()
            return call

        def gae():
            return v.transition_gae(first, L, V, gamma=gamma, lam=lam)

        def vtrace():
            return v.transition_vtrace(first, L, V, rho, gamma, lam, *bars)

        order = [(first + t) % (L + 1) for t in range(L)]
        rew = v.transitions.reward[order].clone()
        fl = v.transitions.flags[order]
        live = 1.0 - ((fl & pglib.TR_TERMINATED) != 0).float()  # (no reset from outside and no limit in this run: no row is CUT or TRUNCATED)
        skip = (fl & pglib.TR_VOID) != 0
        rc, cc, pr = rho.clamp(max=bars[0]), lam * rho.clamp(max=bars[1]), rho.clamp(max=bars[2])

        def torch_vtrace():
            vs, pg = torch.empty((L, n), device="cuda"), torch.empty((L, n), device="cuda")
            x, nxt = torch.zeros(n, device="cuda"), V[L]
            for t in range(L - 1, -1, -1):
                delta = rc[t] * (rew[t] + gamma * V[t + 1] * live[t] - V[t])
                x = torch.where(skip[t], torch.zeros_like(x), delta + gamma * cc[t] * live[t] * x)
                pg[t] = torch.where(skip[t], torch.zeros_like(x), pr[t] * (rew[t] + gamma * nxt * live[t] - V[t]))
                nxt = x + V[t]
                vs[t] = nxt
            return vs, pg

        group = [("gae", v._stream, on_stream(gae), a.calls), ("vtrace", v._stream, on_stream(vtrace), a.calls)]
        with torch.cuda.stream(v._stream):
            vs, pg = vtrace()
            ret = gae()[1]
            if k == 0:
                ref_vs, ref_pg = torch_vtrace()
                close = bool(torch.allclose(vs, ref_vs, rtol=1e-3, atol=1e-3)) and bool(torch.allclose(pg, ref_pg, rtol=1e-3, atol=1e-3))
                group.append(("torch", v._stream, on_stream(torch_vtrace), 2))
        v._stream.synchronize()
        assert k != 0 or close, "the torch loop and transition_vtrace disagree"
        assert vs.shape == ret.shape
        for _ in range(2):  # every shape warm
            gae(), vtrace()
        r = regions(group)
        cells = L * n
        row = {"envs": n, "L": L, "ms": r, "gae_GBps": 1e-6 * (18 * cells + 4 * n) / r["gae"][0], "vtrace_GBps": 1e-6 * (22 * cells + 4 * n) / r["vtrace"][0],
               "vtrace_over_gae": r["vtrace"][0] / r["gae"][0]}
        result["shapes"].append(row)
        print("%-8s %6d envs x L=%3d: transition_gae %.4f ms [%.4f .. %.4f] (spread %.1f %%), %.0f GB/s | transition_vtrace %.4f ms [%.4f .. %.4f] "
              "(spread %.1f %%), %.0f GB/s | vtrace / gae %.3f%s" % (
                  a.game, n, L, *r["gae"], spread(r["gae"]), row["gae_GBps"], *r["vtrace"], spread(r["vtrace"]), row["vtrace_GBps"], row["vtrace_over_gae"],
                  " | torch loop %.3f ms (spread %.1f %%)" % (r["torch"][0], spread(r["torch"])) if "torch" in r else ""), flush=True)
        v.close()
        del v, V, rho, rew, fl, live, skip, rc, cc, pr, vs, pg, ret
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
