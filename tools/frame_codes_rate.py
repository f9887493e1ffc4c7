#!/usr/bin/env python
"""What frame codes over the frame ring cost (include/procgen2_vec.h pgv_frame_codes), beside the torch expression they replace.

In one process, per case (gray or RGB ring, bits) an engine of --game with --envs envs and a ring of --slots slots, stepped until
the ring is full; --entries random (push, env) pairs; each region two HIP events on the env's stream round --calls calls,
--repeats times, the median with its minimum and maximum, the regions INTERLEAVED (every repeat measures one region of each in turn).
    project  pgv_frame_codes with codes and valid, no counting: one launch.
    add      the same with count = add and visits: two launches.
    torch    index the ring, cast to float32, centre, matmul against the float weights, sign, pack to int64 words.
Before anything is timed the engine's codes are held to numpy in int64 on the first --check entries.  GB/s is the entries' frame
bytes over the call's time: what a device-to-device copy of as many bytes is beside (`bench.py --full` prints that rate).

    python tools/frame_codes_rate.py [--json out.json] [--cases gray:64,gray:256,rgb:64,rgb:256]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="coinrun")
    ap.add_argument("--cases", default="gray:64,gray:256,rgb:64,rgb:256")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--entries", type=int, default=16384)
    ap.add_argument("--table", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--calls", type=int, default=16, help="calls a region")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    def regions(group):
        ms = {name: [] for name, _, _ in group}
        for _ in range(a.repeats):
            for name, call, calls in group:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(v._stream)
                for _ in range(calls):
                    call()
                e1.record(v._stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / calls)
        return {name: (statistics.median(x), min(x), max(x)) for name, x in ms.items()}

    result = {"game": a.game, "envs": a.envs, "slots": a.slots, "entries": a.entries, "table": a.table, "calls": a.calls, "repeats": a.repeats,
              "rows_a_tile": pglib.FRAME_CODE_ROWS, "lib": os.environ.get("PROCGEN2_HIP_LIB", "default"), "cases": []}
    gen = torch.Generator(device="cuda")
    for case in a.cases.split(","):
        planes, bits = case.split(":")
        gray, bits = planes == "gray", int(bits)
        v = ProcgenVecEnv(a.game, a.envs, seed_base=1, history=dict(capacity=a.slots, gray=gray), frame_codes=dict(bits=bits, seed=1, table=a.table))
        v.reset()
        for _ in range(a.slots + 2):
            pglib.check(v.L, v.L.pgv_step_synthetic(v._h, a.run_seed), "pgv_step_synthetic")
        v.sync()
        head, T, n, B = v.history.head, a.slots, a.envs, a.entries
        D = v.history.frames.shape[2] * 4096
        gen.manual_seed(4)
        p = torch.randint(head - T, head, (B,), generator=gen, device="cuda", dtype=torch.int64)
        e = torch.randint(0, n, (B,), generator=gen, device="cuda", dtype=torch.int32)
        codes = torch.zeros((B, bits // 32), dtype=torch.int32, device="cuda")
        valid = torch.zeros(B, dtype=torch.uint8, device="cuda")
        visits = torch.zeros(B, dtype=torch.int32, device="cuda")
        q_project = pglib.frame_code_query(None, codes=codes.data_ptr(), valid=valid.data_ptr())
        q_add = pglib.frame_code_query("add", codes=codes.data_ptr(), valid=valid.data_ptr(), visits=visits.data_ptr())

        def engine(q):
            def call():
                pglib.check(v.L, v.L.pgv_frame_codes(v._h, p.data_ptr(), e.data_ptr(), B, ctypes.byref(q)), "pgv_frame_codes")
            return call

        rows = v.history.frames.view(T * n, D)
        index = (p % T) * n + e.to(torch.int64)
        wf = v.frame_code_table.weights.float()
        shifts = torch.arange(32, device="cuda", dtype=torch.int64)

        def torch_codes():
            with torch.cuda.stream(v._stream):
                proj = (rows[index].float() - 128.0) @ wf.T
                return ((proj >= 0).view(B, -1, 32).to(torch.int64) << shifts).sum(-1)

        engine(q_project)()
        v._stream.synchronize()
        k = min(a.check, B)
        w64 = v.frame_code_table.weights.cpu().numpy().astype(np.int64)
        x64 = rows[index[:k]].cpu().numpy().astype(np.int64) - 128
        want = (((x64 @ w64.T) >= 0).reshape(k, -1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
        assert bool(valid.all()) and np.array_equal(codes[:k].cpu().numpy().view(np.uint32), want), "the engine's codes and int64 numpy disagree"
        for call in (engine(q_project), engine(q_add), torch_codes):  # every region warm
            call()
        r = regions([("project", engine(q_project), a.calls), ("add", engine(q_add), a.calls), ("torch", torch_codes, 2)])
        row = {"planes": planes, "bits": bits, "ms": r, "project_GBps": 1e-6 * B * D / r["project"][0], "add_GBps": 1e-6 * B * D / r["add"][0],
               "torch_over_project": r["torch"][0] / r["project"][0], "used": int(v.frame_code_table.used), "dropped": int(v.frame_code_table.dropped)}
        result["cases"].append(row)
        print("%-8s %-4s %3d bits, %d entries: " % (a.game, planes, bits, B) +
              " | ".join("%s %.4f ms [%.4f .. %.4f] (spread %.1f %%)" % (name, *r[name], 100.0 * (r[name][2] - r[name][1]) / r[name][0]) for name in r) +
              " | project %.0f GB/s, add %.0f GB/s of frame bytes | torch / project %.1f" % (row["project_GBps"], row["add_GBps"], row["torch_over_project"]), flush=True)
        v.close()
        del v, rows, wf, codes, valid, visits, p, e, index
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
