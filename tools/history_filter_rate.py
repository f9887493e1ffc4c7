#!/usr/bin/env python
"""What filtering inside the history gather costs (include/procgen2_vec.h pgv_history_gather_filter).

One game, --envs envs (16 384), a ring of --capacity slots (8), filled by stepping; then, for each of --rows (2 048 and
16 384) random (push, env) pairs over the held pushes, K = 4, RGB, --dtype (float16), 64 x 64 with pad 4, one filter set
per row, a bias and a clamp to 0 .. 1, in one process, every variant measured the same way: two HIP events on the stream
round --calls calls, --repeats times, the median, the variants INTERLEAVED (every repeat measures one region of each in turn):
    a  aug        pgv_history_gather_aug of the same rows: the floor, the gather this one grew from;
    b  filter1    pgv_history_gather_filter, kernel 1 (a colour matrix per row);
    c  filter3    pgv_history_gather_filter, kernel 3 (a random convolution per row);
    d  torch1/3   the torch expression (b) and (c) replace: (a) with float32 rows, then einsum (kernel 1) or a grouped
                  conv2d with one group per row (kernel 3), the bias, clamp, and the cast — --torch-chunk rows at a time.
Before anything is timed, (d) must agree with (b) and (c) to 2^-9 (torch sums in another order and rounds to f16 as well).
Ratios: b/a and c/a (what the filter adds to the gather), d/b and d/c (what doing it in torch costs beside it).

    python tools/history_filter_rate.py [--game maze] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="maze")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--rows", type=int, nargs="*", default=[2048, 16384])
    ap.add_argument("--calls", type=int, default=8, help="calls a region")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16", "float32"])
    ap.add_argument("--torch-chunk", type=int, default=2048, help="rows the torch expression filters at a time")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    K, C, T, n, pad = 4, 3, a.capacity, a.envs, 4
    number, es = pglib.POLICY_DTYPES[a.dtype]
    tdtype = getattr(torch, a.dtype)
    env = ProcgenVecEnv(a.game, n, seed_base=1, history=dict(capacity=T, gray=False))
    env.reset()
    for _ in range(T + 3):  # the ring is full and has wrapped
        pglib.check(env.L, env.L.pgv_step_synthetic(env._h, a.run_seed), "pgv_step_synthetic")
    env.sync()
    head = env.history.head
    stream = env._stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)

    results = []
    for count in a.rows:
        pushes = torch.randint(max(0, head - T), head, (count,), generator=gen, device="cuda", dtype=torch.int64)
        envs = torch.randint(0, n, (count,), generator=gen, device="cuda", dtype=torch.int32)
        shape = (count, K * C, 64, 64)
        out = {name: torch.empty(shape, dtype=tdtype, device="cuda") for name in ("aug", "filter1", "filter3", "torch1", "torch3")}
        rows32 = torch.empty(shape, dtype=torch.float32, device="cuda")
        weights = {k: 0.2 * torch.randn((count, C, C, k, k), generator=gen, device="cuda") for k in (1, 3)}
        bias = 0.2 * torch.randn((count, C), generator=gen, device="cuda")
        aug = pglib.gather_aug(64, 64, pad, "replicate", 0, 0, "black", 1, None)
        filters = {k: pglib.gather_filter(k, weights[k].data_ptr(), bias.data_ptr(), C * C * k * k, C, (0.0, 1.0)) for k in (1, 3)}

        def augmented(dtype_number, to):
            def call():
                pglib.check(env.L, env.L.pgv_history_gather_aug(env._h, pushes.data_ptr(), envs.data_ptr(), count, K, dtype_number, pglib.ctypes.byref(aug),
                                                                to.data_ptr()), "pgv_history_gather_aug")
            return call

        def filtered(k):
            def call():
                pglib.check(env.L, env.L.pgv_history_gather_filter(env._h, pushes.data_ptr(), envs.data_ptr(), count, K, number, pglib.ctypes.byref(aug),
                                                                   pglib.ctypes.byref(filters[k]), out["filter%d" % k].data_ptr()), "pgv_history_gather_filter")
            return call

        gather32 = augmented(pglib.POLICY_DTYPES["float32"][0], rows32)
        chunk = min(count, a.torch_chunk)

        def torch_filter(k):
            def call():
                gather32()
                with torch.cuda.stream(stream):
                    for at in range(0, count, chunk):
                        x = rows32[at:at + chunk].view(-1, K, C, 64, 64)
                        m = x.shape[0]
                        if k == 1:
                            y = torch.einsum("boi,bkihw->bkohw", weights[1][at:at + m, :, :, 0, 0], x)
                        else:  # one group per row: the K frames are the batch, the rows' planes the channels
                            y = F.conv2d(x.transpose(0, 1).reshape(K, m * C, 64, 64), weights[3][at:at + m].reshape(m * C, C, 3, 3), padding=1, groups=m)
                            y = y.view(K, m, C, 64, 64).transpose(0, 1)
                        y = (y + bias[at:at + m, None, :, None, None]).clamp_(0.0, 1.0)
                        out["torch%d" % k][at:at + m] = y.reshape(m, K * C, 64, 64)
            return call

        group = [("aug", augmented(number, out["aug"])), ("filter1", filtered(1)), ("filter3", filtered(3)), ("torch1", torch_filter(1)), ("torch3", torch_filter(3))]
        for _, call in group:
            call()
        torch.cuda.synchronize()
        apart = {k: float((out["torch%d" % k].float() - out["filter%d" % k].float()).abs().max()) for k in (1, 3)}
        assert max(apart.values()) <= 2.0 ** -9 * (1 if a.dtype != "bfloat16" else 8), "the torch expression and the filtered gather disagree: %r" % apart
        ms = {name: [] for name, _ in group}
        for _ in range(a.repeats + 1):  # (the first round warms every shape and is dropped)
            for name, call in group:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    call()
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.calls)
        r = {name: (statistics.median(v[1:]), min(v[1:]), max(v[1:])) for name, v in ms.items()}

        def ratio(top, bottom):  # repeat by repeat, so that the spread is that of the pair
            v = [ms[top][k] / ms[bottom][k] for k in range(1, a.repeats + 1)]
            return (statistics.median(v), min(v), max(v))

        ratios = {"filter1/aug": ratio("filter1", "aug"), "filter3/aug": ratio("filter3", "aug"), "torch1/filter1": ratio("torch1", "filter1"),
                  "torch3/filter3": ratio("torch3", "filter3")}
        results.append({"game": a.game, "envs": n, "capacity": T, "rows": count, "stack": K, "dtype": a.dtype, "calls": a.calls, "repeats": a.repeats,
                        "ms": r, "ratios": ratios, "torch_chunk": chunk, "torch_apart": apart})
        print("%-8s %6d rows K=4 RGB %s 64x64 pad 4, ms median (min .. max): " % (a.game, count, a.dtype) +
              " | ".join("%s %.4f (%.4f .. %.4f)" % ((name,) + r[name]) for name, _ in group), flush=True)
        print("%-8s %6d rows ratios, median (min .. max) over the repeats: " % (a.game, count) +
              " | ".join("%s %.2f (%.2f .. %.2f)" % ((name,) + v) for name, v in ratios.items()), flush=True)
        del out, rows32, weights
        torch.cuda.empty_cache()
    env.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
