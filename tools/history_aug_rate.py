#!/usr/bin/env python
"""What augmenting inside the history gather costs (include/procgen2_vec.h pgv_history_gather_aug).

One game, --envs envs (65 536), a ring of --capacity slots (16), filled by stepping; then, for each of --rows (16 384 and
65 536) random (push, env) pairs over the held pushes, K = 4, RGB, --dtype (float16), in one process, every variant measured
the same way: two HIP events on the stream round --calls calls, --repeats times, the median, the variants INTERLEAVED (every
repeat measures one region of each in turn):
    a  plain          pgv_history_gather;
    b  shift          pgv_history_gather_aug at 64 x 64 with pad 4: the same bytes read and written as (a);
    c  crop_cutout    pgv_history_gather_aug at 56 x 56 with pad 0 and a cutout of 8 .. 24;
    d  torch          the torch expression (b) replaces, on (a)'s output: F.pad(mode="replicate") by 4, then every row's own
                      64 x 64 window — the gathered rows moved at least twice more — in two forms, advanced indexing
                      (torch_index) and torch.gather down and along the rows (torch_gather), --torch-chunk rows at a time
                      (replicate padding takes at most 2^31 elements); (d) is the faster one.  (a) is not in its time.
Before anything is timed, both forms of (d) fed with (b)'s own draws must give (b)'s rows bit for bit.
Ratios: b/a (what the augmentation adds to the gather), d/b and (a + d)/b (what doing it in torch costs beside it).

    python tools/history_aug_rate.py [--game maze] [--json out.json]
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
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--rows", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--calls", type=int, default=16, help="calls a region")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--run-seed", type=int, default=3)
    ap.add_argument("--dtype", default="float16", choices=["uint8", "float16", "bfloat16", "float32"])
    ap.add_argument("--torch-chunk", type=int, default=16384, help="rows the torch expression pads at a time")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

    K, T, n, pad = 4, a.capacity, a.envs, 4
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

    def spread(r):
        return 100.0 * (r[2] - r[1]) / r[0]

    results = []
    for count in a.rows:
        pushes = torch.randint(max(0, head - T), head, (count,), generator=gen, device="cuda", dtype=torch.int64)
        envs = torch.randint(0, n, (count,), generator=gen, device="cuda", dtype=torch.int32)
        out_plain = torch.empty((count, K * 3, 64, 64), dtype=tdtype, device="cuda")
        out_shift = torch.empty_like(out_plain)
        out_crop = torch.empty((count, K * 3, 56, 56), dtype=tdtype, device="cuda")
        params = torch.empty((count, 8), dtype=torch.int32, device="cuda")
        shift = pglib.gather_aug(64, 64, pad, "replicate", 0, 0, "black", 1, params.data_ptr())
        crop = pglib.gather_aug(56, 56, 0, "replicate", 8, 24, "random", 1, None)

        def plain():
            pglib.check(env.L, env.L.pgv_history_gather(env._h, pushes.data_ptr(), envs.data_ptr(), count, K, number, out_plain.data_ptr()), "pgv_history_gather")

        def augmented(aug, out):
            def call():
                pglib.check(env.L, env.L.pgv_history_gather_aug(env._h, pushes.data_ptr(), envs.data_ptr(), count, K, number, aug, out.data_ptr()),
                            "pgv_history_gather_aug")
            return call

        shifted, cropped = augmented(pglib.ctypes.byref(shift), out_shift), augmented(pglib.ctypes.byref(crop), out_crop)
        plain(), shifted(), cropped()
        env.sync()
        # what torch does with the plain rows for the same windows (the params row: oy, ox, ...), --torch-chunk rows at a time:
        # replicate padding refuses more than 2^31 elements at once
        chunk = min(count, a.torch_chunk)
        rows_at = torch.arange(chunk, device="cuda")[:, None, None, None]
        planes_at = torch.arange(K * 3, device="cuda")[None, :, None, None]
        ys = (params[:, 0].long() + pad)[:, None, None, None] + torch.arange(64, device="cuda")[None, None, :, None]
        xs = (params[:, 1].long() + pad)[:, None, None, None] + torch.arange(64, device="cuda")[None, None, None, :]
        out_torch = torch.empty_like(out_plain)

        def torch_index():  # every row's window by advanced indexing
            with torch.cuda.stream(stream):
                for at in range(0, count, chunk):
                    padded = F.pad(out_plain[at:at + chunk], (pad, pad, pad, pad), mode="replicate")
                    m = padded.shape[0]
                    out_torch[at:at + chunk] = padded[rows_at[:m], planes_at, ys[at:at + chunk], xs[at:at + chunk]]

        def torch_gather():  # … by torch.gather down the rows, then along them
            with torch.cuda.stream(stream):
                for at in range(0, count, chunk):
                    padded = F.pad(out_plain[at:at + chunk], (pad, pad, pad, pad), mode="replicate")
                    m = padded.shape[0]
                    tall = padded.gather(2, ys[at:at + chunk].expand(m, K * 3, 64, 64 + 2 * pad))
                    torch.gather(tall, 3, xs[at:at + chunk].expand(m, K * 3, 64, 64), out=out_torch[at:at + chunk])

        same = True
        for call in (torch_index, torch_gather):
            out_torch.zero_()
            call()
            torch.cuda.synchronize()
            same = same and bool((out_torch.view(torch.uint8) == out_shift.view(torch.uint8)).all())
        assert same, "the torch expressions and the augmented gather disagree"
        group = [("plain", plain), ("shift", shifted), ("crop_cutout", cropped), ("torch_index", torch_index), ("torch_gather", torch_gather)]
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
        # the ratios repeat by repeat, so that their spread is that of the pair and not of the two medians
        def ratio(top, bottom):
            v = [sum(ms[t][k] for t in top) / ms[bottom][k] for k in range(1, a.repeats + 1)]
            return (statistics.median(v), min(v), max(v))

        best = min(("torch_index", "torch_gather"), key=lambda name: r[name][0])  # (d): the faster of the two torch forms
        ratios = {"shift/plain": ratio(["shift"], "plain"), "crop_cutout/plain": ratio(["crop_cutout"], "plain"),
                  "torch/shift": ratio([best], "shift"), "(plain+torch)/shift": ratio(["plain", best], "shift")}
        bytes_moved = {"plain": count * K * 3 * 4096 * (1 + es), "shift": count * K * 3 * 4096 * (1 + es), "crop_cutout": count * K * 3 * (4096 + 56 * 56 * es)}
        results.append({"game": a.game, "envs": n, "capacity": T, "rows": count, "stack": K, "dtype": a.dtype, "calls": a.calls, "repeats": a.repeats,
                        "ms": r, "ratios": ratios, "bytes": bytes_moved, "torch": best, "torch_chunk": chunk, "torch_equals_shift": same})
        print("%-8s %6d rows K=4 RGB %s: plain %.4f ms %.0f GB/s (spread %.1f %%) | shift 64x64 pad 4 %.4f ms %.0f GB/s (spread %.1f %%) | "
              "crop 56x56 cutout 8..24 %.4f ms %.0f GB/s (spread %.1f %%) | torch pad + windows: indexing %.4f ms (spread %.1f %%), gather %.4f ms (spread %.1f %%)" % (
                  a.game, count, a.dtype, r["plain"][0], 1e-6 * bytes_moved["plain"] / r["plain"][0], spread(r["plain"]), r["shift"][0],
                  1e-6 * bytes_moved["shift"] / r["shift"][0], spread(r["shift"]), r["crop_cutout"][0],
                  1e-6 * bytes_moved["crop_cutout"] / r["crop_cutout"][0], spread(r["crop_cutout"]), r["torch_index"][0], spread(r["torch_index"]), r["torch_gather"][0], spread(r["torch_gather"])), flush=True)
        print("%-8s %6d rows ratios, median (min .. max) over the repeats: shift/plain %.3f (%.3f .. %.3f) | crop/plain %.3f (%.3f .. %.3f) | "
              "torch/shift %.2f (%.2f .. %.2f) | (plain + torch)/shift %.2f (%.2f .. %.2f)" % (
                  (a.game, count) + ratios["shift/plain"] + ratios["crop_cutout/plain"] + ratios["torch/shift"] + ratios["(plain+torch)/shift"]),
              flush=True)
        del out_plain, out_shift, out_crop, out_torch
        torch.cuda.empty_cache()
    env.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
