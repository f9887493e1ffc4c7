#!/usr/bin/env python
"""Cost of the symbolic observations (pgv_state_rows / pgv_tile_rows, include/procgen2_vec.h) beside a plain device copy
and beside the game's own step.

Per game, at --envs envs (65 536): the HIP-event time, on the env's stream, of pgv_state_rows over EVERY env — indices NULL,
and a random permutation — and of pgv_tile_rows over every env, `--repeats` times after `--warmups`, the median.  In the
same process, on the same device, one hipMemcpyAsync device-to-device of the same number of OUTPUT bytes (count × width × 4
for the rows, count × cells for the tiles): boxes differ in what they copy at, so only the ratio taken inside one run means
anything — and a copy reads as many bytes as it writes, while a state row's sources are a fraction of its width (the rest is
the +0.0 behind the dump).  And the game's own step from pgv_timed_steps (no per-launch events), the yardstick for "is a
call per step affordable".

    python tools/state_obs_rate.py [--games coinrun chaser] [--mode extreme] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
from ctypes import c_void_p

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", nargs="*", default=None)
    ap.add_argument("--mode", default=None, help="distribution mode (default: the game's own)")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64, help="synthetic steps before the measurement, and steps of the timed run")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import GAMES, ProcgenVecEnv
    hip = ctypes.CDLL("libamdhip64.so")  # (the runtime torch has loaded: one per process, procgen2_amd/lib.py)
    hip.hipMemcpyAsync.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int, c_void_p]
    D2D = 3

    def timed(stream, fn):
        """Median milliseconds of fn() between two events on `stream`."""
        ms = []
        for k in range(a.warmups + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if k >= a.warmups:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    out = []
    for game in a.games or GAMES:
        env = ProcgenVecEnv(game, a.envs, seed_base=1, distribution_mode=a.mode)
        L, h, st, lay = env.L, env._h, env._stream, env.state_layout
        env.reset()
        for _ in range(a.steps):
            env.step_synthetic(3)
        torch.cuda.synchronize()
        n = a.envs
        rows = torch.empty((n, lay.width), dtype=torch.float32, device=env.device)
        lengths = torch.empty(n, dtype=torch.int32, device=env.device)
        tiles = torch.empty((n, max(lay.cells, 1)), dtype=torch.uint8, device=env.device)
        row_bytes, tile_bytes = n * lay.width * 4, n * lay.cells
        src = torch.empty(max(row_bytes, tile_bytes), dtype=torch.uint8, device=env.device)  # the plain copy's two ends
        other = torch.empty_like(src)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(env.device)
        torch.cuda.synchronize()

        def state(idx):
            pglib.check(L, L.pgv_state_rows(h, c_void_p(idx.data_ptr()) if idx is not None else None, n, c_void_p(rows.data_ptr()),
                                            c_void_p(lengths.data_ptr())), "pgv_state_rows")

        def tile():
            pglib.check(L, L.pgv_tile_rows(h, None, n, c_void_p(tiles.data_ptr())), "pgv_tile_rows")

        def copy(nbytes):
            assert hip.hipMemcpyAsync(c_void_p(other.data_ptr()), c_void_p(src.data_ptr()), nbytes, D2D, c_void_p(st.cuda_stream)) == 0

        state(None)
        torch.cuda.synchronize()
        used = float(lengths.float().mean()) / lay.width  # the share of a row that is dump, not padding
        r = {"game": game, "mode": env.distribution_mode, "envs": n, "width": lay.width, "cells": lay.cells, "dump_share": used,
             "state_ms": timed(st, lambda: state(None)), "state_perm_ms": timed(st, lambda: state(perm)),
             "state_copy_ms": timed(st, lambda: copy(row_bytes))}
        if lay.cells:
            r["tiles_ms"] = timed(st, tile)
            r["tiles_copy_ms"] = timed(st, lambda: copy(tile_bytes))
        total, _ = env.timed_steps(a.steps, run_seed=3, render_events=False)
        r["step_ms"] = total / a.steps
        r["state_of_copy"] = r["state_ms"] / r["state_copy_ms"]
        r["state_perm_of_copy"] = r["state_perm_ms"] / r["state_copy_ms"]
        r["state_of_step"] = r["state_ms"] / r["step_ms"]
        text = ("%-9s width %4d (%2.0f %% dump)  step %6.3f ms | state %6.3f ms = %4.2f x its copy (%6.3f), %4.2f of a step; permuted %6.3f ms = %4.2f x"
                % (game, lay.width, 100 * used, r["step_ms"], r["state_ms"], r["state_of_copy"], r["state_copy_ms"], r["state_of_step"],
                   r["state_perm_ms"], r["state_perm_of_copy"]))
        if lay.cells:
            r["tiles_of_copy"] = r["tiles_ms"] / r["tiles_copy_ms"]
            r["tiles_of_step"] = r["tiles_ms"] / r["step_ms"]
            text += " | tiles %4d B: %6.3f ms = %4.2f x its copy (%6.3f), %4.2f of a step" % (
                lay.cells, r["tiles_ms"], r["tiles_of_copy"], r["tiles_copy_ms"], r["tiles_of_step"])
        print(text, flush=True)
        out.append(r)
        env.close()
        del rows, src, other, tiles
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
