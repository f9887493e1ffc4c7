#!/usr/bin/env python
"""Cost of the path distances (pgv_tile_paths_rows, include/procgen2_vec.h) beside the copy it cannot beat, beside the game's
own step, and beside the torch dilation loop it replaces.

Per case — maze, chaser, coinrun and caveflyer in memory mode — at --envs envs (65 536), over EVERY env (indices NULL), with
passable = {0}, source = the goal where the game has one (probe = the agent), else the agent:
  * the HIP-event time, on the env's stream, of the whole call (distances, probe distance, step code, cells) and of the call
    with dist = NULL (the probe's answers alone: what a scripted policy asks for each step), `--repeats` times after
    `--warmups`, the median;
  * in the same process, pgv_tile_rows of the same rows: the call reads every map once as that one does, and writes two
    bytes a cell where that one writes one — the copy it cannot beat;
  * the game's own step from pgv_timed_steps (no per-launch events);
  * the torch dilation loop over tile_obs(): per BFS level four shifted ORs, an and, an and-not, an any() that the host waits
    for, and a torch.where for the distances, run to the same fixed point from the same source cells, timed by the wall clock
    around a device synchronisation (`--loop-repeats` times, the median) and CHECKED EQUAL to the call's distances.
Boxes differ, so only the ratios taken inside one run mean anything.

    python tools/tile_paths_rate.py [--cases maze coinrun] [--envs 65536] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from ctypes import c_void_p

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"maze": ("maze", None), "chaser": ("chaser", None), "coinrun": ("coinrun", None), "caveflyer-memory": ("caveflyer", "memory")}


def dilation_loop(torch, tiles, source_cells, tile_w, tile_h, passable):
    """(int16 [n, cells], levels): the field by whole-batch dilation, cell (x, y) at [x][y] as the tile rows lie."""
    n = tiles.shape[0]
    may = torch.zeros(256, dtype=torch.bool, device=tiles.device)
    may[list(passable)] = True
    open_ = may[tiles.long()].view(n, tile_w, tile_h)
    has = source_cells >= 0
    front = torch.zeros((n, tile_w * tile_h), dtype=torch.bool, device=tiles.device)
    front[has.nonzero().squeeze(1), source_cells[has].long()] = True
    front = front.view(n, tile_w, tile_h)
    seen = front.clone()
    dist = torch.where(front, 0, -1).to(torch.int16)
    level = 0
    while True:
        level += 1
        near = torch.zeros_like(front)
        near[:, 1:, :] |= front[:, :-1, :]
        near[:, :-1, :] |= front[:, 1:, :]
        near[:, :, 1:] |= front[:, :, :-1]
        near[:, :, :-1] |= front[:, :, 1:]
        front = near & open_ & ~seen
        if not bool(front.any()):  # (the host waits here, once a level)
            break
        seen |= front
        dist = torch.where(front, torch.tensor(level, dtype=torch.int16, device=tiles.device), dist)
    return dist.view(n, tile_w * tile_h), level - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=None, choices=list(CASES))
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64, help="synthetic steps before the measurement, and steps of the timed run")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from procgen2_amd import lib as pglib
    from procgen2_amd.vec_env import ProcgenVecEnv

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
    for case in a.cases or CASES:
        game, mode = CASES[case]
        env = ProcgenVecEnv(game, a.envs, seed_base=1, distribution_mode=mode)
        L, h, st, lay = env.L, env._h, env._stream, env.path_layout
        env.reset()
        for _ in range(a.steps):
            env.step_synthetic(3)
        torch.cuda.synchronize()
        n = a.envs
        source, probe = ("goal", "agent") if lay.has_goal else ("agent", "none")
        dist = torch.empty((n, lay.cells), dtype=torch.int16, device=env.device)
        probe_dist = torch.empty(n, dtype=torch.int32, device=env.device)
        probe_step = torch.empty(n, dtype=torch.uint8, device=env.device)
        cells = torch.empty((n, 2), dtype=torch.int32, device=env.device)
        tiles = torch.empty((n, lay.cells), dtype=torch.uint8, device=env.device)
        torch.cuda.synchronize()

        def paths(with_dist):
            q = pglib.TilePathsStruct(ctypes.sizeof(pglib.TilePathsStruct), 1, pglib.PATH_POINTS[source], None, pglib.PATH_POINTS[probe],
                                      None, dist.data_ptr() if with_dist else None, probe_dist.data_ptr(), probe_step.data_ptr(),
                                      cells.data_ptr())
            pglib.check(L, L.pgv_tile_paths_rows(h, None, n, ctypes.byref(q)), "pgv_tile_paths_rows")

        def tile():
            pglib.check(L, L.pgv_tile_rows(h, None, n, c_void_p(tiles.data_ptr())), "pgv_tile_rows")

        r = {"case": case, "game": game, "mode": env.distribution_mode, "envs": n, "cells": lay.cells, "source": source, "probe": probe,
             "paths_ms": timed(st, lambda: paths(True)), "probe_only_ms": timed(st, lambda: paths(False)), "tiles_ms": timed(st, tile)}
        torch.cuda.synchronize()
        reached = dist >= 0
        r["longest"] = int(dist.max())
        r["reached_share"] = float(reached.float().mean())
        loop_ms = []
        for _ in range(a.loop_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want, levels = dilation_loop(torch, tiles, cells[:, 0], lay.tile_w, lay.tile_h, (0,))
            torch.cuda.synchronize()
            loop_ms.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(want, dist), "%s: the dilation loop and pgv_tile_paths_rows disagree" % case
        assert levels == r["longest"]
        r["loop_ms"] = statistics.median(loop_ms)
        total, _ = env.timed_steps(a.steps, run_seed=3, render_events=False)
        r["step_ms"] = total / a.steps
        for name in ("paths", "probe_only"):
            r[name + "_of_tiles"] = r[name + "_ms"] / r["tiles_ms"]
            r[name + "_of_step"] = r[name + "_ms"] / r["step_ms"]
        r["loop_of_paths"] = r["loop_ms"] / r["paths_ms"]
        print("%-16s %4d cells, longest %3d, %2.0f %% reached  step %6.3f ms | paths %6.3f ms = %5.2f x tile rows (%6.3f), %4.2f of a step | "
              "probe only %6.3f ms = %5.2f x, %4.2f of a step | dilation loop %8.1f ms = %5.0f x (equal)"
              % (case, lay.cells, r["longest"], 100 * r["reached_share"], r["step_ms"], r["paths_ms"], r["paths_of_tiles"], r["tiles_ms"],
                 r["paths_of_step"], r["probe_only_ms"], r["probe_only_of_tiles"], r["probe_only_of_step"], r["loop_ms"], r["loop_of_paths"]),
              flush=True)
        out.append(r)
        env.close()
        del dist, tiles, want, reached
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
