#!/usr/bin/env python
"""Rates of pgv_save_envs / pgv_load_envs (per-env state records, include/procgen2_vec.h) beside a plain device copy.

Per game, at --envs envs (65 536): the HIP-event time, on the env's stream, of one save and of one load of EVERY env —
indices NULL, and a random permutation — `--repeats` times after `--warmups`, the median.  Bytes = 2 × count × record
bytes (read + written).  In the same process, on the same device, the same number of bytes moved by one hipMemcpyAsync
device-to-device: boxes differ in what they copy at, so only the ratio taken inside one run means anything.  A save's
time includes what it does first (bossfight, chaser: the random streams come home), a load's what it does after (chaser:
base layers and the due list; the level generator's launch goes to the side stream and is not on this clock).

    python tools/env_records_rate.py [--games coinrun chaser] [--json out.json]
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
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=64, help="synthetic steps before the measurement (streams change buffers, slots fill)")
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

    rows = []
    for game in a.games or GAMES:
        env = ProcgenVecEnv(game, a.envs, seed_base=1)
        L, h, st = env.L, env._h, env._stream
        env.reset()
        for _ in range(a.steps):
            env.step_synthetic(3)
        torch.cuda.synchronize()
        n, rb, tag = a.envs, env.env_record_bytes, env.env_record_tag
        rec = torch.empty((n, rb), dtype=torch.uint8, device=env.device)
        other = torch.empty_like(rec)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(env.device)
        torch.cuda.synchronize()
        moved = 2.0 * n * rb

        def save(idx):
            pglib.check(L, L.pgv_save_envs(h, c_void_p(idx.data_ptr()) if idx is not None else None, n, c_void_p(rec.data_ptr())), "pgv_save_envs")

        def load(idx):
            pglib.check(L, L.pgv_load_envs(h, c_void_p(idx.data_ptr()) if idx is not None else None, n, c_void_p(rec.data_ptr()), tag), "pgv_load_envs")

        def copy():
            assert hip.hipMemcpyAsync(c_void_p(other.data_ptr()), c_void_p(rec.data_ptr()), n * rb, D2D, c_void_p(st.cuda_stream)) == 0

        save(None)
        row = {"game": game, "envs": n, "record_bytes": rb, "copy_ms": timed(st, copy)}
        for name, fn in (("save", lambda: save(None)), ("save_perm", lambda: save(perm)), ("load", lambda: load(None)),
                         ("load_perm", lambda: load(perm))):
            if name.startswith("load"):  # (records that put every env back where it came from)
                save(perm if name == "load_perm" else None)
            row[name + "_ms"] = timed(st, fn)
        for name in ("copy", "save", "save_perm", "load", "load_perm"):
            row[name + "_GBps"] = moved / row[name + "_ms"] / 1e6
            row[name + "_of_copy"] = row["copy_ms"] / row[name + "_ms"]
        rows.append(row)
        print("%-9s record %6d B  copy %5.0f GB/s | save %5.0f GB/s (%.2f of the copy)  permuted %5.0f (%.2f) | load %5.0f (%.2f)  permuted %5.0f (%.2f)"
              % (game, rb, row["copy_GBps"], row["save_GBps"], row["save_of_copy"], row["save_perm_GBps"], row["save_perm_of_copy"],
                 row["load_GBps"], row["load_of_copy"], row["load_perm_GBps"], row["load_perm_of_copy"]), flush=True)
        env.close()
        del rec, other
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
