"""The benchmark's own workloads against the oracle: bench.py run as the headline is run (default --envs, --settle,
--warmup and --steps), with --dump-outputs, and every dumped observation row replayed on the CPU oracle
(tests/bench_replay.py) — the steady state around step 1 088 that the published figures are measured on.  Every game in
its default mode, the mixed workload and every non-default distribution mode (bench.py --mode).

One bench.py child at a time.  A child that ends by a signal or by its timeout marks the module, and the workloads
after it skip without starting another GPU process."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from bench_replay import check_dump, mixed_blocks
from test_modes import NON_DEFAULT

from procgen2_amd import lib as pglib
from procgen2_amd.vec_env import GAMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_NAMES = {v: k for k, v in pglib.MODES.items()}
WORKLOADS = [(g, None) for g in GAMES] + [("mixed", None)] + [(g, MODE_NAMES[m]) for g, m in NON_DEFAULT]
CHILD_TIMEOUT_S = 120  # one bench.py run at its defaults (make, 1 088 steps of 65 536 envs, the dump) takes seconds
_stopped = []  # why no further child may start: one ended by a signal or by its timeout


@pytest.mark.parametrize("workload,mode", WORKLOADS, ids=["%s-%s" % (w, m or "default") for w, m in WORKLOADS])
def test_bench_outputs_match_the_oracle(workload, mode, tmp_path):
    if _stopped:
        pytest.skip("no GPU process started after " + _stopped[0])
    out = os.path.join(tmp_path, "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", out]
    cmd += ["--workload", "mixed"] if workload == "mixed" else ["--game", workload]
    cmd += ["--mode", mode] if mode else []
    what = "bench.py " + " ".join(cmd[2:])
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _stopped.append("%s ran past its %d s timeout" % (what, CHILD_TIMEOUT_S))
        pytest.fail(_stopped[-1])
    if r.returncode < 0:
        _stopped.append("%s ended by signal %d" % (what, -r.returncode))
        pytest.fail(_stopped[-1] + "\n" + r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    envs = line["config"]["envs_per_gpu"]
    steps = line["settle_steps"] + max(1, line["warmup"]) + line["steps"]
    assert line["n_gpus"] == 1 and steps > 1000, line
    if workload == "mixed":  # the checker's layout is the one bench.py reports
        split = re.search(r"split (\[[0-9, ]+\])", line["config"]["workload"]).group(1)
        assert json.loads(split) == [c for _, _, c in mixed_blocks(envs)], line["config"]["workload"]
    else:
        assert line["config"]["game"] == workload and line["config"]["distribution_mode"] == (mode or "default")
    rows, ended = check_dump(out, workload, envs, steps, mode=mode)
    assert ended > 0, "none of the %d rows ended an episode in %d steps: the auto-reset path went unchecked" % (rows, steps)
    print("%s: %d rows equal the oracle after %d steps, %d of them through an episode end" % (what, rows, steps, ended))
    shutil.rmtree(out)
