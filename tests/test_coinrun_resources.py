"""What the compiler gives the step's render and pre-pass kernels (no GPU: hipcc cross-compiles for gfx950).

A kernel's registers and private memory are those of its largest path, paid by every wavefront.  coinrun's render_kernel
ran every frame under its cap of 96 registers with 127 of them spilled and 200 B of scratch a lane, nearly all of it for the
redo of an early-ended step in its complete path; the pre-pass of four games kept 40 B of scratch for a per-lane choice
between two cameras taken by reference.  These are the figures that must not come back (the compiler's own remarks,
-Rpass-analysis=kernel-resource-usage, of variant 0 built with the product's flags; figures only, no instructions):

  * setup_kernel of coinrun, climber, caveflyer and jumper: scratch 0, nothing spilled;
  * coinrun render_kernel: at least 5 wavefronts a SIMD, at most 17 920 B of LDS (nine envs a CU).  Its scratch and spills
    are NOT asserted: the complete path still sits in this kernel, which leaves 16 B and 3 registers of the 200 B and 127
    (docs/OPTLOG.md, "The step's private memory", says what was measured when it was taken out);
  * coinrun redo_kernel: nothing spilled, at least 5 wavefronts a SIMD.

Also here, because it needs no GPU either: the oracle's own count of the deaths in test_coinrun_lean_gpu.py's protocol.
"""
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

from procgen2_amd import build as pgbuild

KEYS = {"VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy", "VGPRs Spill": "spill",
        "LDS Size [bytes/block]": "lds"}
GAMES = ("coinrun", "climber", "caveflyer", "jumper")


def kernel_figures(game):
    """{kernel name: {vgpr, scratch, occupancy, spill, lds}} of the device code of variant 0 of the game's source."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [pgbuild.hipcc()] + [f for f in pgbuild.COMMON if not f.startswith("-W")] + \
              ["-DPG_VARIANT=0", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(pgbuild.CSRC, game + ".hip"), "-o", os.path.join(tmp, game + ".o")]
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    figures, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            mangled = m.group(1)
            k = re.search(r"\d+([a-z_]+_kernel)", mangled)
            name = k.group(1) if k else mangled
            figures[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass-analysis", line)
        if m and name and m.group(1) in KEYS:
            figures[name][KEYS[m.group(1)]] = int(m.group(2))
    return figures


@pytest.fixture(scope="module")
def figures():
    with ThreadPoolExecutor(len(GAMES)) as pool:
        return dict(zip(GAMES, pool.map(kernel_figures, GAMES)))


def test_coinrun_render_kernel_keeps_its_budget(figures):
    f = figures["coinrun"]["render_kernel"]
    print("coinrun render_kernel", f)
    assert f["occupancy"] >= 5, f
    assert f["lds"] <= 17920, f
    r = figures["coinrun"]["redo_kernel"]
    print("coinrun redo_kernel", r)
    assert r["scratch"] == 0 and r["spill"] == 0 and r["occupancy"] >= 5, r


@pytest.mark.parametrize("game", GAMES)
def test_setup_kernel_keeps_nothing_in_private_memory(figures, game):
    f = figures[game]["setup_kernel"]
    print(game, "setup_kernel", f)
    assert f["scratch"] == 0 and f["spill"] == 0, f


def test_the_early_end_protocol_holds_its_deaths_on_the_oracle():
    from coinrun_lean_util import death_steps, early_deaths
    died = death_steps()
    assert sum(len(d) for d in died) >= 16
    early = early_deaths(died)
    assert sum(len(e) for e in early) >= 12  # on a sub-step before the last: the steps that owe their entities a redo
    assert sum(1 for e in early if len(e)) >= 8
