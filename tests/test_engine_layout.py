"""The engine's own device memory, without a GPU: the level plan's arrays behind a game's state and the episode block's
buffers as their listings (procgen2_amd/csrc/pg_carve.h list_plan, pg_episodes.h list_episodes) lay them out, compiled for
the CPU and held to literal offsets and sizes (tests/cpp/test_engine_layout.cpp).  The plan's offsets are a snapshot's
format: tests/test_snapshot.py finds the arrays there in a snapshot the engine wrote."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "procgen2_amd", "csrc")


def test_plan_and_episode_block_on_the_host(tmp_path):
    exe = str(tmp_path / "test_engine_layout")
    subprocess.run(["g++", "-std=gnu++17", "-O2", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "test_engine_layout.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for section in ("OK level plan", "OK episode block", "ALL OK"):
        assert section in out.stdout, section


def test_the_listing_header_needs_no_hip(tmp_path):
    """pg_carve.h alone, with no include path but the compiler's own: nothing of ROCm, and of the standard library only
    <vector>, <cstdint> and <cstddef>."""
    with open(os.path.join(CSRC, "pg_carve.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstdint>", "<vector>"]
    src = tmp_path / "only_carve.cpp"
    src.write_text('#include "%s"\nint main() { return pg::Carve::size(pg::list_plan, 3) == 96 ? 0 : 1; }\n' % os.path.join(CSRC, "pg_carve.h"))
    exe = str(tmp_path / "only_carve")
    subprocess.run(["g++", "-std=gnu++17", "-Wall", "-Werror", str(src), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
