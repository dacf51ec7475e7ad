"""The HDV stage of the native step controller on narrow state (csrc/step_hdv.hpp), without a GPU:
tests/step_hdv_checks.cpp takes members through the batch path -- gather, ONE grouped call, scatter -- and copies of them through the
solo path, as a program of its own under the sanitizers (it carries their static runtime; nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HOST_CXX = os.environ.get("HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # (the Makefile's)


@pytest.mark.skipif(shutil.which(HOST_CXX) is None, reason="no host compiler")
def test_batch_path_equals_solo_path_under_sanitizers(tmp_path):
    """In the device call's place stands a model: the host twins (pdmpc_hdv_drive_host, pdmpc_hdv_traffic_host) group by group into the
    blocks of pdmpc_hdv_grouped_layout_host, with the capacity protocol of the grouped call, every index checked against its array.
    The cases: one member (1 HDV, 1 CAV, Hp 1); three members of (HDVs, CAVs) = (2, 3), (1, 1), (3, 2) on two maps, measured, at Hp 1
    and 3; the same with drivers on members 0 and 2 -- their first built step (nobody moves: the traffic call), the mixed call (routes
    flat over member 1, drives = 1, 0, 1), once more -- and on all three; a member on its first built step after its drivers were set
    beside one on its second; the capacity retry (room for 8 vertices: two calls, the second with the total and a quarter) for both
    calls.  After scatter every member equals its solo copy byte for byte: rows, lists, offsets, flags, adjacency, vertices, the CAVs'
    sets, poses, and for drivers state, speed and gap.  Compiled with csrc/hdv.cpp and the bounding it calls (csrc/reachable_sets.cpp)
    under -fsanitize=address,undefined."""
    exe = str(tmp_path / "step_hdv_checks")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    sources = [os.path.join(ROOT, "tests", "step_hdv_checks.cpp"), os.path.join(CSRC, "hdv.cpp"), os.path.join(CSRC, "reachable_sets.cpp")]
    build = subprocess.run([HOST_CXX] + flags + ["-o", exe] + sources, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[-1] == "step hdv checks ok", run.stdout
    assert len(lines) == 12, run.stdout  # eleven cases, none left out
