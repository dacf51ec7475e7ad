"""The host-only parts of csrc (launch_plan.hpp, mpa_reach.hpp, choice_host.hpp, reference_tree.hpp): each compiles alone with the host
compiler, and tests/host_only_checks.cpp checks the three behind api.cpp's reach, choice and tree read-back entry points against
expectations that do not share their rules (no GPU needed; the program is its own process and carries the sanitizers' static runtime)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HOST_CXX = os.environ.get("HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # (the Makefile's)
PARTS = ("launch_plan.hpp", "mpa_reach.hpp", "choice_host.hpp", "reference_tree.hpp")


def test_host_only_parts_compile_alone():
    """`make host-parts` reports every host-only part: no HIP header, no handle (-Wall -Werror, syntax only)."""
    run = subprocess.run(["make", "-s", "-C", CSRC, "host-parts"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    also_ok = [line.split()[-1] for line in run.stdout.splitlines() if line.startswith("also ok")]
    for part in PARTS:
        assert part in also_ok, run.stdout


def test_host_only_parts_name_no_hip():
    """Outside comments, none of the three new headers names HIP, the handle's header or a handle."""
    for part in PARTS[1:]:
        code = [line.split("//")[0] for line in open(os.path.join(CSRC, part))]
        assert not [line for line in code if "hip" in line.lower() or "handle" in line], part


@pytest.mark.skipif(shutil.which(HOST_CXX) is None, reason="no host compiler")
def test_host_only_checks_under_sanitizers(tmp_path):
    """The reference's tree out of 300 random arenas against a literal best-first search (and malformed arenas refused, not indexed), the
    reach rectangles of 18 small automata against every trim path (agreement to 1e-12 absolute; the largest difference the program
    prints is 8.9e-16), both reach-list builders on a two-step soup, every refusal of check_choice and one choice written out, the words its lists are staged in (identity, a permutation, the empty
    choice) and the delivery of a hand-built read-back block (either optional array absent; each non-result counter refused), the scratch
    a sampled bank needs (sampled_need: no scratch at the default, trees in LDS and in HBM, ensembles of 2 and 16 at both, against counts
    written out) and the seeds pending for a pack (set, take, a second take, set twice): under
    -fsanitize=address,undefined, which turn any out-of-bounds read into a failure."""
    exe = str(tmp_path / "host_only_checks")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    build = subprocess.run([HOST_CXX] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_only_checks.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.splitlines()[-1] == "host-only checks ok", run.stdout
