"""The host-only rules of the grouped HDV traffic call (csrc/hdv_grouped_host.hpp), without a GPU: the layout of the
groups' blocks (pdmpc_hdv_grouped_layout_host) against a plain restatement, and tests/hdv_grouped_checks.cpp -- the layout again, the
batching rule of the sweep's stage on a model of a handle, the byte-for-byte content check of a map slot, and the plan of the HDV device
calls (csrc/hdv_call_host.hpp: workspace layout, arguments, stage and scatter, refusals) -- as a program of its own under the sanitizers
(it carries their static runtime; nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

from pdmpc import backend, hdv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HOST_CXX = os.environ.get("HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # (the Makefile's)
SIZES = [(2, 3), (0, 4), (1, 0), (3, 1)]  # (HDVs, CAVs) of every group


def _offsets(sizes):
    ho, co = [0], [0]
    for nh, nc in sizes:
        ho.append(ho[-1] + nh)
        co.append(co[-1] + nc)
    return ho, co


@pytest.mark.parametrize("Hp", [1, 6])
def test_layout_against_a_plain_restatement(Hp):
    ho, co = _offsets(SIZES)
    lay = hdv.grouped_layout(ho, co, Hp)
    C = hdv.MAX_CHAINS
    pairs = 0
    for g in range(len(SIZES) + 1):
        h0 = sum(nh for nh, _ in SIZES[:g])
        assert lay["closest"][g] == h0 + g  # the groups in front have h0 + g offset entries: n_h + 1 each
        assert lay["lists"][g] == h0 * C
        assert lay["set_offset"][g] == h0 * C * Hp + g
        assert lay["sets"][g] == h0 * C * Hp
        assert lay["adjacency"][g] == pairs
        if g < len(SIZES):
            pairs += SIZES[g][0] * SIZES[g][1]
    assert pairs == 9


def test_layout_of_no_group_and_refusals():
    lay = hdv.grouped_layout([0], [0], 6)
    assert all(int(v[0]) == 0 and len(v) == 1 for v in lay.values())
    for ho, co in (([0, 2, 1], [0, 1, 2]), ([0, 1, 2], [0, 2, 1]), ([1, 2, 3], [0, 1, 2])):
        with pytest.raises(backend.BackendError) as e:
            hdv.grouped_layout(ho, co, 6)
        assert e.value.status == -1


def test_the_layout_and_batching_header_names_no_hip():
    """... nor do the plan of the device calls (hdv_call_host.hpp) and the carver it shares with step_prep.cpp"""
    run = subprocess.run(["make", "-s", "-C", CSRC, "host-parts"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    alone = [line.split()[-1] for line in run.stdout.splitlines() if line.startswith("also ok")]
    for header in ("hdv_grouped_host.hpp", "hdv_call_host.hpp", "carver.hpp"):
        code = [line.split("//")[0] for line in open(os.path.join(CSRC, header))]
        assert not [line for line in code if "hip" in line.lower() or "handle.hpp" in line], header
        assert header in alone, run.stdout


@pytest.mark.skipif(shutil.which(HOST_CXX) is None, reason="no host compiler")
def test_hdv_grouped_checks_under_sanitizers(tmp_path):
    """tests/hdv_grouped_checks.cpp: the layout for the group sizes above at Hp 1 and 6 into arrays of exactly n_groups + 1 entries, no
    group, decreasing offsets; the batching rule -- 9 distinct maps give 8 + 1, members of 60, 60 and 60 HDVs 120 + 60, equal maps
    share a slot, a resident map costs no upload and a noted one no check, a moved generation forces the check, two controllers that
    take turns upload once each --; the content check of a slot bit by bit.  The plan of the device calls: the workspace layout for these
    groups with and without a drive pass and for the ungrouped call (alignment, no overlap, inputs in front of in_bytes, the read-back
    from `out` on, sizes against sums written out, two layouts byte by byte); every pointer of the argument records at its region;
    a call staged into a block of exactly in_bytes bytes and scattered from one of exactly total - out bytes into arrays of exactly the
    stated sizes -- whole, one vertex short, a group over its lists, a slot over, the precedence of the three, with the drive pass,
    without the traffic passes, ungrouped --; a table of refused calls against two model slots with code and full text, calls with two
    faults among them.  Under -fsanitize=address,undefined."""
    exe = str(tmp_path / "hdv_grouped_checks")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    build = subprocess.run([HOST_CXX] + flags + ["-o", exe, os.path.join(ROOT, "tests", "hdv_grouped_checks.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.splitlines()[-1] == "hdv grouped checks ok", run.stdout
