"""The HDV driver model without a GPU (include/pdmpc_hdv.h: "the driver model"; csrc/hdv_drive_host.hpp): the numpy twin
(pdmpc.hdv.drive) and the host twin (pdmpc_hdv_drive_host) bit for bit on the members of tests/hdv_drive_cases.py, the route checks,
the placement, the refusals, and tests/hdv_drive_checks.cpp -- the same header functions as a program of its own under the sanitizers
(it carries their static runtime; nothing is preloaded)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import hdv_drive_cases as D
from pdmpc import backend, hdv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HOST_CXX = os.environ.get("HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")  # (the Makefile's)
MEMBERS = D.lab_members() + D.hand_members()


@pytest.mark.parametrize("m", MEMBERS, ids=[m.name for m in MEMBERS])
def test_twins_agree_bit_for_bit(m):
    py, host = m.python(), m.host()
    D.assert_same(py, host, m.name)
    D.check_expectations(m, host)
    # ... and the step after it (from the end of an open route: it stays there)
    again = m.after(host, m.name + ", the next step")
    D.assert_same(again.python(), again.host(), again.name)
    if "ends" in m.expect:
        r = again.host()
        assert r["states"] == host["states"] and r["speed"] == [0.0]


def test_a_cav_at_exactly_gap_min_and_one_ulp_either_side():
    m = next(m for m in MEMBERS if m.name.startswith("a CAV 0.6 m ahead"))
    gap = m.host()["gap"][0]
    assert 0.6 - 0.125 - 1e-9 < gap < 0.6 + 1e-9  # (a foot clamped to the end of the segment before the CAV's counts: up to `lateral` less)
    for gap_min, stopped in ((gap, True), (np.nextafter(gap, math.inf), True), (np.nextafter(gap, -math.inf), False)):
        v = D.Member("gap_min %r" % gap_min, m.hmap, [], [], (2.0, float(gap_min), 1.0, 0.125), states=m.states)
        v.routes, v.tiles, v.v_des, v.cav_x, v.cav_y, v.cav_tile = m.routes, m.tiles, m.v_des, m.cav_x, m.cav_y, m.cav_tile
        py, host = v.python(), v.host()
        D.assert_same(py, host, v.name)
        assert host["gap"][0] == gap
        assert (host["speed"][0] == 0.0) == stopped and (host["states"][0] == m.states[0]) == stopped, (v.name, host)
        if not stopped:
            assert 0.0 < host["speed"][0] < 1e-15


def test_the_simultaneous_update_reads_the_old_poses():
    """Two HDVs 0.4 m apart: the follower's gap is the distance to where the leader stood before the step, whichever of them comes
    first in the call."""
    L, R = D.lab(), D.loop_route()
    a = D.Member("follower first", L, [(R, 0.7, D.ZERO, 0.5), (R, 1.1, D.ZERO, 0.5)], []).host()
    b = D.Member("leader first", L, [(R, 1.1, D.ZERO, 0.5), (R, 0.7, D.ZERO, 0.5)], []).host()
    assert D.bits(a["gap"][0]) == D.bits(b["gap"][1]) and a["gap"][1] == b["gap"][0] == math.inf
    assert 0.4 - 0.125 - 1e-9 < a["gap"][0] < 0.4 + 1e-9
    assert a["states"][0] == b["states"][1] and a["states"][1] == b["states"][0]


def test_every_loop_of_the_lab_map_is_a_route():
    from pdmpc.road_network import _PATHS, get_reference_lanelets_loop

    routes = [hdv.route_from_loop(p) for p in sorted(_PATHS)]
    assert max(len(ids) for ids, _ in routes) <= hdv.ROUTE_MAX
    assert all(ids == list(get_reference_lanelets_loop(p)) and closed for (ids, closed), p in zip(routes, sorted(_PATHS)))
    for h, (ids, closed) in enumerate(routes):
        hdv.check_route(D.lab(), ids, closed, h)
    hdv.route_check_native(D.lab(), routes)
    for route in routes[:4]:  # the joints of a loop are ordinary segments: the lanelets miss their successors by up to 3e-5 m
        joints = [hdv._route_segment(D.lab(), route[0], True, r, hdv._route_segments(D.lab(), route[0], True, r) - 1)[4] for r in range(len(route[0]))]
        assert max(joints) < 1e-4


def _refused(routes, text):
    with pytest.raises(backend.BackendError) as e:
        hdv.route_check_native(D.lab(), routes)
    assert e.value.status == -1 and text in str(e.value), str(e.value)
    for h, (ids, closed) in enumerate(routes):
        try:
            hdv.check_route(D.lab(), ids, closed, h)
        except ValueError as v:
            assert text in str(v), str(v)
            return
    raise AssertionError("the Python twin accepts %r" % (routes,))


def test_route_refusals_name_the_hdv_and_the_position():
    ids, _ = D.loop_route()
    good = (ids, True)
    _refused([good, (ids[:2] + [ids[3]], False)], "HDV 1: route position 2: lanelet %d is no successor of lanelet %d" % (ids[3], ids[1]))
    _refused([(ids[:5], True)], "HDV 0: route position 0: lanelet %d is no successor of lanelet %d" % (ids[0], ids[4]))
    _refused([good, good, (ids[:3] + [105], False)], "HDV 2: route position 3: lanelet id 105 out of range")
    _refused([(ids[:1] + [0], False)], "HDV 0: route position 1: lanelet id 0 out of range")
    _refused([((ids * 8)[:hdv.ROUTE_MAX + 1], False)], "HDV 0: a route of %d lanelets" % (hdv.ROUTE_MAX + 1))
    hdv.route_check_native(D.lab(), [((ids * 8)[:hdv.ROUTE_MAX], False)])  # (round the loop again and again: at the limit)
    _refused([([], False)], "HDV 0: a route of 0 lanelets")
    hdv.route_check_native(D.lab(), [(ids[:5], False), good])


def test_placement_is_the_walk_of_the_step():
    L, R = D.lab(), D.loop_route()
    d = [0.0, 0.7, 2.9, D.route_length(L, R) - 1e-3, D.route_length(L, R) + 0.7]
    states, x, y, c, s = hdv.place_native(L, [R] * len(d), d, [D.ZERO] * len(d))
    for q, dist in enumerate(d):
        st = hdv.place(L, R[0], R[1], dist)
        assert st[:2] == states[q][:2] and D.bits(st[2]) == D.bits(states[q][2])
        assert [D.bits(v) for v in hdv.state_pose(L, R[0], R[1], st)] == [D.bits(v) for v in (x[q], y[q], c[q], s[q])]
        assert abs(math.hypot(c[q], s[q]) - 1.0) < 1e-15
    # a step of 0.7 m from the start is the placement at 0.7 m; once round the loop is the same place to rounding
    one = hdv.drive_native(L, [R], [states[0]], [D.ZERO], [0.7], [], [], [], hdv.DRIVE_DEFAULTS, 1.0)
    assert one["states"][0] == states[1]
    assert abs(x[4] - x[1]) < 1e-9 and abs(y[4] - y[1]) < 1e-9


def test_refusals_of_a_step_and_of_a_placement():
    L, R = D.lab(), D.loop_route()
    open3 = (R[0][:3], False)
    st = [hdv.place(L, R[0], R[1], 0.7)]

    def refused(call, text):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.status == -1 and text in str(e.value), str(e.value)

    refused(lambda: hdv.drive_native(L, [R], st, [D.ZERO], [0.5], [], [], [], (2.0, 0.3, 0.1, 0.125), 0.2), "headway < dt")
    hdv.drive_native(L, [R], st, [D.ZERO], [0.5], [], [], [], (2.0, 0.3, 0.2, 0.125), 0.2)  # headway == dt
    refused(lambda: hdv.drive_native(L, [R], st, [D.ZERO], [0.5], [], [], [], (2.0, 0.0, 1.0, 0.125), 0.2), "positive")
    refused(lambda: hdv.drive_native(L, [R], st, [D.ZERO], [0.5], [], [], [], (2.0, 0.3, 1.0, math.nan), 0.2), "positive")
    refused(lambda: hdv.drive_native(L, [R], st, [D.ZERO], [-0.5], [], [], []), "desired speed")
    refused(lambda: hdv.drive_native(L, [R], [(len(R[0]), 0, 0.0)], [D.ZERO], [0.5], [], [], []), "not on its route")
    refused(lambda: hdv.drive_native(L, [R], [(0, 10000, 0.0)], [D.ZERO], [0.5], [], [], []), "not on its route")
    refused(lambda: hdv.drive_native(L, [open3], [(2, hdv._route_segments(L, open3[0], False, 2), 0.0)], [D.ZERO], [0.5], [], [], []), "not on its route")
    refused(lambda: hdv.drive_native(L, [R], [(0, 0, -1.0)], [D.ZERO], [0.5], [], [], []), "not on its route")
    refused(lambda: hdv.place_native(L, [open3], [D.route_length(L, open3) + 0.1], [D.ZERO]), "beyond the end of an open route")
    refused(lambda: hdv.place_native(L, [open3], [-0.1], [D.ZERO]), "negative")
    with pytest.raises(ValueError):
        hdv.place(L, open3[0], False, D.route_length(L, open3) + 0.1)
    with pytest.raises(ValueError):
        hdv.check_drive((2.0, 0.3, 0.1, 0.125), 0.2, [0.5])


def test_the_driver_header_names_no_hip():
    code = [line.split("//")[0] for line in open(os.path.join(CSRC, "hdv_drive_host.hpp"))]
    assert not [line for line in code if "hip" in line.lower() or "handle.hpp" in line]
    run = subprocess.run(["make", "-s", "-C", CSRC, "host-parts"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "hdv_drive_host.hpp" in [line.split()[-1] for line in run.stdout.splitlines() if line.startswith("also ok")], run.stdout


@pytest.mark.skipif(shutil.which(HOST_CXX) is None, reason="no host compiler")
def test_hdv_drive_checks_under_sanitizers(tmp_path):
    """tests/hdv_drive_checks.cpp: routes, placement, window builder and the host step on hand-made maps -- the segment of length 0, the
    window cap, wrap-around, the end of an open route, another tile, the simultaneous update, the refusals -- under
    -fsanitize=address,undefined."""
    exe = str(tmp_path / "hdv_drive_checks")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    build = subprocess.run([HOST_CXX] + flags + ["-o", exe, os.path.join(ROOT, "tests", "hdv_drive_checks.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.splitlines()[-1] == "hdv drive checks ok", run.stdout
