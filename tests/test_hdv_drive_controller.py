"""HDVs that move themselves in the closed loop, without a GPU (pdmpc_controller_set_hdv_drivers / _set_hdv_recording, the drive step in
the traffic stage; PrioritizedSequentialController.set_hdv_drivers / set_hdv_recording; DESIGN.md §3.24 "Drivers"): a driven loop against
a twin that is hand-fed the numpy twin's poses, the native controller against the Python one, a recording against the hand-fed loop,
the rejections, and the safety property of the driver model behind planned CAVs.  The native controller has no handle here: its steps
are build_step, the oracle as the planner, apply -- what pdmpc_controller_run does with a handle (tests/test_gpu_hdv_drive_controller.py)."""
import math

import numpy as np
import pytest

import hdv_cases as H
import hdv_drive_cases as D
from oracle import oracle
from pdmpc import backend, hdv
from pdmpc.mpa import get_mpa
from test_hdv_controller import _oracle_planner, _problem_bytes, _same_info, _twins
from test_native_controller import assert_same_problem

ROUTE = hdv.route_from_loop(D.LOOP)
STARTS, V_DES = [0.7, 2.9], [0.5, 0.35]  # where tests/hdv_cases.py::hdv_poses_at starts its two HDVs
PARAMS = (2.0, 0.3, 1.0, 0.125)


def _driven(options, handle=None):
    py, nat = _twins(options, handle)
    for c in (py, nat):
        c.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS)
    return py, nat


def _native_step(nat, options, mpa):
    nat.build_step()
    q = nat.problem()
    recs, _ = oracle.plan_step(options, mpa, q)
    nat.apply(recs)
    return q


def _same_state(a, b, what):
    for key in ("x", "y", "yaw"):
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)


def _same_driver_state(a, b, what):
    assert a["states"][0][:2] == b["states"][0][:2] and [s[:2] for s in a["states"]] == [s[:2] for s in b["states"]], what
    for key in ("x", "y", "yaw", "speed", "gap"):
        assert [D.bits(v) for v in a[key]] == [D.bits(v) for v in b[key]], (what, key, a[key], b[key])
    assert [D.bits(s[2]) for s in a["states"]] == [D.bits(s[2]) for s in b["states"]], what


def test_a_driven_loop_equals_a_loop_that_is_hand_fed_the_numpy_twins_poses():
    """6 steps, 4 CAVs, 2 HDVs with drivers, the oracle as the planner.  The second controller has no drivers: before each of its steps the
    test moves the HDVs with hdv.drive against that controller's own CAV positions and hands the poses over as directions
    (set_hdv_poses: cos and sin as the driver step gives them; a yaw through libm would not give the same bits).  Problems, traffic
    info and state are the same byte for byte -- and on the parent commit nothing moves the first controller's HDVs."""
    options = H.loop_options(2, max_nodes=1 << 16)
    mpa = get_mpa(options)
    py, driven = _driven(options)
    _, fed = _twins(options)
    hmap = py.hdvs["map"]  # the scenario's own lanelets: what both controllers drive on
    states = [hdv.place(hmap, ROUTE[0], ROUTE[1], d) for d in STARTS]
    poses = [hdv.state_pose(hmap, ROUTE[0], ROUTE[1], s) for s in states]
    moved = 0
    for step in range(1, 7):
        if step > 1:
            st = fed.state()
            r = hdv.drive(hmap, [ROUTE, ROUTE], states, [D.ZERO] * 2, V_DES, list(st["x"]), list(st["y"]), [D.ZERO] * 4, PARAMS, options.dt_seconds)
            moved += sum(a != b for a, b in zip(states, r["states"]))
            states, poses = r["states"], list(zip(r["x"], r["y"], r["cos_yaw"], r["sin_yaw"]))
        fed.set_hdv_poses(*[[p[k] for p in poses] for k in range(4)])
        p, q = _native_step(driven, options, mpa), _native_step(fed, options, mpa)
        assert_same_problem(p, q, "step %d" % step)
        assert _problem_bytes(p, 6) == _problem_bytes(q, 6), step
        _same_info(driven.hdv_info(), fed.hdv_info(), "step %d" % step)
        _same_state(driven.state(), fed.state(), step)
        ds = driven.hdv_driver_state()
        assert ds["states"] == states and [D.bits(v) for v in ds["x"]] == [D.bits(p[0]) for p in poses]
    assert moved >= 10 and sum(len(it.hdv_reachable_sets) for it in p["iters"]) > 0
    driven.close()
    fed.close()


def test_the_python_controller_and_the_native_one_drive_the_same():
    options = H.loop_options(2, max_nodes=1 << 16)
    mpa = get_mpa(options)
    py, nat = _driven(options)
    for step in range(1, 7):
        nat.build_step()
        q = nat.problem()
        info = nat.hdv_info()

        def plan_step(prob):
            assert_same_problem(prob, q, "step %d" % step)
            assert _problem_bytes(prob, 6)[3] == _problem_bytes(q, 6)[3], step
            recs, _ = oracle.plan_step(options, mpa, prob)
            nat.apply(recs)
            return [_info(recs[i], options.Hp) for i in range(len(recs))]

        py.step(plan_step=plan_step)
        _same_info(py.hdv_info, info, "step %d" % step)
        _same_driver_state(py.hdv_driver_state(), nat.hdv_driver_state(), "step %d" % step)
    ds = nat.hdv_driver_state()
    assert ds["states"] != [hdv.place(py.hdvs["map"], ROUTE[0], ROUTE[1], d) for d in STARTS] and max(ds["speed"]) > 0.0
    # ... and with the host twin as the Python controller's driver step
    py2, nat2 = _twins(options)
    py2.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS, drive=lambda *a: hdv.drive_native(py2.hdvs["map"], *a))
    plan = _oracle_planner(options)
    for step in range(3):
        py2.step(plan_step=plan)
    py3, _ = _driven(options)
    for step in range(3):
        py3.step(plan_step=plan)
    _same_driver_state(py2.hdv_driver_state(), py3.hdv_driver_state(), "host twin as the driver step")
    nat.close()
    nat2.close()


def _info(rec, Hp):
    from pdmpc.iteration_data import info_from_record

    return info_from_record(rec, Hp)


def test_a_recording_replays_the_hand_fed_loop():
    """rows 1 .. 4 of hdv_poses_at recorded; 6 steps: steps 5 and 6 take the last row.  Native and Python controller against controllers
    that are fed set_hdv_measurements step by step."""
    options = H.loop_options(2, max_nodes=1 << 16)
    mpa = get_mpa(options)
    rows = [H.hdv_poses_at(s) for s in range(1, 5)]
    rec = [[r[k] for r in rows] for k in range(3)]
    py, nat = _twins(options)
    py_fed, fed = _twins(options)
    nat.set_hdv_recording(*rec)
    py.set_hdv_recording(*rec)
    plan = _oracle_planner(options)
    for step in range(1, 7):
        pose = H.hdv_poses_at(min(step, 4))
        fed.set_hdv_measurements(*pose)
        py_fed.set_hdv_measurements(*pose)
        p, q = _native_step(nat, options, mpa), _native_step(fed, options, mpa)
        assert_same_problem(p, q, "step %d" % step)
        assert _problem_bytes(p, 6) == _problem_bytes(q, 6), step
        _same_info(nat.hdv_info(), fed.hdv_info(), "step %d" % step)
        py.step(plan_step=plan)
        py_fed.step(plan_step=plan)
        H.assert_same(py.hdv_info, py_fed.hdv_info, step)
        _same_info(py.hdv_info, nat.hdv_info(), "python against native, step %d" % step)
    nat.close()
    fed.close()


def test_rejections():
    options = H.loop_options(2, max_nodes=1 << 16)
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import commonroad_scenario

    bare = NativeController(options, commonroad_scenario(options, seed=1), get_mpa(options), None, coupling="distance")

    def refused(call, text):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.status == -1 and text in str(e.value), str(e.value)

    refused(lambda: bare.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS), "before pdmpc_controller_set_hdvs")
    refused(lambda: bare.set_hdv_recording([[0.0, 0.0]], [[0.0, 0.0]], [[0.0, 0.0]]), "before pdmpc_controller_set_hdvs")
    bare.close()
    py, nat = _twins(options)
    open3 = (ROUTE[0][:3], False)
    refused(lambda: nat.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, (2.0, 0.3, 0.1, 0.125)), "headway < dt")
    refused(lambda: nat.set_hdv_drivers([ROUTE, open3], [0.7, D.route_length(py.hdvs["map"], open3) + 0.5], V_DES, PARAMS), "HDV 1: a start distance at or beyond the end of an open route")
    refused(lambda: nat.set_hdv_drivers([ROUTE, ([1, 3, 10], False)], STARTS, V_DES, PARAMS), "HDV 1: route position 2: lanelet 10 is no successor of lanelet 3")
    with pytest.raises(backend.BackendError):  # (nothing was set by the refused calls)
        nat.build_step()
    nat.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS)
    refused(lambda: nat.set_hdv_measurements(*H.hdv_poses_at(1)), "the HDVs move themselves")
    refused(lambda: nat.set_hdv_poses([0.0] * 2, [0.0] * 2, [1.0] * 2, [0.0] * 2), "the HDVs move themselves")
    refused(lambda: nat.set_hdv_recording(*[[v] for v in H.hdv_poses_at(1)]), "have drivers")
    nat.build_step()  # (no measurement is needed: the placement is the first)
    assert nat.hdv_driver_state()["speed"] == [0.0, 0.0] and nat.hdv_driver_state()["gap"] == [math.inf] * 2
    nat.close()
    _, rec = _twins(options)
    rec.set_hdv_recording(*[[v] for v in H.hdv_poses_at(1)])
    refused(lambda: rec.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS), "replay a recording")
    refused(lambda: rec.set_hdv_measurements(*H.hdv_poses_at(1)), "the HDVs move themselves")
    refused(lambda: rec.hdv_driver_state(), "before pdmpc_controller_set_hdv_drivers")
    rec.close()
    # the Python twin
    with pytest.raises(ValueError):
        H.loop_controller(H.loop_options(0)).set_hdv_drivers([], [], [])
    with pytest.raises(ValueError):
        py.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, (2.0, 0.3, 0.1, 0.125))
    with pytest.raises(ValueError):
        py.set_hdv_drivers([ROUTE, open3], [0.7, 100.0], V_DES, PARAMS)
    py.set_hdv_drivers([ROUTE, ROUTE], STARTS, V_DES, PARAMS)
    with pytest.raises(ValueError):
        py.set_hdv_measurements(*H.hdv_poses_at(1))
    with pytest.raises(ValueError):
        py.set_hdv_recording(*[[v] for v in H.hdv_poses_at(1)])


def _arc(hmap, route, x, y):
    """(distance to the route, metres along it) of the nearest point of the route's polyline"""
    ids, closed = route
    best, run = (math.inf, 0.0), 0.0
    for r in range(len(ids)):
        for j in range(hdv._route_segments(hmap, ids, closed, r)):
            ax, ay, dx, dy, length = hdv._route_segment(hmap, ids, closed, r, j)
            if length == 0.0:
                continue
            t = min(1.0, max(0.0, ((x - ax) * dx + (y - ay) * dy) / (length * length)))
            d = math.hypot(x - ax - t * dx, y - ay - t * dy)
            if d < best[0]:
                best = (d, run + t * length)
            run += length
    return best


def test_an_hdv_never_closes_below_gap_min_behind_planned_cavs():
    """30 steps, 4 CAVs planned by the oracle on the loop and 2 HDVs behind them on the same loop -- one 1.06 m behind CAV 1, the other
    0.6 m behind the first --, faster than the CAVs (1.5 m/s) and with headway = dt, the least allowed.  After every move the distance
    ahead along the route from each HDV to the nearest vehicle on its route (the driver model's own measure, from the new state: the
    CAVs where this step measured them, the other HDV where it now stands) is at least gap_min - 1e-9.  The property needs leaders
    that do not reverse: every CAV on the route is checked to move forward along it from step to step."""
    options = H.loop_options(2, max_nodes=1 << 16)
    ctl = H.loop_controller(options)
    hmap = ctl.hdvs["map"]
    params, total = (2.0, 0.3, options.dt_seconds, 0.125), D.route_length(hmap, ROUTE)
    ctl.set_hdv_drivers([ROUTE, ROUTE], [0.8, 1.4], [1.5, 1.5], params)
    plan = _oracle_planner(options)
    before, slowed, closest = None, 0, math.inf
    for step in range(1, 31):
        ctl.step(plan_step=plan)  # (the step's build moved the HDVs against the CAVs as measured at its start: last_problem's x0)
        by_vehicle = dict(zip(ctl.last_problem["order"], ctl.last_problem["iters"]))
        cavs = [(float(by_vehicle[v].x0[0]), float(by_vehicle[v].x0[1])) for v in range(4)]
        arcs = [_arc(hmap, ROUTE, x, y) for x, y in cavs]
        assert all(d <= params[3] for d, _ in arcs)  # (all four drive on the HDVs' route)
        if before is not None:
            for (_, a0), (_, a1) in zip(before, arcs):
                assert (a1 - a0 + total / 2) % total - total / 2 >= -1e-9, (step, a0, a1)  # no CAV reverses
        before = arcs
        ds = ctl.hdv_driver_state()
        for q in range(2):
            W = hdv.build_window(hmap, ROUTE[0], ROUTE[1], ds["states"][q], params[0])
            others = cavs + [(ds["x"][1 - q], ds["y"][1 - q])]
            ahead = min(hdv.gap_item(W, w, ds["states"][q][2], x, y, params[3]) for x, y in others for w in range(len(W)))
            assert ahead >= params[1] - 1e-9, (step, q, ahead)
            closest = min(closest, ahead)
            slowed += ds["speed"][q] < 1.5
    print(slowed, closest)
    assert slowed > 10 and closest < params[1] + 0.05  # (they did catch up, and were held at gap_min)
