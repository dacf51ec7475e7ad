"""Centralized control in the native step controller and in sweeps (pdmpc_controller_centralized_*, pdmpc_sweep_centralized_*,
csrc/step_centralized.hpp) against the Python twin pdmpc.centralized.CentralizedController, without a handle (no GPU): the planner is
tests/joint_reference.py.  The GPU side is tests/test_gpu_centralized.py."""
import ctypes as C

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.backend import BackendError
from pdmpc.centralized import CentralizedController, CentralizedExhaustedError, centralized_mpa, centralized_options
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.iteration_data import info_from_record
from pdmpc.native_controller import NativeController, NativeSweep

import centralized_cases as cc
import joint_reference as jr

ERR_INVALID, ERR_CAPACITY = -1, -4


def road_case():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = centralized_options(Config(scenario_type=ScenarioType.commonroad, amount=2, Hp=5, mpa_type=MpaType.single_speed, max_vehicles=8))
    sc = commonroad_scenario(options, seed=1)
    return options, sc, boundary_provider(sc)


def circle_case(N, Hp):
    options = cc.circle_options(N, Hp)
    # (two rectangles far from the circle: the obstacle set is not empty, and nobody meets it)
    return options, cc.rotated_circle(options, 0.0, [cc.rectangle(9.0, 9.0), cc.rectangle(-5.0, 8.0, 0.3, 0.3)]), None


@pytest.mark.parametrize("case,steps", [("circle2", 6), ("circle3", 4), ("road2", 4)])
def test_native_problem_and_state_equal_the_twin(case, steps):
    """Every step's joint problem bit for bit (pose, trim, reference points, v_ref, boundaries, obstacles) and the state after every
    apply; the planner is the reference joint search.  Three vehicles start from standstill with 12^3 children at the root, so they
    run at Hp 3 (some 80 000 nodes in the first step; at Hp 4 some 350 000)."""
    options, sc, boundary = {"circle2": lambda: circle_case(2, 5), "circle3": lambda: circle_case(3, 3), "road2": road_case}[case]()
    mpa = centralized_mpa(options)
    nat = NativeController(options, sc, mpa, None, coupling="none")
    with_boundaries = []

    def plan(iters):
        k = py.k
        nat.centralized_build()
        got = nat.centralized_problem()
        cc.assert_same_iters(got, iters, "%s step %d" % (case, k))
        with_boundaries.append(all(it.predicted_lanelet_boundary[0] is not None for it in got))
        recs = jr.plan_joint(options, mpa, [iters])
        assert (recs["status"] == abi.OK).all()
        nat.centralized_apply(recs)
        return [info_from_record(r, options.Hp) for r in recs]

    py = CentralizedController(options, sc, mpa, plan, boundary_provider=boundary)
    for k in range(1, steps + 1):
        py.step()
        cc.assert_same_state(nat.state(), cc.state_of_twin(py), k, "%s after step %d" % (case, k))
    assert all(with_boundaries) == (case == "road2")
    moved = nat.state()
    assert (moved["speed"] > 0).all(), "the closed loop never left standstill: the later steps would repeat the first"
    nat.close()


def addresses(ps):
    return tuple(C.cast(p, C.c_void_p).value for p in (ps.offset, ps.x, ps.y)) + (ps.n_polygons,)


def test_every_vehicle_points_to_the_same_obstacle_arrays():
    """What lets the packer and the joint kernel hold the scenario's set once: the same pointers in every entry of the problem (a
    road network: the boundaries are the vehicles' own)."""
    options, sc, _ = road_case()
    sc.obstacles = [cc.rectangle(50.0, 50.0), cc.rectangle(60.0, 50.0)]
    nat = NativeController(options, sc, centralized_mpa(options), None, coupling="none")
    for _ in range(2):
        nat.centralized_build()
        n, vin = nat.centralized_problem(raw=True)
        assert n == 2
        assert vin[0].obstacles.n_polygons == 2
        assert addresses(vin[0].obstacles) == addresses(vin[1].obstacles)
        assert vin[0].dynamic_obstacles.n_polygons == 0 and vin[1].dynamic_obstacles.n_polygons == 0
        assert vin[0].hdv_reachable_sets.n_polygons == 0 and vin[1].hdv_reachable_sets.n_polygons == 0
        assert vin[0].n_left >= 2 and vin[1].n_left >= 2
        assert C.cast(vin[0].left_x, C.c_void_p).value != C.cast(vin[1].left_x, C.c_void_p).value
    nat.close()


def test_apply_with_an_exhausted_record_applies_nothing():
    """The reference has no fallback for this controller and the twin raises: natively apply returns PDMPC_EXHAUSTED, the plant stays
    where it was and the time step stays advanced -- also when only one vehicle's record carries the status."""
    options, sc, _ = circle_case(2, 4)
    mpa = centralized_mpa(options)
    nat = NativeController(options, sc, mpa, None, coupling="none")
    good = cc.reference_loop(2, 4, 2)
    nat.centralized_build()
    nat.centralized_apply(good[0])
    before = nat.state()
    assert before["k"] == 1
    nat.centralized_build()
    bad = good[1].copy()
    bad["status"][1] = abi.EXHAUSTED
    with pytest.raises(BackendError, match="exhausted at time step 2") as e:
        nat.centralized_apply(bad)
    assert e.value.status == abi.EXHAUSTED
    after = nat.state()
    cc.assert_same_state(after, before, 2, "after the refused apply")
    # the twin, handed the same records, raises at the same step
    def plan(iters):
        recs = good[py.k - 1] if py.k == 1 else bad
        return [info_from_record(r, options.Hp) for r in recs]

    py = CentralizedController(options, sc, mpa, plan)
    py.step()
    with pytest.raises(CentralizedExhaustedError):
        py.step()
    assert py.k == 2
    # ... and the records of the step are accepted afterwards (nothing was half applied): the twin that was never refused
    nat.centralized_apply(good[1])
    py2 = CentralizedController(options, sc, mpa, lambda iters: [info_from_record(r, options.Hp) for r in good[py2.k - 1]])
    py2.step()
    py2.step()
    cc.assert_same_state(nat.state(), cc.state_of_twin(py2), 2, "after the accepted apply")
    nat.close()


def plan_problems(options_of, problems):
    """jr.plan_joint for every problem of a sweep with its own member's options (the members differ in vehicle count)"""
    return np.concatenate([jr.plan_joint(o, centralized_mpa(o), [prob]) for o, prob in zip(options_of, problems)])


def test_sweep_without_a_handle_equals_the_solo_runs_and_retires_an_exhausted_member():
    """Members of 1, 2 and 3 vehicles at Hp 3 on circles turned against each other.  The concatenated problems and their tags; after
    centralized_apply each member is where its solo controller is; a member that is handed an exhausted record is retired -- not
    applied, not built again, its time step stands still -- while the others go on."""
    Hp = 3
    sizes, angles = (1, 2, 3), (0.0, 0.4, 0.9)
    options_of = [cc.circle_options(n, Hp) for n in sizes]
    members = [cc.native_on_circle(n, Hp, a) for n, a in zip(sizes, angles)]
    solo = [cc.native_on_circle(n, Hp, a) for n, a in zip(sizes, angles)]
    sweep = NativeSweep(members, None)
    assert sweep.centralized_status() == [0, 0, 0]
    live = [0, 1, 2]
    for step in range(1, 5):
        sweep.centralized_build()
        q = sweep.centralized_problem()
        assert q["member"] == live
        assert q["problem_offset"] == np.concatenate([[0], np.cumsum([sizes[m] for m in live])]).tolist()
        for m in live:
            solo[m].centralized_build()
        for p, m in enumerate(live):
            cc.assert_same_iters(q["problems"][p], solo[m].centralized_problem(), "step %d member %d" % (step, m))
        recs = plan_problems([options_of[m] for m in live], q["problems"])
        assert (recs["status"] == abi.OK).all()
        if step == 2:  # member 1's search "ran empty"
            a, b = q["problem_offset"][1], q["problem_offset"][2]
            recs[a:b] = cc.exhausted(recs[a:b])
        sweep.centralized_apply(recs)
        for p, m in enumerate(live):
            a, b = q["problem_offset"][p], q["problem_offset"][p + 1]
            if step == 2 and m == 1:
                with pytest.raises(BackendError) as e:
                    solo[m].centralized_apply(recs[a:b])
                assert e.value.status == abi.EXHAUSTED
            else:
                solo[m].centralized_apply(recs[a:b])
        for m in range(3):
            cc.assert_same_native_state(members[m], solo[m], "step %d member %d" % (step, m))
        if step == 2:
            live = [0, 2]
        assert sweep.centralized_status() == ([0, 0, 0] if step < 2 else [0, 2, 0])
    assert [m.state()["k"] for m in members] == [4, 2, 4]
    sweep.close()
    for c in members + solo:
        c.close()


def test_sweep_whose_members_are_all_retired_builds_nothing():
    members = [cc.native_on_circle(1, 3, 0.0), cc.native_on_circle(2, 3, 0.5)]
    sweep = NativeSweep(members, None)
    sweep.centralized_build()
    q = sweep.centralized_problem()
    recs = plan_problems([cc.circle_options(1, 3), cc.circle_options(2, 3)], q["problems"])
    sweep.centralized_apply(cc.exhausted(recs))
    assert sweep.centralized_status() == [1, 1]
    sweep.centralized_build()
    q = sweep.centralized_problem()
    assert q["member"] == [] and q["problem_offset"] == [0]
    assert [m.state()["k"] for m in members] == [1, 1]
    sweep.close()
    for c in members:
        c.close()


def test_rejections():
    """More than PDMPC_JOINT_MAX vehicles: PDMPC_ERR_CAPACITY from every entry point, for a controller and for a member, before
    anything advances; step and run without a handle: PDMPC_ERR_INVALID; apply and problem before a build: PDMPC_ERR_INVALID."""
    five = cc.native_on_circle(5, 3)
    with pytest.raises(BackendError, match="PDMPC_JOINT_MAX") as e:
        five.centralized_build()
    assert e.value.status == ERR_CAPACITY
    for call in (five.centralized_step, lambda: five.centralized_run(2)):  # (without a handle that is what is refused first)
        with pytest.raises(BackendError, match="no backend handle") as e:
            call()
        assert e.value.status == ERR_INVALID
    assert five.state()["k"] == 0
    two = cc.native_on_circle(2, 3)
    sweep = NativeSweep([two, five], None)
    with pytest.raises(BackendError, match="PDMPC_JOINT_MAX") as e:
        sweep.centralized_build()
    assert e.value.status == ERR_CAPACITY
    assert two.state()["k"] == 0 and five.state()["k"] == 0
    sweep.close()
    for call in (two.centralized_step, lambda: two.centralized_run(1)):
        with pytest.raises(BackendError, match="no backend handle") as e:
            call()
        assert e.value.status == ERR_INVALID
    for call in (two.centralized_problem, lambda: two.centralized_apply(abi.out_array(2)[:2])):
        with pytest.raises(BackendError, match="before pdmpc_controller_centralized_build") as e:
            call()
        assert e.value.status == ERR_INVALID
    sweep = NativeSweep([two], None)
    for call in (sweep.centralized_step, lambda: sweep.centralized_run(1)):
        with pytest.raises(BackendError, match="no backend handle") as e:
            call()
        assert e.value.status == ERR_INVALID
    with pytest.raises(BackendError, match="before pdmpc_sweep_centralized_build"):
        sweep.centralized_apply(abi.out_array(2)[:2])
    assert two.state()["k"] == 0
    # ... and none of the refusals broke anything: a step still builds
    sweep.centralized_build()
    assert two.state()["k"] == 1
    sweep.close()
    two.close()
    five.close()


def test_polygon_sets_of_the_same_arrays_are_packed_once():
    """abi.pack_vehicles hands the packer the same arrays for vehicles whose obstacle lists hold the same array objects, as
    CentralizedController.build_iters' do; lists of equal but distinct arrays stay apart."""
    options, sc, _ = circle_case(3, 3)
    ctl = CentralizedController(options, sc, centralized_mpa(options), None)
    iters = ctl.build_iters()
    arr, keep = abi.pack_vehicles(iters, options.Hp)
    assert arr[0].obstacles.n_polygons == 2
    assert addresses(arr[0].obstacles) == addresses(arr[1].obstacles) == addresses(arr[2].obstacles)
    iters[1].obstacles = [o.copy() for o in iters[1].obstacles]
    arr, keep = abi.pack_vehicles(iters, options.Hp)
    assert addresses(arr[0].obstacles) == addresses(arr[2].obstacles) != addresses(arr[1].obstacles)
    del keep
