"""HDVs in the Python controller (PrioritizedSequentialController.set_hdvs) on the CPU: what a search receives, that the
oracle's plans respect it, that the traffic call's three twins give the controller the same problems, and that nothing changes without
HDVs."""
import numpy as np
import pytest

import hdv_cases as H
from oracle import oracle
from pdmpc import backend, hdv
from pdmpc.config import Config, ScenarioType
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController
from test_native_controller import assert_same_problem


def _oracle_planner(options):
    mpa = get_mpa(options)

    def plan(prob):
        recs, _ = oracle.plan_step(options, mpa, prob)
        return [info_from_record(r, options.Hp) for r in recs]

    return plan


def _problem_bytes(prob, Hp):
    """what distinguishes two step problems that assert_same_problem (tests/test_native_controller.py) has found equal otherwise: the
    HDV sets, bit for bit, with the order and the couplings"""
    sets = [[np.ascontiguousarray(p).tobytes() for row in it.hdv_reachable_sets for p in row] for it in prob["iters"]]
    return prob["order"], prob["preds"], prob["level_sizes"], sets, [(it.x0.tobytes(), np.asarray(it.reference_trajectory_points).tobytes()) for it in prob["iters"]]


def test_an_hdv_ahead_changes_the_plan_and_the_plan_stays_out_of_its_sets():
    """The committed pose: an HDV standing on CAV 0's lane 0.6 m ahead of it.  CAV 0's oracle plan differs from the run without the HDV,
    and no edge of any step's area crosses an edge of that step's reachable lanes."""
    base = H.loop_controller(H.loop_options(0, max_nodes=1 << 16))
    base.step(plan_step=_oracle_planner(base.options))
    ctl = H.loop_controller(H.loop_options(1, max_nodes=1 << 16))
    ctl.set_hdv_measurements(*[[v] for v in H.HDV_AHEAD_POSE])
    ctl.step(plan_step=_oracle_planner(ctl.options))
    assert ctl.hdv_info["adjacency"][0, 0] == 1
    it0 = ctl.last_problem["iters"][ctl.last_problem["order"].index(0)]
    assert len(it0.hdv_reachable_sets) == len(ctl.hdv_info["row_hdv"]) >= 1 and all(len(row) == 6 for row in it0.hdv_reachable_sets)
    a, b = base.infos[0], ctl.infos[0]
    assert not a.is_exhausted and not b.is_exhausted
    assert not np.array_equal(a.y_predicted, b.y_predicted) and list(a.predicted_trims) != list(b.predicted_trims)
    # the run without the HDV drives through its sets, the run with it does not touch them
    through = sum(H.crossings(a.shapes[k], row[k]) for row in it0.hdv_reachable_sets for k in range(6))
    assert through > 0
    for k in range(6):
        for row in it0.hdv_reachable_sets:
            assert H.crossings(b.shapes[k], row[k]) == 0, k


def test_the_three_twins_give_the_controller_the_same_problems_over_6_steps():
    """4 CAVs, 2 HDVs moved by the test along the loop at constant speed, Hp 6: the numpy twin and the host twin as the controller's
    traffic call build the same problems, HDV sets bit for bit"""
    sets, hmap = H.local_sets(6), hdv.lab_hdv_map()
    a = H.loop_controller(H.loop_options(2, max_nodes=1 << 16))
    b = H.loop_controller(H.loop_options(2, max_nodes=1 << 16), traffic=lambda *args: hdv.hdv_traffic_native(hmap, sets, *args))
    plan = _oracle_planner(a.options)
    received = 0
    for step in range(1, 7):
        for c in (a, b):
            c.set_hdv_measurements(*H.hdv_poses_at(step))
            c.step(plan_step=plan)
        H.assert_same(a.hdv_info, b.hdv_info, step)
        assert_same_problem(a.last_problem, b.last_problem, "step %d" % step)
        assert _problem_bytes(a.last_problem, 6) == _problem_bytes(b.last_problem, 6)
        received += sum(len(it.hdv_reachable_sets) for it in a.last_problem["iters"])
        for i in range(4):
            assert np.array_equal(a.infos[i].y_predicted, b.infos[i].y_predicted)
    assert received > 0


def test_without_hdvs_nothing_changes():
    """manual_control 0, and HDVs that are adjacent to nobody (on another copy of the map): the problems of a controller that has never
    heard of HDVs"""
    plain = H.loop_controller(H.loop_options(0, max_nodes=1 << 16))
    far = H.loop_controller(H.loop_options(1, max_nodes=1 << 16))
    far.hdvs["tile"] = [(120.0, 0.0)]
    far.set_hdv_measurements([H.HDV_AHEAD_POSE[0] + 120.0], [H.HDV_AHEAD_POSE[1]], [H.HDV_AHEAD_POSE[2]])
    plan = _oracle_planner(plain.options)
    for _ in range(3):
        plain.step(plan_step=plan)
        far.step(plan_step=plan)
        assert not far.hdv_info["adjacency"].any()
        assert all(it.hdv_reachable_sets == [] for it in far.last_problem["iters"])
        assert_same_problem(plain.last_problem, far.last_problem, "without HDVs")
        assert _problem_bytes(plain.last_problem, 6) == _problem_bytes(far.last_problem, 6)


def test_rejections():
    from pdmpc.controller import PrioritizedSequentialController
    from pdmpc.scenario import circle_scenario

    sets, hmap = H.local_sets(6), hdv.lab_hdv_map()
    with pytest.raises(ValueError):  # no HDVs configured
        H.loop_controller(H.loop_options(0)).set_hdvs(sets, hmap)
    circle = Config(scenario_type=ScenarioType.circle, amount=3, Hp=6, manual_control=1)
    with pytest.raises(ValueError):  # a scenario without lanelets
        PrioritizedSequentialController(circle, circle_scenario(circle), get_mpa(circle), None).set_hdvs(sets, hmap)
    ctl = H.loop_controller(H.loop_options(2))
    with pytest.raises(ValueError):  # one pose for two HDVs
        ctl.set_hdv_measurements([0.0], [0.0], [0.0])
    with pytest.raises(ValueError):  # a step before the first measurement
        ctl.step(plan_step=_oracle_planner(ctl.options))


# ---- the native step controller (pdmpc_controller_set_hdvs) against the Python twin


def _hdv_mpa(Hp):
    """the HDVs' automaton: single_speed without the recursive-feasibility mask (ManualVehicle.m:20-27)"""
    from pdmpc.config import MpaType

    return get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=Hp, mpa_type=MpaType.single_speed, recursive_feasibility=False))


def _twins(options, handle=None, tile=None):
    """the Python controller and the native one on the four-CAV loop with options.manual_control HDVs on the scenario's own lanelets"""
    from pdmpc.controller import PrioritizedSequentialController
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    sc = commonroad_scenario(options, seed=1)
    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    nat = NativeController(options, sc, mpa, handle, coupling="distance")
    if options.manual_control:
        hmap = hdv.scenario_hdv_map(sc)
        py.set_hdvs(H.local_sets(options.Hp), hmap, tile=tile)
        nat.set_hdvs(_hdv_mpa(options.Hp), hmap.successors, hmap.relationship, tile=tile)
    return py, nat


def _same_info(a, b, what):
    H.assert_same({k: v for k, v in a.items() if k != "set_offset"}, {k: v for k, v in b.items() if k != "set_offset"}, what)


def test_native_problems_equal_the_python_twins_over_6_steps():
    """4 CAVs, 2 HDVs moved by the test along the loop at constant speed, Hp 6, the oracle as the planner: every step's problem --
    order, couplings, poses, references, boundaries, obstacles, fallbacks and the HDV sets -- bit for bit, and the traffic info itself"""
    options = H.loop_options(2, max_nodes=1 << 16)
    mpa = get_mpa(options)
    py, nat = _twins(options)
    received = 0
    for step in range(1, 7):
        pose = H.hdv_poses_at(step)
        py.set_hdv_measurements(*pose)
        nat.set_hdv_measurements(*pose)
        nat.build_step()
        q = nat.problem()
        info = nat.hdv_info()

        def plan_step(prob):
            assert_same_problem(prob, q, "step %d" % step)
            assert _problem_bytes(prob, 6)[3] == _problem_bytes(q, 6)[3], step  # (the HDV sets; everything else: assert_same_problem)
            recs, _ = oracle.plan_step(options, mpa, prob)
            nat.apply(recs)
            return [info_from_record(recs[i], options.Hp) for i in range(len(recs))]

        py.step(plan_step=plan_step)
        _same_info(py.hdv_info, info, "step %d" % step)
        received += sum(len(it.hdv_reachable_sets) for it in q["iters"])
        st = nat.state()
        assert np.array_equal(st["x"], np.array([m.x for m in py.meas])) and np.array_equal(st["yaw"], np.array([m.yaw for m in py.meas])), step
    assert received > 0
    nat.close()


def test_native_explorative_and_optimal_batches_carry_the_same_rows_in_every_instance():
    from pdmpc.explorative import build_exploration_batch

    options = H.loop_options(2, max_nodes=1 << 16)
    py, nat = _twins(options)
    pose = H.hdv_poses_at(1)
    py.set_hdv_measurements(*pose)
    nat.set_hdv_measurements(*pose)
    py.k += 1
    batch = build_exploration_batch(py, 4, seed=py.k)
    nat.explore_build(4, 1)
    q = nat.explore_problem()
    assert q["instance"] == batch["instance"] and q["vehicle"] == batch["vehicle"]
    assert _problem_bytes(q, 6)[3] == _problem_bytes(batch, 6)[3] and any(_problem_bytes(q, 6)[3])
    nat.close()


def test_a_native_controller_without_hdvs_builds_what_it_built_before():
    """manual_control 0 against HDVs that are adjacent to nobody (another copy of the map): the same problems, 3 steps"""
    plain_py, plain = _twins(H.loop_options(0, max_nodes=1 << 16))
    far_py, far = _twins(H.loop_options(1, max_nodes=1 << 16), tile=[(120.0, 0.0)])
    far.set_hdv_measurements([H.HDV_AHEAD_POSE[0] + 120.0], [H.HDV_AHEAD_POSE[1]], [H.HDV_AHEAD_POSE[2]])
    mpa = get_mpa(plain.options)
    for step in range(3):
        plain.build_step()
        far.build_step()
        p, q = plain.problem(), far.problem()
        assert_same_problem(p, q, step)
        assert all(it.hdv_reachable_sets == [] for it in q["iters"]) and not far.hdv_info()["adjacency"].any()
        recs, _ = oracle.plan_step(plain.options, mpa, p)
        plain.apply(recs)
        far.apply(recs)
    plain.close()
    far.close()


def test_native_rejections():
    """PDMPC_ERR_INVALID: a scenario without lanelets; centralized_build with HDVs set; a step before the first measurement (the third
    of the issue's cases, the separating-axis checker, needs a handle: tests/test_gpu_hdv_controller.py)"""
    from pdmpc.scenario import circle_scenario

    hmap = hdv.lab_hdv_map()
    circle = Config(scenario_type=ScenarioType.circle, amount=3, Hp=6, manual_control=1)
    nat = NativeController(circle, circle_scenario(circle), get_mpa(circle), None)
    with pytest.raises(backend.BackendError) as e:
        nat.set_hdvs(_hdv_mpa(6), hmap.successors, hmap.relationship)
    assert e.value.status == -1 and "lanelets" in str(e.value)
    nat.close()
    _, nat = _twins(H.loop_options(2))
    with pytest.raises(backend.BackendError) as e:
        nat.build_step()
    assert e.value.status == -1 and "measurements" in str(e.value)
    nat.set_hdv_measurements(*H.hdv_poses_at(1))
    with pytest.raises(backend.BackendError) as e:
        nat.centralized_build()
    assert e.value.status == -1 and "HDV" in str(e.value)
    nat.build_step()  # (and a prioritized step is built)
    nat.close()
    with pytest.raises(ValueError):  # the Python twin: the centralized controller refuses HDVs as well
        from pdmpc.centralized import CentralizedController
        from pdmpc.road_network import boundary_provider, commonroad_scenario

        o = H.loop_options(1)
        sc = commonroad_scenario(o, seed=1)
        CentralizedController(o, sc, get_mpa(o), None, boundary_provider=boundary_provider(sc)).set_hdvs(H.local_sets(6), hmap)
