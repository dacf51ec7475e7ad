"""Closed loops with HDVs on the MI355X: 4 CAVs and 2 HDVs the test moves along the loop, Hp 6, 6 steps of the
Python controller.  Every step's traffic info comes from ONE pdmpc_hdv_traffic on the searches' handle and equals the host twin's; every
step is planned by one launch whose searches receive the adjacent HDVs' rows, and the records equal the oracle's on the controller's own
problems -- with the graph search, with the sampled optimizer, and for one explorative step of 4 prioritizations."""
import numpy as np
import pytest

import hdv_cases as H
import sampled_step_reference as ref_step
from oracle import oracle
from pdmpc import hdv
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa
from test_gpu_parity import assert_records_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


def _device_controller(opt, options):
    """the loop controller whose traffic call runs on opt's handle, checked against the host twin call by call"""
    sets, hmap = H.local_sets(options.Hp), hdv.lab_hdv_map()
    hdv.upload_hdv_map(opt.handle, hmap, sets)  # (the module's calls: they take a group's rank-0 handle as well)
    calls = []

    def traffic(*args):
        dev = hdv.hdv_traffic_native(None, None, *args, handle=opt.handle)
        H.assert_same(dev, hdv.hdv_traffic_native(hmap, sets, *args), "step's traffic call")
        calls.append(len(dev["row_hdv"]))
        return dev

    return H.loop_controller(options, traffic=traffic), calls


def _run(opt, options, plan_records, reference, steps=6):
    mpa = get_mpa(options)
    ctl, calls = _device_controller(opt, options)
    received = crossing_free = 0

    def plan_step(prob):
        nonlocal received
        gpu = plan_records(prob, mpa)
        assert_records_equal(gpu, reference(prob, mpa, ctl), "step %d" % ctl.k)
        received += sum(len(it.hdv_reachable_sets) for it in prob["iters"])
        return [info_from_record(gpu[i], options.Hp) for i in range(len(gpu))]

    for step in range(1, steps + 1):
        ctl.set_hdv_measurements(*H.hdv_poses_at(step))
        ctl.step(plan_step=plan_step)
        for s, v in enumerate(ctl.last_problem["order"]):  # a plan that was found stays out of the sets its search received
            if not ctl.infos[v].is_exhausted:
                it = ctl.last_problem["iters"][s]
                assert all(H.crossings(ctl.infos[v].shapes[k], row[k]) == 0 for row in it.hdv_reachable_sets for k in range(options.Hp))
                crossing_free += len(it.hdv_reachable_sets)
    assert len(calls) == steps and min(calls) >= 2  # ONE traffic call per step
    assert received > 0 and crossing_free > 0
    return ctl


def test_closed_loop_with_the_graph_search():
    from pdmpc.optimizer import GraphSearchHip

    options = H.loop_options(2, max_nodes=1 << 16, max_vehicles=16)
    opt = GraphSearchHip(options)

    def plan(prob, mpa):
        opt._ensure_mpa(mpa)
        return opt.handle.plan_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])

    _run(opt, options, plan, lambda prob, mpa, ctl: oracle.plan_step(options, mpa, prob)[0])
    assert opt.handle.stats()["kernel"] == 2
    opt.handle.close()


def test_closed_loop_with_the_sampled_optimizer():
    from pdmpc.optimizer import MonteCarloTreeSearchHip

    options = H.loop_options(2, max_vehicles=16)
    opt = MonteCarloTreeSearchHip(options)
    _run(opt, options, opt.plan_step_records, lambda prob, mpa, ctl: ref_step.plan_step_sampled(options, mpa, prob, ref_step.step_seeds(prob, ctl.k)))
    opt.handle.close()


def test_one_explorative_step_of_4_prioritizations():
    from pdmpc.explorative import explore_step
    from pdmpc.optimizer import GraphSearchHip

    options = H.loop_options(2, max_nodes=1 << 16, max_vehicles=32)
    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    ctl, calls = _device_controller(opt, options)
    ctl.set_hdv_measurements(*H.hdv_poses_at(1))

    def plan_batch(batch):
        gpu = opt.handle.plan_step(batch["iters"], batch["preds"], [f if f is not None else [] for f in batch["fallback"]])
        assert_records_equal(gpu, oracle.plan_step(options, mpa, batch)[0], "explorative batch")
        return gpu

    batch, records, chosen = explore_step(ctl, plan_batch, 4)
    assert batch["n_instances"] == 4 and len(records) == 16
    # the same rows for a vehicle in every instance (instances 2 .. 4 are built from the traffic state instance 1 refreshed)
    per_vehicle = {}
    for it, v in zip(batch["iters"], batch["vehicle"]):
        key = [np.ascontiguousarray(p).tobytes() for row in it.hdv_reachable_sets for p in row]
        assert per_vehicle.setdefault(v, key) == key
    assert any(per_vehicle[v] for v in per_vehicle)
    opt.handle.close()


def test_closed_loop_on_a_group_of_two_logical_ranks():
    """the same loop planned by a group of two ranks on one GPU; the traffic call runs on rank 0's handle and the sets travel in the
    vehicles' records as always"""
    from pdmpc import backend
    from pdmpc.backend import Group

    options = H.loop_options(2, max_nodes=1 << 16, max_vehicles=16)
    g = Group(options, n_devices=2, devices=[0, 0], collective=backend.COLLECTIVE_COPY)
    g.upload_mpa(get_mpa(options))

    class OnRank0:
        handle = g.rank0()

    plan = lambda prob, mpa: g.plan_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])  # noqa: E731
    _run(OnRank0, options, plan, lambda prob, mpa, ctl: oracle.plan_step(options, mpa, prob)[0])
    g.close()


# ---- the native step controller with HDVs (pdmpc_controller_set_hdvs): its traffic call runs on the handle, its steps are one launch


def _hdv_mpa(Hp):
    from pdmpc.config import Config, MpaType, ScenarioType

    return get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=Hp, mpa_type=MpaType.single_speed, recursive_feasibility=False))


def _native_twins(options, handle, optimizer="graph_search"):
    """(the Python controller with the numpy twin as its traffic call, the native controller on `handle`), HDVs on the scenario's lanelets"""
    from pdmpc.controller import PrioritizedSequentialController
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    sc = commonroad_scenario(options, seed=1)
    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    nat = NativeController(options, sc, mpa, handle, coupling="distance", optimizer=optimizer)
    if options.manual_control:
        hmap = hdv.scenario_hdv_map(sc)
        py.set_hdvs(H.local_sets(options.Hp), hmap)
        nat.set_hdvs(_hdv_mpa(options.Hp), hmap.successors, hmap.relationship)
    return py, nat


def _native_loop(py, nat, options, reference, step_native=None, steps=6):
    """6 steps: the native step (traffic call on the device, ONE launch) ends where the Python twin planned by the reference ends; the
    problems, the traffic info and the records are the same"""
    from test_native_controller import assert_same_problem

    mpa = get_mpa(options)
    received = 0
    for step in range(1, steps + 1):
        pose = H.hdv_poses_at(step)
        py.set_hdv_measurements(*pose)
        nat.set_hdv_measurements(*pose)
        recs = step_native() if step_native else nat.step()
        q, info = nat.problem(), nat.hdv_info()

        def plan_step(prob):
            assert_same_problem(prob, q, "step %d" % step)
            for a, b in zip(prob["iters"], q["iters"]):
                assert [p.tobytes() for row in a.hdv_reachable_sets for p in row] == [np.ascontiguousarray(p).tobytes() for row in b.hdv_reachable_sets for p in row]
            ref = reference(prob, mpa, py)
            assert_records_equal(recs, ref, "native step %d" % step)
            return [info_from_record(ref[i], options.Hp) for i in range(len(ref))]

        py.step(plan_step=plan_step)
        H.assert_same({k: v for k, v in py.hdv_info.items()}, info, "traffic info of step %d" % step)
        received += sum(len(it.hdv_reachable_sets) for it in q["iters"])
        st = nat.state()
        assert np.array_equal(st["x"], np.array([m.x for m in py.meas])) and np.array_equal(st["yaw"], np.array([m.yaw for m in py.meas])), step
    assert received > 0 and nat.last_timing()["build"] > 0


def test_native_closed_loop_with_the_graph_search_and_one_explorative_step():
    from pdmpc.explorative import explore_step
    from pdmpc.optimizer import GraphSearchHip

    options = H.loop_options(2, max_nodes=1 << 16, max_vehicles=32)
    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    py, nat = _native_twins(options, opt.handle)
    _native_loop(py, nat, options, lambda prob, mpa, ctl: oracle.plan_step(options, mpa, prob)[0])
    pose = H.hdv_poses_at(7)
    py.set_hdv_measurements(*pose)
    nat.set_hdv_measurements(*pose)
    recs, chosen_nat = nat.explore_step(4)
    kept = {}

    def plan_batch(batch):
        kept["ref"] = oracle.plan_step(options, mpa, batch)[0]
        return kept["ref"]

    _, _, chosen = explore_step(py, plan_batch, 4)
    assert list(chosen_nat) == chosen
    assert_records_equal(recs, kept["ref"], "native explorative step")
    st = nat.state()
    assert np.array_equal(st["x"], np.array([m.x for m in py.meas]))
    nat.close()
    opt.handle.close()


def test_native_closed_loop_with_the_sampled_optimizer():
    from pdmpc.backend import Handle

    options = H.loop_options(2, max_vehicles=16)
    h = Handle(options)
    h.upload_mpa(get_mpa(options))
    py, nat = _native_twins(options, h, optimizer="sampled")
    _native_loop(py, nat, options, lambda prob, mpa, ctl: ref_step.plan_step_sampled(options, mpa, prob, ref_step.step_seeds(prob, ctl.k)))
    nat.close()
    h.close()


def test_native_closed_loop_on_a_group_and_in_a_sweep():
    """on a group of two logical ranks the traffic call runs on rank 0's handle; in a sweep a member with HDVs makes its own call next to
    a member without"""
    from pdmpc import backend
    from pdmpc.backend import Group
    from pdmpc.native_controller import NativeSweep

    options = H.loop_options(2, max_nodes=1 << 16, max_vehicles=16)
    g = Group(options, n_devices=2, devices=[0, 0], collective=backend.COLLECTIVE_COPY)
    g.upload_mpa(get_mpa(options))
    py, nat = _native_twins(options, g.rank0())
    nat.set_group(g, backend.SHARD_AUTO)
    _native_loop(py, nat, options, lambda prob, mpa, ctl: oracle.plan_step(options, mpa, prob)[0], steps=3)
    nat.close()
    # the sweep: member 0 with HDVs, member 1 without, each against its twin stepped alone on the same handle
    plain = H.loop_options(0, max_nodes=1 << 16, max_vehicles=16)
    solo = [_native_twins(options, g.rank0())[1], _native_twins(plain, g.rank0())[1]]
    swept = [_native_twins(options, g.rank0())[1], _native_twins(plain, g.rank0())[1]]
    sweep = NativeSweep(swept, g.rank0())
    for step in range(1, 4):
        for c in (solo[0], swept[0]):
            c.set_hdv_measurements(*H.hdv_poses_at(step))
        alone = [c.step() for c in solo]
        together = sweep.step()
        for i in range(2):
            assert together[i].tobytes() == alone[i].tobytes(), (step, i)
        H.assert_same(solo[0].hdv_info(), swept[0].hdv_info(), "sweep member's traffic info")
    sweep.close()
    for c in solo + swept:
        c.close()
    g.close()


def test_native_rejection_of_the_separating_axis_checker():
    from pdmpc import abi, backend
    from pdmpc.backend import Handle
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import commonroad_scenario

    options = H.loop_options(1, max_vehicles=8)
    h = Handle(options, checker=abi.CHECK_SAT)
    h.upload_mpa(get_mpa(options))
    sc = commonroad_scenario(options, seed=1)
    nat = NativeController(options, sc, get_mpa(options), h, coupling="distance")
    hmap = hdv.scenario_hdv_map(sc)
    with pytest.raises(backend.BackendError) as e:
        nat.set_hdvs(_hdv_mpa(6), hmap.successors, hmap.relationship)
    assert e.value.status == -1 and "separating-axis" in str(e.value)
    nat.close()
    h.close()
