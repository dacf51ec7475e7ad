"""The sampled optimizer's whole-step path without a GPU: the reference helper (sampled_step_reference.py) against the Python
controller's own level loop, the native controller with PDMPC_OPTIMIZER_SAMPLED against its Python twin (planner = the reference
helper), and the argument checks of the new entry points."""
import ctypes as C

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController

import sampled_step_reference as ref_step
from test_native_controller import assert_same_problem

ERR_INVALID = -1


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def oracle_level_loop(options, mpa):
    from oracle import oracle

    def plan_level(iters, seeds):
        _, recs = oracle.plan_batch_sampled(options, mpa, iters, seeds, n_threads=min(16, len(iters)))
        return [info_from_record(recs[i], options.Hp) for i in range(len(iters))]

    plan_level.wants_seeds = True
    return plan_level


def helper_loop_equals_level_loop(options, scenario, coupling, n_steps, boundary=None, force_exhaustion=None):
    mpa = get_mpa(options)
    lvl = PrioritizedSequentialController(options, scenario, mpa, oracle_level_loop(options, mpa), coupling=coupling, boundary_provider=boundary)
    one = PrioritizedSequentialController(options, scenario, mpa, None, coupling=coupling, boundary_provider=boundary)
    exhausted = 0
    for k in range(n_steps):
        infos_lvl = lvl.step()

        def plan_step(prob):
            recs = ref_step.plan_step_sampled(options, mpa, prob, ref_step.step_seeds(prob, one.k))
            return [info_from_record(recs[i], options.Hp) for i in range(len(recs))]

        infos_one = one.step(plan_step=plan_step)
        exhausted += sum(1 for i in infos_one if i.is_exhausted)
        for a, b in zip(infos_lvl, infos_one):
            assert a.is_exhausted == b.is_exhausted and a.needs_fallback == b.needs_fallback, k
            assert np.array_equal(bits(a.y_predicted), bits(b.y_predicted)), k
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a.shapes, b.shapes)), k
        assert np.array_equal(bits([m.x for m in lvl.meas]), bits([m.x for m in one.meas])), k
        assert np.array_equal(bits([m.yaw for m in lvl.meas]), bits([m.yaw for m in one.meas])), k
    return exhausted


def test_reference_helper_equals_the_level_loop_on_the_road_network():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8)
    sc = commonroad_scenario(options, seed=1)
    helper_loop_equals_level_loop(options, sc, "distance", 10, boundary_provider(sc))


def test_reference_helper_equals_the_level_loop_on_the_circle():
    """Full coupling, separating-axis checks; the sampled searches of the later levels run empty (exhaustion, fallbacks)."""
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=8, Hp=6)
    exhausted = helper_loop_equals_level_loop(options, circle_scenario(options), "full", 10)
    assert exhausted > 0, "no search ran empty: the fallback hand-over was not exercised"


def native_twin(options, sc, coupling, boundary, n_steps):
    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling=coupling, boundary_provider=boundary)
    nat = NativeController(options, sc, mpa, None, coupling=coupling, optimizer="sampled")
    for k in range(n_steps):
        nat.build_step()
        q = nat.problem()
        seeds = nat.seeds()
        assert seeds == ref_step.step_seeds(q, k + 1)

        def plan_step(prob):
            assert_same_problem(prob, q, "step %d" % (k + 1))
            recs = ref_step.plan_step_sampled(options, mpa, prob, seeds)
            nat.apply(recs)
            return [info_from_record(recs[i], options.Hp) for i in range(len(recs))]

        py.step(plan_step=plan_step)
        st = nat.state()
        assert np.array_equal(bits(st["x"]), bits([m.x for m in py.meas])) and np.array_equal(bits(st["y"]), bits([m.y for m in py.meas])), k
        assert np.array_equal(bits(st["yaw"]), bits([m.yaw for m in py.meas])), k
        assert st["needs_fallback"].tolist() == [bool(i.needs_fallback) for i in py.infos], k
    return py, nat, mpa


def test_native_controller_equals_its_twin_on_the_road_network():
    from pdmpc.explorative import explore_step
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8)
    sc = commonroad_scenario(options, seed=1)
    py, nat, mpa = native_twin(options, sc, "distance", boundary_provider(sc), 10)
    # an explorative step (n_perm 4): the seeds of every instance are the step's, the choice is pdmpc.explorative's
    K = 4
    nat.explore_build(K, seed=py.k + 1)
    q = nat.explore_problem()
    seeds = nat.seeds()
    assert seeds == ref_step.step_seeds(q, py.k + 1) and len(seeds) == K * options.amount

    def plan_batch(batch):
        assert_same_problem(batch, q, "explorative step")
        recs = ref_step.plan_step_sampled(options, mpa, batch, seeds)
        plan_batch.chosen_nat, _ = nat.explore_choose(recs)
        return recs

    _, _, chosen = explore_step(py, plan_batch, K)
    assert chosen == plan_batch.chosen_nat.tolist()
    nat.close()


def test_native_controller_equals_its_twin_on_the_circle_and_the_optimal_choice():
    from pdmpc.optimal import optimal_step
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=6)
    py, nat, mpa = native_twin(options, circle_scenario(options), "full", None, 10)
    nat.L.pdmpc_controller_optimal_build(nat.c, 24)
    seeds = nat.seeds()
    assert len(seeds) == 24 * options.amount

    def plan_batch(batch):
        assert seeds == ref_step.step_seeds(batch, py.k)
        recs = ref_step.plan_step_sampled(options, mpa, batch, seeds)
        chosen = np.zeros(options.amount, dtype=np.int32)
        cost = np.zeros(options.amount * 24)
        assert nat.L.pdmpc_controller_optimal_choose(nat.c, abi.out_ptr(np.ascontiguousarray(recs)), chosen.ctypes.data_as(abi.c_int32_p),
                                                     cost.ctypes.data_as(abi.c_double_p)) == 0
        plan_batch.chosen_nat = chosen
        return recs

    _, _, chosen = optimal_step(py, plan_batch, 24)
    assert chosen == plan_batch.chosen_nat.tolist()
    nat.close()


def test_argument_checks():
    from pdmpc.backend import load_library
    from pdmpc.scenario import circle_scenario

    L = load_library()
    options = Config(scenario_type=ScenarioType.circle, amount=2, Hp=5)
    nat = NativeController(options, circle_scenario(options), get_mpa(options), None)
    assert L.pdmpc_controller_set_optimizer(nat.c, 2) == ERR_INVALID
    assert L.pdmpc_controller_set_optimizer(nat.c, -1) == ERR_INVALID
    assert L.pdmpc_controller_set_optimizer(None, 1) == ERR_INVALID
    # the default optimizer is the graph search: a controller with a handle plans with pdmpc_plan_step (pdmpc_controller_step), and
    # without one the seeds are reported whatever the optimizer
    nat.build_step()
    assert nat.seeds() == [2, 3]
    assert L.pdmpc_controller_set_optimizer(nat.c, 1) == 0 and L.pdmpc_controller_set_optimizer(nat.c, 0) == 0
    nat.close()
    # NULL handle, NULL seeds with n > 0
    vin = (abi.VehicleIn * 1)()
    out = (abi.VehicleOut * 1)()
    assert L.pdmpc_plan_step_sampled(None, 1, vin, None, None, None, (C.c_uint32 * 1)(1), out) == ERR_INVALID
    assert L.pdmpc_plan_step_sampled(None, 1, vin, None, None, None, None, out) == ERR_INVALID
    assert L.pdmpc_set_step_seeds(None, 1, (C.c_uint32 * 1)(1)) == ERR_INVALID


def test_controller_problem_carries_the_time_step():
    from pdmpc.explorative import build_exploration_batch
    from pdmpc.optimizer import MonteCarloTreeSearchHip
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=3, Hp=5)
    ctl = PrioritizedSequentialController(options, circle_scenario(options), get_mpa(options), None, coupling="full")
    ctl.k = 7
    prob = ctl.build_step_problem()
    assert MonteCarloTreeSearchHip.step_seeds(prob) == [8, 9, 10] == ref_step.step_seeds(prob, 7)
    batch = build_exploration_batch(ctl, 2, seed=7)
    assert MonteCarloTreeSearchHip.step_seeds(batch) == [7 + v + 1 for v in batch["vehicle"]]
