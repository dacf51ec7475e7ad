"""Whole time steps of the sampled optimizer in one launch (pdmpc_plan_step_sampled) on the GPU against the
oracle's sampled optimizer planned level by level (sampled_step_reference.py): records byte for byte, one launch per step."""
import copy

import numpy as np
import pytest

from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa

import sampled_step_reference as ref_step
from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu


def one_launch(h):
    st = h.stats()
    assert st["kernel"] == 3 and st["n_launches"] == 1 and st["safe_replans"] == 0, st


def closed_loop(options, scenario, coupling, n_steps, boundary=None, **kw):
    """n_steps of the Python controller, every step planned by one pdmpc_plan_step_sampled and compared with the reference."""
    from pdmpc.optimizer import MonteCarloTreeSearchHip

    mpa = get_mpa(options)
    opt = MonteCarloTreeSearchHip(options)
    ctl = PrioritizedSequentialController(options, scenario, mpa, None, coupling=coupling, boundary_provider=boundary, **kw)
    seen = {"levels": 0, "exhausted": 0}

    def plan_step(prob):
        gpu = opt.plan_step_records(prob, mpa)
        one_launch(opt.handle)
        ref = ref_step.plan_step_sampled(options, mpa, prob, ref_step.step_seeds(prob, ctl.k))
        assert_records_equal(gpu, ref, "sampled step %d" % ctl.k)
        seen["levels"] = max(seen["levels"], len(prob["level_sizes"]))
        seen["exhausted"] += int(np.sum(np.asarray(gpu["status"]) != 0))
        return [info_from_record(gpu[i], options.Hp) for i in range(len(gpu))]

    states = []
    for _ in range(n_steps):
        ctl.step(plan_step=plan_step)
        states.append([(m.x, m.y) for m in ctl.meas])
    opt.handle.close()
    assert states[0] != states[-1]  # the vehicles moved
    return seen


def test_c2_like_steps():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32)
    sc = commonroad_scenario(options, seed=1)
    seen = closed_loop(options, sc, "distance", 10, boundary_provider(sc))
    assert seen["levels"] > 1


def test_circle_full_coupling_deep_chain():
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=8, Hp=6, max_vehicles=8)
    seen = closed_loop(options, circle_scenario(options), "full", 6)
    assert seen["levels"] == 8


def test_triple_speed_steps():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=10, Hp=6, mpa_type=MpaType.triple_speed, max_vehicles=16)
    sc = commonroad_scenario(options, seed=2)
    closed_loop(options, sc, "distance", 5, boundary_provider(sc))


def test_exhausted_predecessor_hands_its_fallback_to_its_successors():
    """Slot 0 is boxed in by an obstacle (every edge collides: exhausted); its fallback areas lie across the others' way.  Its record
    carries them, and every successor plans against them on the device like the reference does on the host."""
    from pdmpc.backend import Handle
    from pdmpc.reference_trajectory import get_occupied_areas
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=6, Hp=6, max_vehicles=8)
    mpa = get_mpa(options)
    sc = circle_scenario(options)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="full")
    ctl.k = 3
    prob = ctl.build_step_problem()
    it0 = copy.copy(prob["iters"][0])
    x, y = float(it0.x0[0]), float(it0.x0[1])
    box = np.array([[x - 0.8, x + 0.8, x + 0.8, x - 0.8, x - 0.8], [y - 0.8, y - 0.8, y + 0.8, y + 0.8, y - 0.8]])
    it0.obstacles = list(it0.obstacles) + [box]
    prob["iters"][0] = it0
    veh = sc.vehicles[0]
    x1, y1, yaw1 = (float(v) for v in prob["iters"][1].x0[:3])
    _, rect = get_occupied_areas(x1 + veh.Length * np.cos(yaw1), y1 + veh.Length * np.sin(yaw1), yaw1, veh.Length, 2 * veh.Width, options.offset)
    prob["fallback"][0] = [np.asarray(rect, dtype=np.float64) for _ in range(options.Hp)]  # right in front of slot 1
    seeds = ref_step.step_seeds(prob, ctl.k)
    h = Handle(options)
    h.upload_mpa(mpa)
    gpu = h.plan_step_sampled(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]], seeds)
    one_launch(h)
    ref = ref_step.plan_step_sampled(options, mpa, prob, seeds)
    assert_records_equal(gpu, ref, "exhausted predecessor")
    assert int(gpu[0]["status"]) == 1
    assert list(gpu[0]["shape_cols"][: options.Hp]) == [rect.shape[1]] * options.Hp
    # without the fallback areas the successors plan otherwise: the hand-over is what the records above show
    prob["fallback"][0] = None
    other = h.plan_step_sampled(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]], seeds)
    assert not all(np.array_equal(other[s]["tree_path"], gpu[s]["tree_path"]) for s in range(1, len(gpu)))
    h.close()


@pytest.mark.parametrize("Hp", [6, 16])
def test_device_generator_matches_mt19937ar(Hp):
    from oracle import oracle
    from pdmpc.backend import Handle

    options = Config(scenario_type=ScenarioType.circle, amount=2, Hp=6, max_vehicles=4)
    h = Handle(options)
    seeds = [0, 1, 7, 31, 12345, 4294967295]
    got = h.debug_random_numbers(seeds, Hp * 250)
    for i, s in enumerate(seeds):
        want = oracle.mt19937_doubles(s if s else 5489, Hp * 250)  # (Seed = 0 is MATLAB's default seed 5489, mt19937ar.hpp)
        assert np.array_equal(got[i].view(np.uint64), want.view(np.uint64)), s
    # (and the argument checks that need a live handle: NULL seeds with vehicles to plan)
    import ctypes as C

    from pdmpc import abi

    vin, out = (abi.VehicleIn * 1)(), (abi.VehicleOut * 1)()
    assert h.L.pdmpc_plan_step_sampled(h.h, 1, vin, None, None, None, None, out) == -1
    assert h.L.pdmpc_set_step_seeds(h.h, 1, None) == -1
    h.close()


def test_oversubscribed_colouring_step_of_512_vehicles():
    from pdmpc.optimizer import MonteCarloTreeSearchHip
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=512, Hp=8, max_vehicles=512, max_nodes=1 << 12)
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=3, tiles=26)
    opt = MonteCarloTreeSearchHip(options)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc), priority_strategy="coloring")

    def plan_step(prob):
        gpu = opt.plan_step_records(prob, mpa)
        one_launch(opt.handle)
        ref = ref_step.plan_step_sampled(options, mpa, prob, ref_step.step_seeds(prob, ctl.k))
        assert_records_equal(gpu, ref, "512 vehicles")
        assert len(prob["level_sizes"]) > 1
        return [info_from_record(gpu[i], options.Hp) for i in range(len(gpu))]

    for _ in range(2):
        ctl.step(plan_step=plan_step)
    opt.handle.close()


def test_oversubscribed_explorative_batch():
    from pdmpc.explorative import explore_step
    from pdmpc.optimizer import MonteCarloTreeSearchHip
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    K = 52
    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=20 * K, max_nodes=1 << 12)
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=1)
    opt = MonteCarloTreeSearchHip(options)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))

    def plan_batch(batch):
        assert len(batch["iters"]) >= 1024
        gpu = opt.plan_step_records(batch, mpa)
        one_launch(opt.handle)
        ref = ref_step.plan_step_sampled(options, mpa, batch, ref_step.step_seeds(batch, ctl.k))
        assert_records_equal(gpu, ref, "explorative batch")
        return gpu

    for _ in range(2):
        explore_step(ctl, plan_batch, K)
    opt.handle.close()


def test_starved_predecessors_are_replanned_in_resident_slices(monkeypatch):
    """reverse_dispatch=1 hands the slots out in reverse: in a batch of 1 024 slots (128 instances of an 8-vehicle chain) the
    successors fill the chip and spin for predecessors that have not been dispatched.  The watchdog ends them (spin_limit), the
    step is planned again in resident slices, and the records are the reference's."""
    from pdmpc.explorative import explore_step
    from pdmpc.optimizer import MonteCarloTreeSearchHip
    from pdmpc.scenario import circle_scenario

    monkeypatch.setenv("PDMPC_TUNING", "reverse_dispatch=1,spin_limit=20000")
    K = 128
    options = Config(scenario_type=ScenarioType.circle, amount=8, Hp=6, max_vehicles=8 * K, max_nodes=1 << 12)
    mpa = get_mpa(options)
    opt = MonteCarloTreeSearchHip(options)
    ctl = PrioritizedSequentialController(options, circle_scenario(options), mpa, None, coupling="full")

    def plan_batch(batch):
        gpu = opt.plan_step_records(batch, mpa)
        ref = ref_step.plan_step_sampled(options, mpa, batch, ref_step.step_seeds(batch, ctl.k))
        assert_records_equal(gpu, ref, "after the safe re-plan")
        return gpu

    explore_step(ctl, plan_batch, K)
    st = opt.handle.stats()
    assert st["safe_replans"] >= 1 and st["kernel"] == 3
    before = st["safe_replans"]
    opt.handle.set_safe_launch(True)
    explore_step(ctl, plan_batch, K)
    assert opt.handle.stats()["safe_replans"] == before
    opt.handle.close()


def test_native_controller_with_the_sampled_optimizer():
    """pdmpc_controller_step / _explore_step / _optimal_step with PDMPC_OPTIMIZER_SAMPLED on the device against the Python twins
    driven by the reference."""
    from pdmpc.backend import Handle
    from pdmpc.explorative import explore_step
    from pdmpc.native_controller import NativeController
    from pdmpc.optimal import optimal_step
    from pdmpc.road_network import boundary_provider, commonroad_scenario
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=80)
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=1)
    h = Handle(options)
    h.upload_mpa(mpa)
    nat = NativeController(options, sc, mpa, h, coupling="distance", optimizer="sampled")
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))

    def plan_step(prob):
        ref = ref_step.plan_step_sampled(options, mpa, prob, ref_step.step_seeds(prob, py.k))
        return [info_from_record(ref[i], options.Hp) for i in range(len(ref))]

    def plan_batch(batch):
        return ref_step.plan_step_sampled(options, mpa, batch, ref_step.step_seeds(batch, py.k))

    for k in range(20):
        recs = nat.step()
        assert h.stats()["kernel"] == 3
        py.step(plan_step=plan_step)
        st = nat.state()
        assert np.array_equal(st["x"], np.array([m.x for m in py.meas])) and np.array_equal(st["y"], np.array([m.y for m in py.meas])), k
        assert np.array_equal(st["yaw"], np.array([m.yaw for m in py.meas])), k
    _, chosen_nat = nat.explore_step(4)
    _, _, chosen = explore_step(py, plan_batch, 4)
    assert list(chosen_nat) == chosen
    nat.close()
    h.close()

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=6, max_vehicles=4 * 24)
    mpa = get_mpa(options)
    sc = circle_scenario(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    nat = NativeController(options, sc, mpa, h, coupling="full", optimizer="sampled")
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="full")
    for _ in range(2):
        _, chosen_nat = nat.optimal_step(24)
        _, _, chosen = optimal_step(py, plan_batch, 24)
        assert list(chosen_nat) == chosen
        st = nat.state()
        assert np.array_equal(st["x"], np.array([m.x for m in py.meas])) and np.array_equal(st["yaw"], np.array([m.yaw for m in py.meas]))
    nat.close()
    h.close()


def test_matlab_shaped_entry_equals_the_c_entry():
    """pdmpc_ml_plan_step_sampled (what the MEX command `plan_step_sampled` calls) fed with MATLAB-shaped data in VEHICLE order equals
    pdmpc_plan_step_sampled."""
    import ctypes as C

    import matlab_shapes as ms
    from pdmpc import abi
    from pdmpc.backend import Handle
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32)
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=4)
    h = Handle(options)
    h.upload_mpa(mpa)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    L = ms.lib()
    L.pdmpc_ml_plan_step_sampled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(abi.VehicleOut)]
    L.pdmpc_ml_plan_step_sampled.restype = C.c_int

    def plan_step(prob):
        n = len(prob["iters"])
        seeds = ref_step.step_seeds(prob, ctl.k)
        keep = ms.Keep()
        step = ms.step_create(ms.vehicle_order_problem(prob), options.Hp, keep)
        by_vehicle = abi.out_array(n)
        sd = (C.c_uint32 * n)(*[ctl.k + v + 1 for v in range(n)])
        assert L.pdmpc_ml_plan_step_sampled(h.h, step, sd, abi.out_ptr(by_vehicle)) == 0
        L.pdmpc_ml_step_destroy(step)
        gpu = h.plan_step_sampled(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]], seeds)
        assert_records_equal(by_vehicle[np.asarray(prob["order"])], gpu, "matlab-shaped sampled step")
        return [info_from_record(gpu[i], options.Hp) for i in range(n)]

    for _ in range(4):
        ctl.step(plan_step=plan_step)
    h.close()
