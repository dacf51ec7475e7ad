"""Future collision assessment on the MI355X (csrc/fca_kernel.hip): the device counts equal the host twin's for
batches of every shape, the handle's buffers are reused from call to call, and the native controller with a handle (FCA on the device,
random priorities and random weights on the host, one search launch per step) drives the same closed loop as the Python controller
planned by the oracle."""
import copy
import math
import os

import numpy as np
import pytest

from pdmpc.backend import Handle, fca_collisions_host, fca_pairs
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import VEHICLE_LENGTH, VEHICLE_WIDTH, get_mpa

from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu


def _traffic(rng, n, Hp, side):
    refs = []
    for _ in range(n):
        x0, y0 = rng.uniform(0, side, 2)
        a = rng.uniform(-math.pi, math.pi)
        t = np.arange(Hp) * rng.uniform(0.02, 0.08)
        refs.append(np.stack([x0 + math.cos(a) * t, y0 + math.sin(a) * t], axis=1))
    return refs


def _box(rng, side, size):
    x, y = rng.uniform(0, side, 2)
    return np.array([[x, x + size, x + size, x], [y, y, y + size, y + size]])


def test_kernel_equals_host_twin_for_every_batch_shape():
    options = Config(scenario_type=ScenarioType.commonroad, Hp=10, mpa_type=MpaType.single_speed, max_vehicles=512)
    h = Handle(options)
    try:
        rng = np.random.default_rng(5)
        hits = 0
        for n, coupling, n_obst, n_rows in ((1, "none", 2, 1), (2, "full", 0, 0), (3, "none", 4, 2), (64, "full", 0, 0), (64, "full", 6, 2),
                                            (65, "distance", 3, 0), (256, "distance", 8, 3), (512, "distance", 0, 0), (512, "distance", 16, 4)):
            Hp = 10
            side = max(0.6, math.sqrt(n) * 0.35)
            refs = _traffic(rng, n, Hp, side)
            if coupling == "full":
                A = np.ones((n, n), dtype=np.int64) - np.eye(n, dtype=np.int64)
            elif coupling == "none":
                A = np.zeros((n, n), dtype=np.int64)
            else:
                p = np.array([r[0] for r in refs])
                A = (np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]) <= 0.8).astype(np.int64)
                np.fill_diagonal(A, 0)
            pairs = fca_pairs(A)
            obst = [_box(rng, side, 0.2) for _ in range(n_obst)]
            dyn = [[_box(rng, side, 0.1) for _ in range(Hp)] for _ in range(n_rows)]
            want, want_prio = fca_collisions_host(refs, pairs, VEHICLE_LENGTH, VEHICLE_WIDTH, 0.01, obst, dyn)
            got, prio = h.fca_collisions(refs, pairs, VEHICLE_LENGTH, VEHICLE_WIDTH, 0.01, obst, dyn)
            assert np.array_equal(got, want), (n, coupling, n_obst, n_rows)
            assert np.array_equal(prio, want_prio), (n, coupling)
            assert h.fca_kernel_ms() > 0.0
            again, prio2 = h.fca_collisions(refs, pairs, VEHICLE_LENGTH, VEHICLE_WIDTH, 0.01, obst, dyn)  # the same buffers, no clearing by the caller
            assert np.array_equal(again, got) and np.array_equal(prio2, prio)
            hits += int(got.sum())
        # an empty pair list after a full one: the counts are cleared on the device
        refs = _traffic(rng, 64, 10, 2.0)
        got, _ = h.fca_collisions(refs, np.zeros((0, 2), dtype=np.int32), VEHICLE_LENGTH, VEHICLE_WIDTH, 0.01)
        assert got.tolist() == [0] * 64
        assert hits > 0
    finally:
        h.close()


def _closed_loop(options, scenario, boundary, n_steps, **kw):
    """pdmpc_controller_step with a handle against the Python controller planned by the oracle: records of every step and the plant
    state after it are identical."""
    from oracle import oracle
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip

    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, scenario, mpa, opt.handle, coupling="distance", **kw)
    py = PrioritizedSequentialController(options, scenario, mpa, None, coupling="distance", boundary_provider=boundary, **kw)
    unbounded = copy.copy(options)
    unbounded.max_nodes = 1 << 30
    parallel = 0
    try:
        for k in range(n_steps):
            gpu = nat.step()
            ref_box = []

            def plan_step(prob):
                ref, _ = oracle.plan_step(unbounded, mpa, prob, n_threads=min(os.cpu_count() or 1, 16))
                ref_box.append(ref)
                return [info_from_record(ref[i], options.Hp) for i in range(len(ref))]

            py.step(plan_step=plan_step)
            assert_records_equal(gpu, ref_box[0], "native step %d" % (k + 1))
            parallel += int(np.sum(np.asarray(py.last_directed) != np.asarray(py.last_directed_seq)))
            st = nat.state()
            assert np.array_equal(st["x"], np.array([m.x for m in py.meas])) and np.array_equal(st["y"], np.array([m.y for m in py.meas])), k
            assert np.array_equal(st["yaw"], np.array([m.yaw for m in py.meas])), k
            assert np.array_equal(st["speed"], np.array([m.speed for m in py.meas])), k
            assert st["needs_fallback"].tolist() == [bool(i.needs_fallback) for i in py.infos], k
    finally:
        nat.close()
        opt.handle.close()
    return py, parallel


@pytest.mark.parametrize("strategy", ["fca", "random"])
def test_c2_like_closed_loop_on_device(strategy):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=6, max_vehicles=32, max_nodes=1 << 17)
    sc = commonroad_scenario(options, seed=1)
    py, _ = _closed_loop(options, sc, boundary_provider(sc), 8, priority_strategy=strategy)
    assert py.last_adjacency.sum() > 0


@pytest.mark.parametrize("strategy", ["fca", "random"])
def test_c3_like_closed_loop_cut_to_two_levels_with_random_weights_on_device(strategy):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=5, max_num_CLs=2, max_vehicles=64, max_nodes=1 << 17)
    sc = commonroad_scenario(options, seed=2, tiles=2)
    py, parallel = _closed_loop(options, sc, boundary_provider(sc), 6, priority_strategy=strategy, weight_strategy="random")
    assert int(py.last_levels.max()) <= 2
    assert parallel > 0, "no coupling was cut"
