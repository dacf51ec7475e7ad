"""The reachable-set coupler on the MI355X (csrc/reachable_kernel.hip): adjacency and area bits equal the host
twin's for batches of every shape, and the native controller with a handle (coupling on the device, one launch per step) drives the
same closed loop as the Python controller planned by the oracle, with parallel predecessors as reachable sets."""
import copy
import math
import os

import numpy as np
import pytest

from pdmpc import reachability as R
from pdmpc.backend import Handle, reachable_set_coupling_call
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa

from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_kernel_equals_host_twin_for_every_batch_shape():
    options = Config(scenario_type=ScenarioType.commonroad, Hp=8, mpa_type=MpaType.single_speed, max_vehicles=512)
    mpa = get_mpa(options)
    L = mpa.local_reachable_sets_conv
    h = Handle(options)
    try:
        h.upload_reachable_sets(L)
        rng = np.random.default_rng(11)
        coupled = 0
        for n in (1, 2, 63, 64, 65, 256, 512):
            side = max(1.0, math.sqrt(n) * 0.6)  # about as dense as a tile of the road network
            x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
            yaw = rng.uniform(-math.pi, math.pi, n)
            trim = rng.integers(1, mpa.n_trims + 1, n)
            if n >= 3:
                yaw[0] = 0.0
                x[1], y[1], yaw[1], trim[1] = x[0], y[0], yaw[0], trim[0]  # identical poses
                a = R.reachable_sets_at_pose(L, x[0], y[0], 0.0, int(trim[0]))[-1]
                x[2], y[2], yaw[2], trim[2] = x[0] + (a[0].max() - a[0].min()), y[0], 0.0, trim[0]  # boxes that (about) touch
            if n >= 4:
                x[3], y[3] = x[0] + 100.0, y[0]  # far apart
            adj_d, area_d = h.reachable_set_coupling(x, y, yaw, trim)
            adj_h, area_h = reachable_set_coupling_call(L, x, y, yaw, trim)
            assert np.array_equal(adj_d, adj_h), n
            assert np.array_equal(_bits(area_d), _bits(area_h)), n
            assert not adj_d.diagonal().any() and np.array_equal(adj_d, adj_d.T)
            if n >= 3:
                assert adj_d[0, 1] == 1 and adj_d[0, 2] == 0
            coupled += int(adj_d.sum())
            assert h.reachable_set_coupling_kernel_ms() > 0.0
        assert coupled > 0
    finally:
        h.close()


def _closed_loop(options, scenario, boundary, n_steps, **kw):
    """pdmpc_controller_step with a handle (coupling kernel + one search launch per step) against the Python controller planned by
    the oracle: records of every step and the plant state after it are identical."""
    from oracle import oracle
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip

    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, scenario, mpa, opt.handle, coupling="reachable_set", **kw)
    py = PrioritizedSequentialController(options, scenario, mpa, None, coupling="reachable_set", boundary_provider=boundary, **kw)
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


def test_c2_like_closed_loop_with_reachable_sets_on_device():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=6, max_vehicles=32, max_nodes=1 << 17, is_deal_prediction_inconsistency=True)
    sc = commonroad_scenario(options, seed=1)
    py, _ = _closed_loop(options, sc, boundary_provider(sc), 10)
    assert py.last_adjacency.sum() > 0


def test_c3_like_closed_loop_cut_to_two_levels_on_device():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=5, max_num_CLs=2, max_vehicles=64, max_nodes=1 << 17,
                     is_deal_prediction_inconsistency=True)
    sc = commonroad_scenario(options, seed=2, tiles=2)
    _, parallel = _closed_loop(options, sc, boundary_provider(sc), 10, priority_strategy="coloring")
    assert parallel > 0, "no parallel coupling in ten steps"


def test_circle_closed_loop_on_the_sat_checker():
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 17, is_deal_prediction_inconsistency=True)
    py, _ = _closed_loop(options, circle_scenario(options), None, 10)
    assert py.last_adjacency.sum() > 0
