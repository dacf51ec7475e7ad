"""Lanelet bounding and the coupler on the bounded sets on the MI355X (csrc/bounded_kernel.hip): the device's bounded
sets, flags, adjacency and area bits equal the host twin's for batches of every shape; limits return PDMPC_ERR_CAPACITY and leave the
handle working; the native controller with a handle (bounding and coupling on the device, one search launch per step) drives the same
closed loop as the Python controller planned by the oracle; an explorative step builds the same problem on the device as on the host."""
import math

import numpy as np
import pytest

from pdmpc import reachability as R
from pdmpc.backend import BackendError, Handle, bound_reachable_sets_call, polygon_set_coupling_call
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.mpa import get_mpa

from test_gpu_reachable_coupling import _closed_loop

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _lanelet_polygons(seed=1):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    o = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8)
    sc = commonroad_scenario(o, seed=seed)
    py = PrioritizedSequentialController(o, sc, get_mpa(o), None, coupling="reachable_set", boundary_provider=boundary_provider(sc))
    py._traffic_info()
    return [R.lanelet_polygon(*b) for b in py.boundary], py


def _batch(rng, polys, n, n_trims):
    lan = [polys[i % len(polys)] for i in range(n)]
    x, y = np.zeros(n), np.zeros(n)
    for i in range(n):
        p = lan[i][:, rng.integers(lan[i].shape[1])]
        x[i], y[i] = p + rng.normal(0.0, 0.15, 2)
    yaw = rng.uniform(-math.pi, math.pi, n)
    trim = rng.integers(1, n_trims + 1, n)
    if n >= 2:
        lan[1] = None  # not bounded
    return x, y, yaw, trim, lan


def _same_sets(a, fa, b, fb):
    assert np.array_equal(fa, fb)
    for v in range(len(a)):
        for q in range(len(a[v])):
            assert a[v][q].shape == b[v][q].shape and np.array_equal(_bits(a[v][q]), _bits(b[v][q])), (v, q)


@pytest.mark.parametrize("Hp", [8, 10])
def test_device_equals_host_twin_for_every_batch_shape(Hp):
    options = Config(scenario_type=ScenarioType.commonroad, Hp=Hp, mpa_type=MpaType.single_speed, max_vehicles=512)
    mpa = get_mpa(options)
    L = mpa.local_reachable_sets_conv
    polys, _ = _lanelet_polygons()
    h = Handle(options)
    try:
        h.upload_reachable_sets(L)
        rng = np.random.default_rng(Hp)
        coupled = 0
        for n in (1, 2, 63, 64, 65, 256, 512):
            x, y, yaw, trim, lan = _batch(rng, polys, n, mpa.n_trims)
            for all_steps in (0, 1):
                dev, fd = h.bound_reachable_sets(x, y, yaw, trim, lan, all_steps)
                host, fh = bound_reachable_sets_call(L, x, y, yaw, trim, lan, all_steps)
                _same_sets(dev, fd, host, fh)
                adj_d, area_d = h.bounded_set_coupling()
                adj_h, area_h = polygon_set_coupling_call([s[-1] for s in host])
                assert np.array_equal(adj_d, adj_h), (n, all_steps)
                assert np.array_equal(_bits(area_d), _bits(area_h)), (n, all_steps)
                assert not adj_d.diagonal().any() and np.array_equal(adj_d, adj_d.T)
                coupled += int(adj_d.sum())
                t_bound, t_couple = h.bounded_reachable_kernel_ms()
                assert t_bound > 0.0 and (n < 2 or t_couple > 0.0)
        assert coupled > 0
        # a small ungrouped coupler call directly behind a larger grouped one (both stage through one body): nothing of the larger
        # call's group table is read
        x, y, yaw, trim, lan = _batch(rng, polys, 65, mpa.n_trims)
        h.bound_reachable_sets(x, y, yaw, trim, lan, 0)
        assert sum(int(adj.sum()) for adj, _ in h.bounded_set_coupling_grouped([1, 0, 40, 24])) > 0
        for n in (3, 1):
            h.bound_reachable_sets(x[:n], y[:n], yaw[:n], trim[:n], lan[:n], 0)
            host, _ = bound_reachable_sets_call(L, x[:n], y[:n], yaw[:n], trim[:n], lan[:n], 0)
            adj_d, area_d = h.bounded_set_coupling()
            adj_h, area_h = polygon_set_coupling_call([s[-1] for s in host])
            assert np.array_equal(adj_d, adj_h) and np.array_equal(_bits(area_d), _bits(area_h)), n
    finally:
        h.close()


def test_device_equals_host_twin_on_closed_loop_states():
    from test_bounded_reachable_sets import _states
    from pdmpc.road_network import commonroad_scenario

    o = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, mpa_type=MpaType.single_speed, max_vehicles=32, max_nodes=1 << 20)
    mpa, states = _states(o, commonroad_scenario(o, seed=1), 3)
    h = Handle(o)
    try:
        h.upload_reachable_sets(mpa.local_reachable_sets_conv)
        for st in states:
            for all_steps in (0, 1):
                dev, fd = h.bound_reachable_sets(st["x"], st["y"], st["yaw"], st["trim"], st["lanelets"], all_steps)
                host, fh = bound_reachable_sets_call(mpa.local_reachable_sets_conv, st["x"], st["y"], st["yaw"], st["trim"], st["lanelets"], all_steps)
                _same_sets(dev, fd, host, fh)
                adj_d, area_d = h.bounded_set_coupling()
                adj_p, area_p = R.polygon_set_coupling([s[-1] for s in host])
                assert np.array_equal(adj_d, adj_p) and np.array_equal(_bits(area_d), _bits(area_p))
    finally:
        h.close()


def test_limits_return_capacity_and_the_handle_still_works():
    import ctypes as C

    from pdmpc import abi
    from pdmpc.backend import ERR_CAPACITY, _coupling_args, _pack_lanelet_polygons

    options = Config(scenario_type=ScenarioType.commonroad, Hp=8, max_vehicles=8)
    mpa = get_mpa(options)
    L = mpa.local_reachable_sets_conv
    polys, _ = _lanelet_polygons()
    rng = np.random.default_rng(3)
    x, y, yaw, trim, lan = _batch(rng, polys, 4, mpa.n_trims)
    h = Handle(options)
    try:
        h.upload_reachable_sets(L)
        big = list(lan)
        t = np.linspace(0.0, 2 * math.pi, 600, endpoint=False)[::-1]
        big[0] = np.array([x[0] + 3.0 * np.cos(t), y[0] + 3.0 * np.sin(t)])  # 600 vertices > PDMPC_LANELET_POLY_MAX_COLS
        with pytest.raises(BackendError, match="status -4|PDMPC_LANELET_POLY_MAX_COLS"):
            h.bound_reachable_sets(x, y, yaw, trim, big, 1)
        # a capacity too small: PDMPC_ERR_CAPACITY with offsets that size the second call
        xa, ya, c, s, tr = _coupling_args(x, y, yaw, trim)
        lp, keep = _pack_lanelet_polygons(lan)
        off = np.zeros(4 + 1, dtype=np.int32)
        bx = np.zeros(3)
        by = np.zeros(3)
        rc = h.L.pdmpc_bound_reachable_sets(h.h, 4, xa.ctypes.data_as(abi.c_double_p), ya.ctypes.data_as(abi.c_double_p), c.ctypes.data_as(abi.c_double_p),
                                            s.ctypes.data_as(abi.c_double_p), tr.ctypes.data_as(abi.c_int32_p), C.byref(lp), 0, 3,
                                            off.ctypes.data_as(abi.c_int32_p), bx.ctypes.data_as(abi.c_double_p), by.ctypes.data_as(abi.c_double_p), None)
        del keep
        assert rc == ERR_CAPACITY and off[-1] > 3
        dev, fd = h.bound_reachable_sets(x, y, yaw, trim, lan, 0)
        host, fh = bound_reachable_sets_call(L, x, y, yaw, trim, lan, 0)
        _same_sets(dev, fd, host, fh)
        assert sum(d[0].shape[1] for d in dev) == off[-1]
        adj_d, area_d = h.bounded_set_coupling()
        adj_h, area_h = polygon_set_coupling_call([s_[-1] for s_ in host])
        assert np.array_equal(adj_d, adj_h) and np.array_equal(_bits(area_d), _bits(area_h))
    finally:
        h.close()


def test_c2_like_closed_loop_with_bounding_on_device():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=6, max_vehicles=32, max_nodes=1 << 17, is_deal_prediction_inconsistency=True,
                     bound_reachable_sets=True)
    sc = commonroad_scenario(options, seed=1)
    py, _ = _closed_loop(options, sc, boundary_provider(sc), 10)
    assert py.reachable_sets_bounded and py.last_adjacency.sum() > 0


def test_c3_like_closed_loop_with_bounding_cut_to_two_levels_on_device():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=5, max_num_CLs=2, max_vehicles=64, max_nodes=1 << 17,
                     is_deal_prediction_inconsistency=True, bound_reachable_sets=True)
    sc = commonroad_scenario(options, seed=2, tiles=2)
    py, parallel = _closed_loop(options, sc, boundary_provider(sc), 10, priority_strategy="coloring")
    assert py.reachable_sets_bounded and parallel > 0


def test_circle_closed_loop_with_bounding_switched_on():
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 17, is_deal_prediction_inconsistency=True,
                     bound_reachable_sets=True)
    py, _ = _closed_loop(options, circle_scenario(options), None, 10)
    assert not py.reachable_sets_bounded and py.last_adjacency.sum() > 0


def test_explorative_step_with_bounding_on_device_equals_host_twin():
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip
    from pdmpc.road_network import commonroad_scenario
    from test_native_controller import assert_same_problem

    options = Config(scenario_type=ScenarioType.commonroad, amount=14, Hp=5, max_num_CLs=3, max_vehicles=64, max_nodes=1 << 17,
                     is_deal_prediction_inconsistency=True, bound_reachable_sets=True)
    sc = commonroad_scenario(options, seed=5)
    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    dev = NativeController(options, sc, mpa, opt.handle, coupling="reachable_set", priority_strategy="coloring")
    host = NativeController(options, sc, mpa, None, coupling="reachable_set", priority_strategy="coloring")
    try:
        dev.explore_build(4, seed=1)
        host.explore_build(4, seed=1)
        assert_same_problem(dev.explore_problem(), host.explore_problem(), "explorative step, device against host")
    finally:
        dev.close()
        host.close()
        opt.handle.close()
