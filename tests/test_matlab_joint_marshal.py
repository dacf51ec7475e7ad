"""The MATLAB boundary of centralized control (pdmpc_ml_joint_step_create / pdmpc_ml_plan_joint, include/pdmpc_matlab.h) without
MATLAB: the IterationData of all vehicles in MATLAB's shapes (N-row fields, an N x Hp x 2 column-major reference, an N x 2 boundary
cell, the shared obstacle cells) against the Python packing of the same vehicles (abi.pack_vehicles)."""
import ctypes as C

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.centralized import CentralizedController, centralized_mpa, centralized_options
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.scenario import circle_scenario

import matlab_shapes as ms

_dp = C.POINTER(C.c_double)


class MlJointIter(C.Structure):
    _fields_ = [("amount", C.c_int32), ("x0", ms.MlMatrix), ("trim_indices", ms.MlMatrix), ("reference_trajectory_points", _dp), ("v_ref", ms.MlMatrix),
                ("boundary_rows", C.c_int32), ("boundary_cols", C.c_int32), ("predicted_lanelet_boundary", C.POINTER(ms.MlMatrix)),
                ("n_obstacles", C.c_int32), ("obstacles", C.POINTER(ms.MlMatrix)), ("dyn_rows", C.c_int32), ("dyn_cols", C.c_int32),
                ("dynamic_obstacle_area", C.POINTER(ms.MlMatrix))]


def lib():
    L = ms.lib()
    L.pdmpc_ml_joint_step_create.argtypes = [C.c_int32, C.POINTER(MlJointIter), C.POINTER(C.c_void_p)]
    L.pdmpc_ml_plan_joint.argtypes = [C.c_void_p, C.c_int32, C.POINTER(MlJointIter), C.POINTER(abi.VehicleOut)]
    return L


def ml_joint_iter(iters, Hp, keep, boundaries=True):
    """IterationData with amount = N as pdmpc_joint_iter_struct.m hands it over: row v = vehicle v."""
    N = len(iters)
    s = MlJointIter()
    s.amount = N
    s.x0 = keep.matrix(np.array([np.asarray(it.x0, dtype=np.float64) for it in iters]))
    s.trim_indices = keep.matrix(np.array([[float(it.trim_index)] for it in iters]))
    ref = np.asfortranarray(np.array([np.asarray(it.reference_trajectory_points, dtype=np.float64) for it in iters]))  # N x Hp x 2
    keep.refs.append(ref)
    s.reference_trajectory_points = ref.ctypes.data_as(_dp)
    s.v_ref = keep.matrix(np.array([np.asarray(it.v_ref, dtype=np.float64) for it in iters]))
    if boundaries:
        s.boundary_rows, s.boundary_cols = N, 2
        s.predicted_lanelet_boundary = keep.cell([list(it.predicted_lanelet_boundary) for it in iters], N, 2)
    obst = iters[0].obstacles
    s.n_obstacles = len(obst)
    s.obstacles = keep.cell([[o] for o in obst], len(obst), 1)
    dyn = iters[0].dynamic_obstacle_area
    s.dyn_rows, s.dyn_cols = len(dyn), Hp
    s.dynamic_obstacle_area = keep.cell(dyn, len(dyn), Hp)
    return s


def _polys(ps):
    out = []
    for p in range(ps.n_polygons):
        a, b = ps.offset[p], ps.offset[p + 1]
        out.append([(ps.x[q], ps.y[q]) for q in range(a, b)])
    return out


def assert_vehicle_in_equal(got, want, Hp):
    assert (got.x0, got.y0, got.yaw0, got.trim0) == (want.x0, want.y0, want.yaw0, want.trim0)
    for name in ("ref_x", "ref_y", "v_ref"):
        assert [getattr(got, name)[k] for k in range(Hp)] == [getattr(want, name)[k] for k in range(Hp)], name
    for side in ("left", "right"):
        n = getattr(want, "n_" + side)
        assert getattr(got, "n_" + side) == n, side
        for c in ("_x", "_y"):
            assert [getattr(got, side + c)[q] for q in range(n)] == [getattr(want, side + c)[q] for q in range(n)], side + c
    for name in ("obstacles", "dynamic_obstacles", "hdv_reachable_sets"):
        assert _polys(getattr(got, name)) == _polys(getattr(want, name)), name


def commonroad_iters(N=3, Hp=5):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = centralized_options(Config(scenario_type=ScenarioType.commonroad, amount=N, Hp=Hp, mpa_type=MpaType.single_speed))
    sc = commonroad_scenario(options, seed=2)
    ctl = CentralizedController(options, sc, centralized_mpa(options), None, boundary_provider=boundary_provider(sc))
    iters = ctl.build_iters()
    # scenario obstacles, shared by every vehicle, as the reference's iter holds them once
    box = np.array([[1.0, 1.3, 1.3, 1.0], [1.0, 1.0, 1.2, 1.2]])
    dyn = [[box + 0.05 * k for k in range(Hp)], [box - 0.05 * k for k in range(Hp)]]
    for it in iters:
        it.obstacles = [box, box + 2.0]
        it.dynamic_obstacle_area = dyn
    return options, iters


def test_joint_iter_from_matlab_shapes_is_the_python_packing():
    options, iters = commonroad_iters()
    Hp = options.Hp
    assert all(it.predicted_lanelet_boundary[0] is not None for it in iters)
    keep = ms.Keep()
    J = ml_joint_iter(iters, Hp, keep)
    step = C.c_void_p()
    assert lib().pdmpc_ml_joint_step_create(Hp, C.byref(J), C.byref(step)) == 0, ms.lib().pdmpc_ml_last_error()
    n, vin, po, pi, fb, order, levels = ms.step_problem(step)
    want, keep_w = abi.pack_vehicles(iters, Hp)
    assert n == len(iters)
    for v in range(n):
        assert order[v] == v + 1 and levels[v] == 1 and po[v + 1] == po[v]
        assert_vehicle_in_equal(vin[v], want[v], Hp)
    ms.lib().pdmpc_ml_step_destroy(step)
    del keep_w


def test_joint_iter_without_boundaries_and_rejections():
    options = centralized_options(Config(scenario_type=ScenarioType.circle, amount=2, Hp=4, mpa_type=MpaType.single_speed))
    ctl = CentralizedController(options, circle_scenario(options), centralized_mpa(options), None)
    iters = ctl.build_iters()
    keep = ms.Keep()
    J = ml_joint_iter(iters, options.Hp, keep, boundaries=False)
    step = C.c_void_p()
    assert lib().pdmpc_ml_joint_step_create(options.Hp, C.byref(J), C.byref(step)) == 0
    n, vin, *_ = ms.step_problem(step)
    want, keep_w = abi.pack_vehicles(iters, options.Hp)
    for v in range(n):
        assert_vehicle_in_equal(vin[v], want[v], options.Hp)
    ms.lib().pdmpc_ml_step_destroy(step)
    # iter.amount outside 1 .. PDMPC_JOINT_MAX, and an N-row field of the wrong height
    five = ml_joint_iter(iters * 3, options.Hp, keep, boundaries=False)
    five.amount = 5
    assert lib().pdmpc_ml_joint_step_create(options.Hp, C.byref(five), C.byref(step)) == abi_invalid()
    bad = ml_joint_iter(iters, options.Hp, keep, boundaries=False)
    bad.v_ref = keep.matrix(np.zeros((1, options.Hp)))
    assert lib().pdmpc_ml_joint_step_create(options.Hp, C.byref(bad), C.byref(step)) == abi_invalid()
    del keep_w


def abi_invalid():
    return -1  # PDMPC_ERR_INVALID


@pytest.mark.gpu
def test_plan_joint_from_matlab_shapes_equals_the_python_entry_point():
    from pdmpc.backend import Handle

    options, iters = commonroad_iters(N=2, Hp=5)
    mpa = centralized_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    want = h.plan_joint([iters])
    keep = ms.Keep()
    J = ml_joint_iter(iters, options.Hp, keep)
    out = abi.out_array(len(iters))
    assert lib().pdmpc_ml_plan_joint(h.h, options.Hp, C.byref(J), abi.out_ptr(out)) == 0, ms.lib().pdmpc_ml_last_error()
    assert out[: len(iters)].tobytes() == want.tobytes()
    h.close()
