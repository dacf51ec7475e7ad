"""Shared cases of the centralized-control tests (tests/test_native_centralized.py, tests/test_gpu_centralized.py): scenarios, the
comparison of a native joint problem with the twin's, and reference closed loops that are computed once per session."""
import functools
import math

import numpy as np

from pdmpc import abi
from pdmpc.centralized import CentralizedController, centralized_mpa, centralized_options
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.iteration_data import info_from_record
from pdmpc.native_controller import NativeController
from pdmpc.scenario import Scenario, Vehicle

import joint_reference as jr


def circle_options(N, Hp, **kw):
    return centralized_options(Config(scenario_type=ScenarioType.circle, amount=N, Hp=Hp, mpa_type=MpaType.single_speed, T_end=4, max_vehicles=16, **kw))


def rotated_circle(options, angle=0.0, obstacles=()):
    """Circle.m's layout (pdmpc.scenario.circle_scenario) turned by `angle` about the circle's centre, with static obstacles."""
    n, radius = options.amount, 2
    speed = max(centralized_mpa(options).get_straight_speeds_of_mpa())
    vehicles = []
    for i in range(n):
        yaw = math.pi * 2 / n * i + angle
        s, c = math.sin(yaw), math.cos(yaw)
        x0, y0 = -c * radius + 2.25, -s * radius + 2
        vehicles.append(Vehicle(x_start=x0, y_start=y0, yaw_start=yaw, reference_path=np.array([[x0, y0], [x0 + c * 2 * radius, y0 + s * 2 * radius]]), reference_speed=speed))
    return Scenario(vehicles=vehicles, obstacles=list(obstacles))


def rectangle(cx, cy, w=0.2, h=0.1):
    return np.array([[cx - w, cx + w, cx + w, cx - w], [cy - h, cy - h, cy + h, cy + h]])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_same_iters(got, want, ctx):
    """A native joint problem against the twin's build_iters, bit for bit: pose, trim, reference points, v_ref, boundaries, obstacles."""
    assert len(got) == len(want), ctx
    for v, (a, b) in enumerate(zip(got, want)):
        where = "%s vehicle %d" % (ctx, v)
        assert np.array_equal(bits(a.x0[:3]), bits(b.x0[:3])), where
        assert a.trim_index == b.trim_index, where
        assert np.array_equal(bits(a.reference_trajectory_points), bits(b.reference_trajectory_points)), where
        assert np.array_equal(bits(a.v_ref), bits(b.v_ref)), where
        for side in (0, 1):
            x, y = a.predicted_lanelet_boundary[side], b.predicted_lanelet_boundary[side]
            assert (x is None or np.size(x) == 0) == (y is None or np.size(y) == 0), where
            if x is not None and np.size(x):
                assert np.array_equal(bits(x), bits(y)), where
        assert len(a.obstacles) == len(b.obstacles) and all(np.array_equal(bits(p), bits(q)) for p, q in zip(a.obstacles, b.obstacles)), where
        assert len(a.dynamic_obstacle_area) == 0 and len(b.dynamic_obstacle_area) == 0, where


def state_of_twin(ctl):
    return {name: np.array([getattr(m, name) for m in ctl.meas]) for name in ("x", "y", "yaw", "speed", "steering")}


def assert_same_state(st, want, k, ctx=""):
    for name in ("x", "y", "yaw", "speed", "steering"):
        assert np.array_equal(bits(st[name]), bits(want[name])), "%s %s" % (ctx, name)
    assert st["k"] == k, ctx
    assert not st["needs_fallback"].any(), ctx


def assert_same_native_state(a, b, ctx=""):
    """two native controllers byte for byte where pdmpc_controller_state can see"""
    sa, sb = a.state(), b.state()
    assert_same_state(sa, sb, sb["k"], ctx)


@functools.lru_cache(maxsize=None)
def reference_loop(N, Hp, steps, angle=0.0):
    """The reference's closed loop (CentralizedController around joint_reference.plan_joint) on the circle turned by `angle`: the
    records of every step.  Computed once per session and shared; callers must not write into it."""
    options = circle_options(N, Hp)
    mpa = centralized_mpa(options)
    recs = []

    def plan(iters):
        recs.append(jr.plan_joint(options, mpa, [iters]))
        return [info_from_record(r, Hp) for r in recs[-1]]

    ctl = CentralizedController(options, rotated_circle(options, angle), mpa, plan)
    for _ in range(steps):
        ctl.step()
    return tuple(recs)


def moving_start_records(options, scenario, mpa):
    """Records that put every vehicle of `scenario` one maneuver ahead of its start, straight on at the fastest trim its standstill
    trim reaches: a moving start without a search (what an apply reads of a record: y_predicted(:, 1) and predicted_trims(1))."""
    n = len(scenario.vehicles)
    recs = abi.out_array(n)[:n]
    t0 = mpa.trim_from_values(0.0, 0.0) - 1
    succ = [j for j in range(mpa.n_trims) if mpa.transition_matrix_single[t0, j, 0] and mpa.maneuvers[t0][j] is not None]
    j = max(succ, key=lambda q: (mpa.trims[q].steering == 0, mpa.trims[q].speed))
    assert mpa.trims[j].speed > 0
    m = mpa.maneuvers[t0][j]
    for v, veh in enumerate(scenario.vehicles):
        c, s = math.cos(veh.yaw_start), math.sin(veh.yaw_start)
        recs["y_predicted"][v][0] = [veh.x_start + c * m.dx - s * m.dy, veh.y_start + s * m.dx + c * m.dy, veh.yaw_start + m.dyaw]
        recs["predicted_trims"][v][0] = j + 1
    return recs


def native_on_circle(N, Hp, angle=0.0, handle=None, obstacles=(), moving=False):
    """A native controller on the circle turned by `angle`; moving: one centralized step taken with moving_start_records (no GPU),
    so that it joins a test from a moving start."""
    options = circle_options(N, Hp)
    mpa = centralized_mpa(options)
    sc = rotated_circle(options, angle, obstacles)
    nat = NativeController(options, sc, mpa, handle, coupling="none")
    if moving:
        nat.centralized_build()
        nat.centralized_apply(moving_start_records(options, sc, mpa))
    return nat


def twin_iters_from_a_moving_start(N, Hp, angle=0.0):
    """(options, mpa, build_iters of the twin) on the circle after one step with moving_start_records."""
    from pdmpc.controller import Measurement

    options = circle_options(N, Hp)
    mpa = centralized_mpa(options)
    sc = rotated_circle(options, angle)
    ctl = CentralizedController(options, sc, mpa, None)
    recs = moving_start_records(options, sc, mpa)
    ctl.k = 1
    for v in range(N):
        t = mpa.trims[int(recs["predicted_trims"][v][0]) - 1]
        ctl.meas[v] = Measurement(*[float(q) for q in recs["y_predicted"][v][0]], t.speed, t.steering)
    return options, mpa, ctl.build_iters()


JOINT_PASSES = ((64 * 1024, True), (64 * 1024, False), (160 * 1024, True), (160 * 1024, False))  # layout_joint's (budget, areas in LDS)


def joint_soup_capacity(mpa, Hp, budget=160 * 1024, areas_in_lds=False):
    """The soup columns (16 bytes each) layout_joint can give a problem in one of its passes (JOINT_PASSES; the default: the last one,
    which takes the whole 160 KB of LDS and leaves the automaton's areas in L2): the budget less the automaton's tables, the
    per-vehicle references, the node's areas, the offsets, the successor lists and the smallest open list (256 entries of 12
    bytes).  A launch's soup_cap is the soup columns of its largest problem (pdmpc_joint_soup_columns) and two more."""
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    n = mpa.n_trims
    n_man = sum(1 for row in mpa.maneuvers for m in row if m is not None)
    off = a16(Hp * n * ((n + 63) // 64) * 8)
    off = a16(off + n * n * 2)
    off = a16(off + n_man * 32)
    if areas_in_lds:
        off = a16(off + n_man * 3 * abi.VMAX * 16)
    off += abi.JOINT_MAX * 3 * abi.HP_MAX * 8 + abi.JOINT_MAX * 2 * abi.VMAX * 16
    off = a16(off + (abi.JOINT_MAX * (abi.HP_MAX + 1) + 3 * abi.JOINT_MAX + abi.HP_MAX + 1) * 4)
    off = a16(off + abi.JOINT_MAX * n * 4)
    return (budget - 256 * 12 - off) // 16


def far_rectangles(count):
    """`count` convex rectangles in rows far from the circle (which lies within [0, 4.5] x [0, 4])"""
    return [rectangle(20.0 + 0.5 * (q % 40), 20.0 + 0.3 * (q // 40), 0.2, 0.1) for q in range(count)]


def exhausted(recs):
    out = recs.copy()
    out["status"] = abi.EXHAUSTED
    return out
