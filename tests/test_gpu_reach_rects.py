"""The oriented reach rule of the graph search (include/pdmpc_reach.h) on the device: the step problems of
test_gpu_reach_lists.py turned to a root yaw other than zero, with obstacle segments just inside and just outside a step's
rectangle in front of and beside the vehicle, a segment directly behind it (inside the square of the disc bound, outside the
rectangle), and predecessors whose solved areas lie behind the follower or ahead of it -- records byte for byte the oracle's,
through the product, the generic and the compact instantiation and with the wide kernel's automaton."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from pdmpc import abi, backend

import test_gpu_reach_lists as base

pytestmark = pytest.mark.gpu

SHIFT = (2.25, -1.5)
MARGIN = 2.0 ** -20
DP, IP = abi.c_double_p, abi.c_int32_p


def rects_of(mpa, Hp):
    s, keep = abi.pack_mpa(mpa)
    out = np.zeros((mpa.n_trims, Hp, 4))
    assert backend.load_library().pdmpc_mpa_reach_rects_host(C.byref(s), Hp, out.ctypes.data_as(DP)) == 0
    del keep
    return out


def widened(rect, rx, ry):
    m = MARGIN * (1.0 + abs(rx) + abs(ry) + float(np.max(np.abs(rect))))
    return rect[0] - m, rect[1] + m, rect[2] - m, rect[3] + m


def placed(p, yaw):
    """Points (2, n) given in the frame of a vehicle at the origin heading along +x, where the turned and shifted vehicle sees them."""
    p = np.asarray(p, dtype=np.float64)
    c, s = math.cos(yaw), math.sin(yaw)
    return np.vstack([c * p[0] - s * p[1] + SHIFT[0], s * p[0] + c * p[1] + SHIFT[1]])


def turned(v, yaw):
    """A vehicle of test_gpu_reach_lists.py (built around the x axis) with everything it sees turned by yaw about the origin and shifted."""
    v = copy.copy(v)
    at = placed(np.array([[v.x0[0]], [v.x0[1]]]), yaw)
    v.x0 = np.array([at[0, 0], at[1, 0], v.x0[2] + yaw, v.x0[3]])
    v.reference_trajectory_points = placed(np.asarray(v.reference_trajectory_points).T, yaw).T.copy()
    v.predicted_lanelet_boundary = tuple(None if b is None else placed(b, yaw) for b in v.predicted_lanelet_boundary)
    v.obstacles = [placed(o, yaw) for o in v.obstacles]
    v.dynamic_obstacle_area = [[placed(a, yaw) for a in d] for d in v.dynamic_obstacle_area]
    return v


def turned_problem(iters, preds, fallback, yaw):
    fb = [None if f is None else [placed(a, yaw) for a in f] for f in fallback]
    return base.step_problem([turned(v, yaw) for v in iters], preds, fb)


def listed_at(mpa, Hp, rects, root, seg, k):
    """Whether the host twin lists the segment (2, 2) for step k of the search rooted at `root`."""
    x, y = np.ascontiguousarray(seg[0]), np.ascontiguousarray(seg[1])
    first = np.zeros(Hp, dtype=np.int32)
    count = np.array([2 if q == k else 0 for q in range(1, Hp + 1)], dtype=np.int32)
    lo, lst = np.zeros(Hp + 1, dtype=np.int32), np.zeros(2, dtype=np.int32)
    rc = backend.load_library().pdmpc_reach_lists_oriented_host(Hp, mpa.n_trims, rects.ctypes.data_as(DP), int(root.trim_index), float(root.x0[0]), float(root.x0[1]), float(root.x0[2]),
                                                                x.ctypes.data_as(DP), y.ctypes.data_as(DP), first.ctypes.data_as(IP), count.ctypes.data_as(IP), lo.ctypes.data_as(IP), lst.ctypes.data_as(IP))
    assert rc == 0
    return int(lo[Hp]) == 1


@pytest.mark.parametrize("variant,Hp", base.CASES)
def test_segments_at_the_sides_of_a_steps_rectangle_and_behind_the_vehicle(variant, Hp, monkeypatch, capfd):
    """Root yaw pi/4 and -2.0, a straight corridor along the heading.  For k = 1, 2, Hp: a segment across the lane 1e-9 m inside the front
    side of step k's widened rectangle and one along the lane 1e-9 m inside its left side; the same 1e-9 m outside (for k = Hp those
    are beyond every step's reach: the obstacle-free plan); and a segment across the lane directly behind the vehicle, within the
    square of the disc bound and outside every rectangle: the obstacle-free plan again."""
    options, mpa = base.setup(variant, Hp, monkeypatch)
    rects = rects_of(mpa, Hp)
    dmax, amax = base.reach(mpa)
    for yaw in (math.pi / 4, -2.0):
        plain = base.vehicle(options, mpa)
        root = turned(plain, yaw)
        rect = rects[plain.trim_index - 1]
        free, _ = base.plan(options, mpa, base.step_problem([root], [[]]), "no obstacle")
        for k in sorted({1, 2, Hp}):
            x_lo, x_hi, y_lo, y_hi = widened(rect[k - 1], root.x0[0], root.x0[1])
            mid = 0.5 * (x_lo + x_hi)
            for d, inside in ((-1e-9, True), (1e-9, False)):
                front = placed(np.array([[x_hi + d, x_hi + d], [-0.2, 0.2]]), yaw)
                side = placed(np.array([[mid - 0.05, mid + 0.05], [y_hi + d, y_hi + d]]), yaw)
                assert listed_at(mpa, Hp, rects, root, front, k) == inside and listed_at(mpa, Hp, rects, root, side, k) == inside
                v = copy.copy(root)
                v.obstacles = [front, side]
                got, _ = base.plan(options, mpa, base.step_problem([v], [[]]), "yaw %g: segments %s step %d's rectangle" % (yaw, "inside" if inside else "outside", k))
                if k == Hp and not inside:
                    assert got.tobytes() == free.tobytes()
        behind = placed(np.array([[rect[:, 0].min() - 0.05, rect[:, 0].min() - 0.05], [-0.2, 0.2]]), yaw)
        assert abs(rect[:, 0].min() - 0.05) < amax  # (inside the square of step 1 already)
        assert not any(listed_at(mpa, Hp, rects, root, behind, k) for k in range(1, Hp + 1))
        v = copy.copy(root)
        v.obstacles = [behind]
        got, _ = base.plan(options, mpa, base.step_problem([v], [[]]), "yaw %g: a segment directly behind the vehicle" % yaw)
        assert got.tobytes() == free.tobytes()
    base.assert_kernel(capfd, variant)


@pytest.mark.parametrize("variant,Hp", base.CASES)
def test_predecessor_areas_behind_and_ahead_of_the_follower(variant, Hp, monkeypatch, capfd):
    yaw = math.pi / 4
    options, mpa = base.setup(variant, Hp, monkeypatch)
    follower = base.vehicle(options, mpa)
    ahead_x = base.AHEAD[options.mpa_type][0]
    behind = base.standing(options, mpa, -0.45, 0.0)  # stands right behind the follower: in the square of steps 2 and later, in no rectangle
    ahead = base.blocked_ahead(options, mpa)  # in the follower's lane, just in front of it, and blocked: it brakes
    alone, _ = base.plan(options, mpa, turned_problem([follower], [[]], [None], yaw), "follower alone")
    # solved areas behind the follower, expected areas in its lane ahead: parked nodes come back, nothing is due for a re-check
    gpu, _ = base.plan(options, mpa, turned_problem([behind, follower], [[], [0]], [base.boxes(ahead_x, 0.0, Hp, 0.05), None], yaw), "solved behind, expected ahead")
    assert gpu[1:].tobytes() == alone.tobytes()
    # solved areas in the lane ahead, expected areas behind the follower: the arrival is marked, the follower yields
    gpu2, _ = base.plan(options, mpa, turned_problem([ahead, follower], [[], [0]], [base.boxes(-0.45, 0.0, Hp), None], yaw), "solved ahead, expected behind")
    if Hp > 2:  # (two steps are over before the follower gets anywhere near)
        assert gpu2[1:].tobytes() != alone.tobytes(), "the follower does not yield: the case tests nothing"
    base.assert_kernel(capfd, variant)


@pytest.mark.parametrize("variant", ["product", "generic"])
def test_helpers_rebuild_their_lists_on_an_arrival_turned(variant, monkeypatch, capfd):
    """test_helpers_rebuild_their_lists_on_an_arrival of test_gpu_reach_lists.py at root yaw pi/4: owner and helpers build their lists
    from the same root, and rebuild them when the predecessor arrives."""
    yaw = math.pi / 4
    Hp = base.VARIANTS[variant][1][-1]
    options, mpa = base.setup(variant, Hp, monkeypatch, "share_min=16,tile=16,round0=64")
    pred, heavy = base.helper_scenario(options, mpa)
    alone, _ = base.plan(options, mpa, turned_problem([heavy], [[]], [None], yaw), "the follower alone")
    gpu, stats = base.plan(options, mpa, turned_problem([pred, heavy], [[], [0]], [base.boxes(0.0, 80.0, Hp), None], yaw), "shared rounds with an arrival")
    assert gpu[1:].tobytes() != alone.tobytes(), "the predecessor's solved areas do not change the follower's plan: a stale list would go unnoticed"
    assert int(gpu[1]["n_expanded"]) > 10 * int(gpu[0]["n_expanded"])  # (the predecessor's search is by far the shorter one)
    assert stats["shared_rounds"] >= 2 and stats["helper_checked"] > 0 and stats["speculation_arrivals"] >= 1, stats
    base.assert_kernel(capfd, variant)
