"""What the HDV tests share (tests/test_hdv_host.py, tests/test_gpu_hdv.py): the maps, the HDV automaton's local sets,
the traffic cases with the reason each is there, and the bit-for-bit comparison of two results."""
import math

import numpy as np

from pdmpc import hdv
from pdmpc import reachability as R
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.mpa import get_mpa

_SETS = {}


def local_sets(Hp):
    """the HDV automaton's local reachable sets: single_speed without the recursive-feasibility mask (ManualVehicle.m:20-27)"""
    if Hp not in _SETS:
        o = Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=Hp, mpa_type=MpaType.single_speed, recursive_feasibility=False)
        _SETS[Hp] = R.local_reachable_sets_conv(get_mpa(o))
    return _SETS[Hp]


def ngon_sets(m, Hp, radius=0.4):
    """one trim whose every step hull is a clockwise m-gon (m = 256: a hull at PDMPC_REACHABLE_MAX_COLS), growing with the step"""
    out = []
    for k in range(Hp):
        a = -2.0 * math.pi * (np.arange(m) + 0.25) / m
        r = radius * (1.0 + 0.25 * k)
        out.append(np.array([r * np.cos(a), r * np.sin(a)]))
    return [out]


def hand_map(width=0.5, related=True):
    """Three lanelets by hand: 1 runs from (0, 0) to (2, 0), 2 follows it to (4, 0), 3 comes up from (0, -1) and merges into 2 at
    (2, 0).  1 - 2 and 2 - 3 are longitudinal, 1 - 3 merging; related = False: a table without any relationship."""
    w = width / 2
    xs = (0.0, 1.0, 2.0)
    left = [[(x, w) for x in xs], [(x + 2.0, w) for x in xs], [(x, -1.0 + 0.5 * x + w) for x in xs]]
    right = [[(x, -w) for x in xs], [(x + 2.0, -w) for x in xs], [(x, -1.0 + 0.5 * x - w) for x in xs]]
    rel = np.zeros((3, 3), dtype=np.uint8)
    if related:
        rel[0, 1], rel[1, 2], rel[0, 2] = hdv.LONGITUDINAL, hdv.LONGITUDINAL, hdv.MERGING
    return hdv.HdvMap(left, right, [[2], [], [2]], rel)


def u_map():
    """One lanelet without successor that runs right along y = 0, turns and comes back along y = 1 (0.3 wide): a set that covers both
    arms but not the turn meets it in two regions (PDMPC_BOUND_MULTIPLE)."""
    left = [(0.0, 0.15), (1.0, 0.15), (1.85, 0.15), (1.85, 0.85), (1.0, 0.85), (0.0, 0.85)]
    right = [(0.0, -0.15), (1.0, -0.15), (2.15, -0.15), (2.15, 1.15), (1.0, 1.15), (0.0, 1.15)]
    return hdv.HdvMap([left], [right], [[]], np.zeros((1, 1), dtype=np.uint8))


def along(hmap, lanelet, q):
    """centre point q of a lanelet and the heading of the centre line there -> (x, y, yaw)"""
    c = hmap.centre[lanelet - 1]
    b = min(q + 1, c.shape[0] - 1)
    return float(c[q, 0]), float(c[q, 1]), math.atan2(c[b, 1] - c[b - 1, 1], c[b, 0] - c[b - 1, 0])


class Case:
    """one traffic call: hdvs = [(x, y, yaw, trim, (dx, dy))], cavs = [(x, y, lanelet, (dx, dy))]"""

    def __init__(self, name, hmap, sets, hdvs, cavs):
        self.name, self.hmap, self.sets, self.hdvs, self.cavs = name, hmap, sets, hdvs, cavs

    def args(self):
        h, c = self.hdvs, self.cavs
        return ([v[0] for v in h], [v[1] for v in h], [v[2] for v in h], [v[3] for v in h], [v[4] for v in h],
                [v[0] for v in c], [v[1] for v in c], [v[2] for v in c], [v[3] for v in c])

    def python(self):
        return hdv.hdv_traffic(self.hmap, self.sets, *self.args())

    def host(self, **kw):
        return hdv.hdv_traffic_native(self.hmap, self.sets, *self.args(), **kw)

    def device(self, handle, **kw):
        return handle.hdv_traffic(*self.args(), **kw)


def _cavs(hmap, ids, tile=(0.0, 0.0)):
    return [along(hmap, i, 1)[:2] + (i, tile) for i in ids]


def traffic_cases():
    """The cases of the device test (and of the twins' comparison on the CPU), by what each reaches:
    n_hdv 1 and 3, n_cav 1 and 5, Hp 1 and 6, the fork (lanelet 3 -> 5, 23: two chains of one lanelet), the point with 8 closest
    lanelets (8 rows of one HDV), an HDV 1 m off the road (polygons of 0 vertices), hulls of PDMPC_REACHABLE_MAX_COLS vertices, and a
    tile offset (the HDV and one CAV on a copy of the map 12 m away, the other CAVs not)."""
    lab = hdv.lab_hdv_map()
    zero = (0.0, 0.0)
    out = []
    x, y, yaw = along(lab, 3, 0)
    out.append(Case("lanelet 3's first point, Hp 6, 1 HDV, 1 CAV", lab, local_sets(6), [(x, y, yaw, 1, zero)], _cavs(lab, [5])))
    out.append(Case("Hp 1, 1 HDV, 5 CAVs", lab, local_sets(1), [(x, y, yaw, 1, zero)], _cavs(lab, [3, 5, 23, 1, 64])))
    x8, y8, yaw8 = along(lab, 17, 10)
    xf, yf, yawf = along(lab, 3, 3)
    out.append(Case("3 HDVs (8 closest lanelets; the fork; a straight), 5 CAVs", lab, local_sets(6),
                    [(x8, y8, yaw8, 1, zero), (xf, yf, yawf, 1, zero), along(lab, 64, 3) + (1, zero)], _cavs(lab, [17, 3, 5, 64, 66])))
    xo, yo, yawo = along(lab, 64, 3)
    out.append(Case("1 m off the road: empty early steps", lab, local_sets(6), [(xo - 1.0 * math.sin(yawo), yo + 1.0 * math.cos(yawo), yawo, 1, zero)], _cavs(lab, [64])))
    out.append(Case("hulls of 256 vertices", lab, ngon_sets(256, 6), [(xf, yf, yawf, 1, zero), (x8, y8, yaw8, 1, zero)], _cavs(lab, [3])))
    tile = (12.0, 24.0)
    out.append(Case("tile offset", lab, local_sets(6), [(xf + tile[0], yf + tile[1], yawf, 1, tile)],
                    [along(lab, 64, 1)[:2] + (64, zero), (along(lab, 64, 1)[0] + tile[0], along(lab, 64, 1)[1] + tile[1], 64, tile)]))
    return out


def assert_same(a, b, what):
    """two results of a traffic call, bit for bit: lists, rows, offsets (through the shapes), vertices, flags, adjacency"""
    assert a["closest"] == b["closest"], (what, a["closest"], b["closest"])
    assert a["row_hdv"] == b["row_hdv"], (what, a["row_hdv"], b["row_hdv"])
    assert np.array_equal(a["flags"], b["flags"]), (what, a["flags"], b["flags"])
    assert np.array_equal(a["adjacency"], b["adjacency"]), (what, a["adjacency"], b["adjacency"])
    if "set_offset" in a and "set_offset" in b:
        assert np.array_equal(a["set_offset"], b["set_offset"]), what
    assert len(a["sets"]) == len(b["sets"]), what
    for r, (ra, rb) in enumerate(zip(a["sets"], b["sets"])):
        for k, (pa, pb) in enumerate(zip(ra, rb)):
            assert pa.shape == pb.shape and np.ascontiguousarray(pa).tobytes() == np.ascontiguousarray(pb).tobytes(), (what, r, k, pa.shape, pb.shape)


# ---- closed loops with HDVs (tests/test_hdv_controller.py, tests/test_gpu_hdv_controller.py)

LOOP_PATH_IDS = [9, 10, 12, 13]  # four CAVs on loop 2 of the lab map (lanelets 1, 3, 23, 10, 12, 17, ...)
# An HDV standing on CAV 0's lane 0.6 m ahead of its start (path id 9 starts at (2.25, 3.745) heading along +x): chosen on the CPU with
# the oracle -- CAV 0's plan goes round it (tests/test_hdv_controller.py)
HDV_AHEAD_POSE = (2.8499986954287677, 3.745683977765627, -0.0032222030068918763)


def loop_options(n_hdv, Hp=6, **kw):
    return Config(scenario_type=ScenarioType.commonroad, amount=len(LOOP_PATH_IDS), Hp=Hp, mpa_type=MpaType.single_speed, path_ids=list(LOOP_PATH_IDS),
                  manual_control=n_hdv, **kw)


def hdv_poses_at(step, speed=0.5, dt=0.2):
    """Two HDVs driven by the test at constant speed along the centre line of loop 2, 0.7 m and 2.9 m ahead of CAV 0's start -> (x, y, yaw)
    lists for time step `step` (1-based)."""
    from pdmpc.road_network import generate_reference_path_loop, get_reference_lanelets_loop, lab_map

    path, _ = generate_reference_path_loop(get_reference_lanelets_loop(9), lab_map().lanelets)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(path, axis=0).T))])
    xs, ys, yaws = [], [], []
    for start in (0.7, 2.9):
        at = start + speed * dt * (step - 1)
        j = int(np.searchsorted(s, at))
        xs.append(float(np.interp(at, s, path[:, 0])))
        ys.append(float(np.interp(at, s, path[:, 1])))
        yaws.append(math.atan2(path[j, 1] - path[j - 1, 1], path[j, 0] - path[j - 1, 0]))
    return xs, ys, yaws


def loop_controller(options, traffic=None, **kw):
    """the Python controller on the four-CAV loop with distance coupling; with options.manual_control HDVs set (traffic: see set_hdvs)"""
    from pdmpc.controller import PrioritizedSequentialController
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    sc = commonroad_scenario(options, seed=1)
    ctl = PrioritizedSequentialController(options, sc, get_mpa(options), None, coupling="distance", boundary_provider=boundary_provider(sc), **kw)
    if options.manual_control:
        ctl.set_hdvs(local_sets(options.Hp), hdv.lab_hdv_map(), traffic=traffic)
    return ctl


def crossings(shape, poly):
    """pairs of edges of two closed or open polygons (2, m) that properly cross or touch (orientation tests in double arithmetic)"""
    def edges(p):
        p = np.asarray(p, dtype=np.float64)
        if p.shape[1] < 2:
            return np.zeros((0, 4))
        q = np.roll(p, -1, axis=1)
        return np.column_stack([p[0], p[1], q[0], q[1]])

    n = 0
    for ax, ay, bx, by in edges(shape):
        for cx, cy, dx, dy in edges(poly):
            o1 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            o2 = (bx - ax) * (dy - ay) - (by - ay) * (dx - ax)
            o3 = (dx - cx) * (ay - cy) - (dy - cy) * (ax - cx)
            o4 = (dx - cx) * (by - cy) - (dy - cy) * (bx - cx)
            if o1 * o2 < 0 and o3 * o4 < 0:
                n += 1
    return n
