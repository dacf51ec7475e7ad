"""What the tests of the HDV driver model share (tests/test_hdv_drive_host.py, tests/test_gpu_hdv_drive.py): the maps,
the members -- one step of the HDVs and CAVs of one member, with the reason each is there -- and the bit-for-bit comparison."""
import math
import struct

import numpy as np

from pdmpc import hdv

ZERO = (0.0, 0.0)
LOOP = 9  # the lab map's loop the closed-loop tests drive on (tests/hdv_cases.py: LOOP_PATH_IDS)
_CACHE = {}


def lab():
    if "lab" not in _CACHE:
        _CACHE["lab"] = hdv.lab_hdv_map()
    return _CACHE["lab"]


def hand_map():
    """hdv_cases.hand_map with two things made by hand: lanelet 1 has its middle point twice (a segment of length 0 at j = 1), and a
    fourth lanelet, alone, of 101 points 0.01 m apart along y = 5: more than PDMPC_HDV_WINDOW_MAX segments inside any look-ahead."""
    w = 0.25
    x1 = (0.0, 1.0, 1.0, 2.0)
    xs = (0.0, 1.0, 2.0)
    fine = [0.01 * q for q in range(101)]
    left = [[(x, w) for x in x1], [(x + 2.0, w) for x in xs], [(x, -1.0 + 0.5 * x + w) for x in xs], [(x, 5.0 + w) for x in fine]]
    right = [[(x, -w) for x in x1], [(x + 2.0, -w) for x in xs], [(x, -1.0 + 0.5 * x - w) for x in xs], [(x, 5.0 - w) for x in fine]]
    rel = np.zeros((4, 4), dtype=np.uint8)
    rel[0, 1], rel[1, 2], rel[0, 2] = hdv.LONGITUDINAL, hdv.LONGITUDINAL, hdv.MERGING
    return hdv.HdvMap(left, right, [[2], [], [2], []], rel)


def loop_route():
    return hdv.route_from_loop(LOOP)


def route_length(hmap, route):
    ids, closed = route
    return sum(hdv._route_segment(hmap, ids, closed, r, j)[4] for r in range(len(ids)) for j in range(hdv._route_segments(hmap, ids, closed, r)))


def at(hmap, route, distance, tile=ZERO, side=0.0):
    """the point `distance` metres along the route, `side` metres to the left of it -> (x, y)"""
    state = hdv.place(hmap, route[0], route[1], distance)
    x, y, c, s = hdv.state_pose(hmap, route[0], route[1], state, tile)
    return x - side * s, y + side * c


def arc(hmap, route, state):
    """metres from the start of the route to a state (the sum of the segments in front of it, then u)"""
    ids, closed = route
    r0, j0, u = state
    return sum(hdv._route_segment(hmap, ids, closed, r, j)[4] for r in range(r0 + 1) for j in range(hdv._route_segments(hmap, ids, closed, r)) if (r, j) < (r0, j0)) + u


class Member:
    """one step of one member: hdvs = [(route, start distance, tile, v_des)], cavs = [(x, y, tile)]"""

    def __init__(self, name, hmap, hdvs, cavs, params=hdv.DRIVE_DEFAULTS, dt=0.2, states=None):
        self.name, self.hmap, self.params, self.dt = name, hmap, tuple(params), dt
        self.routes = [h[0] for h in hdvs]
        self.states = states if states is not None else [hdv.place(hmap, h[0][0], h[0][1], h[1]) for h in hdvs]
        self.tiles = [h[2] for h in hdvs]
        self.v_des = [h[3] for h in hdvs]
        self.cav_x, self.cav_y, self.cav_tile = [c[0] for c in cavs], [c[1] for c in cavs], [c[2] for c in cavs]

    def args(self):
        return (self.routes, self.states, self.tiles, self.v_des, self.cav_x, self.cav_y, self.cav_tile, self.params, self.dt)

    def python(self):
        return hdv.drive(self.hmap, *self.args())

    def host(self):
        return hdv.drive_native(self.hmap, *self.args())

    def group(self, slot, **more):
        return dict(slot=slot, routes=self.routes, states=self.states, tiles=self.tiles, v_des=self.v_des, cav_x=self.cav_x, cav_y=self.cav_y, cav_tile=self.cav_tile,
                    params=self.params, dt=self.dt, **more)

    def after(self, result, name):
        """the member one step later, the CAVs where they were"""
        m = Member(name, self.hmap, [], [], self.params, self.dt, states=result["states"])
        m.routes, m.tiles, m.v_des, m.cav_x, m.cav_y, m.cav_tile = self.routes, self.tiles, self.v_des, self.cav_x, self.cav_y, self.cav_tile
        return m


def bits(v):
    return struct.pack("<d", float(v))


def assert_same(a, b, what):
    """two results of a driver step, bit for bit: state, pose, cos and sin, speed, gap"""
    assert len(a["states"]) == len(b["states"]), what
    for q, (sa, sb) in enumerate(zip(a["states"], b["states"])):
        assert sa[:2] == sb[:2] and bits(sa[2]) == bits(sb[2]), (what, q, sa, sb)
    for key in ("x", "y", "cos_yaw", "sin_yaw", "speed", "gap"):
        assert [bits(v) for v in a[key]] == [bits(v) for v in b[key]], (what, key, a[key], b[key])


def lab_members():
    """The members on the lab map by what each reaches; `expect` holds what the step must give beyond equal bits."""
    L, R = lab(), loop_route()
    total = route_length(L, R)
    first = sum(hdv._route_segment(L, R[0], R[1], 0, j)[4] for j in range(hdv._route_segments(L, R[0], R[1], 0)))  # lanelet 1 of the route with its joint
    open3 = (R[0][:3], False)
    end3 = route_length(L, open3)
    tile = (12.0, 24.0)
    out = []

    def add(name, hdvs, cavs, expect, **kw):
        m = Member(name, L, hdvs, cavs, **kw)
        m.expect = expect
        out.append(m)

    add("free road", [(R, 0.7, ZERO, 0.5)], [], dict(speed=[0.5], gap=[math.inf]))
    add("a CAV 0.6 m ahead: slowed", [(R, 0.7, ZERO, 0.5)], [at(L, R, 1.3) + (ZERO,)], dict(slowed=[0]))
    add("a CAV 0.2 m ahead: inside gap_min, stopped", [(R, 0.7, ZERO, 0.5)], [at(L, R, 0.9) + (ZERO,)], dict(speed=[0.0]))
    add("a CAV 0.1 m beside the route, lateral just above", [(R, 0.7, ZERO, 0.5)], [at(L, R, 1.3, side=0.1) + (ZERO,)], dict(slowed=[0]), params=(2.0, 0.3, 1.0, 0.1 + 1e-9))
    add("a CAV 0.1 m beside the route, lateral just below", [(R, 0.7, ZERO, 0.5)], [at(L, R, 1.3, side=0.1) + (ZERO,)], dict(speed=[0.5], gap=[math.inf]),
        params=(2.0, 0.3, 1.0, 0.1 - 1e-9))
    add("a CAV behind", [(R, 0.7, ZERO, 0.5)], [at(L, R, 0.4) + (ZERO,)], dict(speed=[0.5], gap=[math.inf]))
    add("an HDV follows an HDV: the gap is to where the leader WAS", [(R, 0.7, ZERO, 0.5), (R, 1.1, ZERO, 0.5)], [], dict(slowed=[0], speed=[None, 0.5]))
    add("a step over several segments and a lanelet joint", [(R, first - 0.05, ZERO, 3.0)], [], dict(speed=[3.0], crosses=[0]), params=(2.0, 0.3, 1.0, 0.125))
    add("wrap-around on the closed route, a CAV behind the wrap", [(R, total - 0.02, ZERO, 0.5)], [at(L, R, 0.5) + (ZERO,)], dict(slowed=[0], wraps=[0]))
    add("the end of an open route", [(open3, end3 - 0.05, ZERO, 0.5)], [], dict(speed=[0.0], ends=[0]))
    add("a CAV ahead on another tile, one on the HDV's own", [(R, 0.7, ZERO, 0.5), (R, 0.7, tile, 0.5)], [at(L, R, 1.3, tile) + (tile,)], dict(speed=[0.5, None], slowed=[1]))
    return out


def hand_members():
    """... on the hand-made map: the segment of length 0, and the window cap"""
    Hm = hand_map()
    out = []

    def add(name, hdvs, cavs, expect, **kw):
        m = Member(name, Hm, hdvs, cavs, **kw)
        m.expect = expect
        out.append(m)

    r12, r32, r4 = ([1, 2], False), ([3, 2], False), ([4], False)
    add("over the segment of length 0, a CAV behind it", [(r12, 0.95, ZERO, 2.0)], [(1.75, 0.0, ZERO)], dict(slowed=[0], crosses=[0]))
    add("the window cap: a CAV 0.8 m ahead lies behind segment 64", [(r4, 0.0, ZERO, 0.5)], [(0.8, 5.0, ZERO)], dict(speed=[0.5], gap=[math.inf]))
    add("the window cap: a CAV 0.5 m ahead lies within it", [(r4, 0.0, ZERO, 0.5)], [(0.5, 5.0, ZERO)], dict(slowed=[0]))
    add("merging routes: the HDV on lanelet 3 sees the one on lanelet 2", [(r32, 1.9, ZERO, 0.5), (r12, 2.4, ZERO, 0.5)], [], dict(slowed=[0]))
    return out


def check_expectations(m, r):
    """what a member's step must give beyond equal bits"""
    e = m.expect
    for q, v in enumerate(e.get("speed", [])):
        if v is not None:
            assert r["speed"][q] == v, (m.name, q, r["speed"])
    for q, v in enumerate(e.get("gap", [])):
        assert r["gap"][q] == v, (m.name, q, r["gap"])
    for q in e.get("slowed", []):
        assert 0.0 < r["speed"][q] < m.v_des[q] and math.isfinite(r["gap"][q]), (m.name, q, r["speed"], r["gap"])
    for q in e.get("crosses", []):
        assert r["states"][q][:2] != m.states[q][:2], (m.name, r["states"])
    for q in e.get("wraps", []):
        assert r["states"][q][0] == 0 and m.states[q][0] == len(m.routes[q][0]) - 1, (m.name, r["states"], m.states)
    for q in e.get("ends", []):
        ids, closed = m.routes[q]
        rr, jj, u = r["states"][q]
        assert rr == len(ids) - 1 and jj == hdv._route_segments(m.hmap, ids, closed, rr) - 1 and u == hdv._route_segment(m.hmap, ids, closed, rr, jj)[4], (m.name, r["states"])
