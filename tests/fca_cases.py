"""The input families of the exact collision-assessment tests (tests/test_fca_exact.py on the CPU, tests/test_gpu_fca_limits.py on the
device).  The reference is tests/fca_reference.py; here are only inputs and, where a family has one, its closed form.

Lattice families use length 0.5, width 0.25, offset 0.125: half sizes 0.375 and 0.25, and every coordinate a multiple of 2^-10."""
import math

import numpy as np

import exact_geometry as X
from pdmpc.backend import fca_collisions_host, fca_pairs
from pdmpc.mpa import VEHICLE_LENGTH, VEHICLE_WIDTH

LENGTH, WIDTH, OFFSET = 0.5, 0.25, 0.125
HL, HW = 0.375, 0.25
STEP = 2.0 ** -10
GENERAL_SIZES = (VEHICLE_LENGTH, VEHICLE_WIDTH, 0.01)
HEADINGS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


class Case:
    """the arguments of one call; `expected`: the family's closed-form counts, if it has one; `lattice`: every test lattice-exact"""

    def __init__(self, family, refs, pairs, headings, obstacles=(), dynamic=(), sizes=(LENGTH, WIDTH, OFFSET), lattice=True, expected=None):
        self.family, self.refs, self.pairs, self.headings = family, refs, np.asarray(pairs, dtype=np.int32).reshape(-1, 2), headings
        self.obstacles, self.dynamic, self.sizes, self.lattice, self.expected = list(obstacles), list(dynamic), sizes, lattice, expected

    @property
    def n(self):
        return len(self.refs)

    @property
    def Hp(self):
        return len(self.refs[0])

    def call(self, f, **kw):
        """f = backend.fca_collisions_host or Handle.fca_collisions -> counts"""
        return f(self.refs, self.pairs, *self.sizes, self.obstacles, self.dynamic, headings=self.headings, **kw)[0]

    def python_twin(self, with_headings=True):
        from pdmpc.prioritizer import fca_priorities

        A = np.zeros((self.n, self.n), dtype=np.int64)
        for a, b in self.pairs.tolist():
            A[a, b] = A[b, a] = 1
        prio, coll = fca_priorities(A, self.refs, *self.sizes, self.obstacles, self.dynamic, headings=self.headings if with_headings else None)
        return np.asarray(coll, dtype=np.int64)

    def exact(self):
        import fca_reference as F

        return F.counts(self.refs, self.pairs, *self.sizes, self.obstacles, self.dynamic, headings=self.headings, lattice=self.lattice)


UNDECIDED_CAP = 0.01  # the share of undecided tests a general-position family may have; a lattice family may have none


def check(case, margins, python=True, device=None):
    """every twin (the host twin, the Python twin, `device`: a Handle) against the exact counts where decided, against the closed form
    if the family has one, and against the host twin bit for bit; recorded in `margins`; -> the assessment"""
    a = case.exact()
    what = (case.family, case.n, case.Hp)
    if case.expected is not None:
        assert a.counts == list(case.expected), ("the reference misses the closed form", what)
    if case.lattice:
        assert a.undecided == 0 and all(a.decided)
    host = case.call(fca_collisions_host)
    twins = [("host", host)]
    if python:
        twins.append(("python", case.python_twin()))
    if device is not None:
        twins.append(("device", case.call(device.fca_collisions)))
    for twin, got in twins:
        wrong = margins.add(case.family, twin, a, got)
        assert not wrong, (what, twin, "(vehicle, got, exact)", wrong[:8])
        assert np.array_equal(np.asarray(got, dtype=np.int64), np.asarray(host, dtype=np.int64)), (what, twin, "differs from the host twin")
    return a


def full(n):
    return fca_pairs(np.ones((n, n)) - np.eye(n))


def turned(n, Hp, heading):
    """every vehicle at every step with the one heading (cos, sin)"""
    return np.full((n, Hp), heading[0]), np.full((n, Hp), heading[1])


def box(x0, y0, x1, y1):
    return np.array([[x0, x1, x1, x0], [y0, y0, y1, y1]], dtype=np.float64)


# ---- lattice families


def abutting_grid(heading, Hp=4, side=4, gap=0.0, origin=(0.0, 0.0), alternate=False):
    """side x side vehicles of one heading, the pitch the footprint's size (+ gap): with gap 0 neighbours share an edge and diagonal
    neighbours a corner, which intersect_sat.m counts as collisions; all move together by 2^-4 per step.  alternate: every other
    vehicle turned by a half turn (the same box from the opposite corners).  Closed form: 8-neighbours x Hp, or 0 with a gap."""
    ex, ey = (2 * HL, 2 * HW) if heading[1] == 0.0 else (2 * HW, 2 * HL)
    n = side * side
    refs = [np.stack([origin[0] + (v % side) * (ex + gap) + np.arange(Hp) / 16.0, np.full(Hp, origin[1] + (v // side) * (ey + gap))], axis=1) for v in range(n)]
    c, s = turned(n, Hp, heading)
    if alternate:
        c[1::2], s[1::2] = -c[1::2], -s[1::2]
    neighbours = [sum(1 for dv in (-1, 0, 1) for dh in (-1, 0, 1) if (dv or dh) and 0 <= v // side + dv < side and 0 <= v % side + dh < side) for v in range(n)]
    expected = [Hp * m if gap == 0.0 else 0 for m in neighbours]
    return Case("abutting grid", refs, full(n), (c, s), expected=expected)


def polygon_zoo(seed=3):
    """Static polygons of 1, 2, 3, 5, 8, 17 and 64 vertices in shuffled order around two standing vehicles (vehicle 0 at the origin
    heading east, vehicle 1 at (8, 0) heading north; vehicle 2, the last, stands on an obstacle of its own, which does not count):
    points inside, on an edge, on a corner and just outside; segments along an edge, a step off it, across the footprint and along
    the line of an edge beyond the corner; a triangle that only its closing edge's axis separates from the footprint; n-gons in and out."""
    Hp = 2
    refs = [np.tile([[0.0, 0.0]], (Hp, 1)), np.tile([[8.0, 0.0]], (Hp, 1)), np.tile([[0.0, 8.0]], (Hp, 1))]
    c, s = turned(3, Hp, (1.0, 0.0))
    c[1], s[1] = 0.0, 1.0
    pt = lambda x, y: np.array([[x], [y]])
    seg = lambda x0, y0, x1, y1: np.array([[x0, x1], [y0, y1]])
    obst = [
        pt(0.125, 0.0625), pt(HL, 0.125), pt(HL, HW), pt(HL + STEP, 0.0), pt(-HL, -HW - STEP),  # vehicle 0: inside, edge, corner, 2 x outside
        pt(8.0 + HW, HL), pt(8.0 + HW + STEP, HL),  # vehicle 1 (half sizes swapped by the quarter turn): corner, outside
        seg(-0.25, HW, 0.25, HW), seg(-0.25, HW + STEP, 0.25, HW + STEP), seg(-1.0, -0.5, 1.0, 0.5), seg(0.5, HW, 1.0, HW),
        seg(8.0 - HW, -1.0, 8.0 - HW, 1.0), seg(8.0 - HW - STEP, -1.0, 8.0 - HW - STEP, 1.0),
        np.array([[0.25, 0.625, 0.625], [0.5, 0.5, 0.125]]),  # hypotenuse x + y = 0.75 closes it; the corner (0.375, 0.25) is below
        np.array([[0.0, 0.5, 0.5], [0.5, 0.5, 0.0]]),  # this one cuts the corner off (x + y = 0.5)
        np.array([[8.0, 8.5, 7.5], [0.25, -1.0, -1.0]]),
        X.arr(X.ngon(5, 0.3, 0.4, 8.5, 0.3)), X.arr(X.ngon(5, 0.3, 0.4, 8.875, 0.75)),
        X.arr(X.ngon(8, 0.2, 0.1, 7.6, -0.5)), X.arr(X.ngon(8, 0.2, 0.1, 7.5, -0.625)),
        X.arr(X.ngon(17, 0.5, 1.0, 8.0, 0.8)), X.arr(X.ngon(17, 0.5, 1.0, 8.0, 1.0)),
        X.arr(X.ngon(64, 1.0, 0.0, -1.2, 0.0)), X.arr(X.ngon(64, 1.0, 0.0, 1.5, 1.2)), X.arr(X.ngon(64, 1.0, 0.02, 0.0, 1.2)),
        box(-0.25, 7.75, 0.25, 8.25),  # under the last vehicle only
    ]
    order = np.random.default_rng(seed).permutation(len(obst))
    return Case("point, segment, polygon", refs, full(3), (c, s), [obst[i] for i in order], lattice=False)


def dynamic_rows():
    """3 rows x Hp 5 over 4 vehicles (the last has no row and would skip it).  Vehicle v at step k stands at (20 k, 20 v); the polygon of
    (row r, step k) is a 3 + ((2 r + 3 k) % 7)-gon of radius 2 with one vertex on vehicle r's step-k point: the vertex farthest from its
    first four, so that those four alone miss the footprint.  Every polygon hits its vehicle at its step and nothing else: Hp each."""
    Hp, n = 5, 4
    refs = [np.stack([20.0 * np.arange(Hp), np.full(Hp, 20.0 * v)], axis=1) for v in range(n)]
    rows = []
    for r in range(3):
        row = []
        for k in range(Hp):
            m = 3 + ((2 * r + 3 * k) % 7)
            j = (3 + m) // 2 if m >= 5 else 0
            phase = 0.3 + r + 0.7 * k
            t = phase - 2 * math.pi * j / m
            row.append(X.arr(X.ngon(m, 2.0, phase, 20.0 * k - 2.0 * math.cos(t), 20.0 * r - 2.0 * math.sin(t))))
        rows.append(row)
    return Case("dynamic rows", refs, full(n), turned(n, Hp, (1.0, 0.0)), dynamic=rows, lattice=False, expected=[Hp, Hp, Hp, 0])


def with_repeats(P, mode):
    """(2, m) polygon -> 1: closed by its first vertex (as the reference's shapes are), 2: an interior vertex doubled, 3: both"""
    cols = list(range(P.shape[1]))
    if mode & 2:
        cols.insert(P.shape[1] // 2, P.shape[1] // 2)
    if mode & 1:
        cols.append(0)
    return P[:, cols]


def zero_length_edges(mode):
    """two standing vehicles and a few obstacles that touch, overlap and miss them; mode 0 as they are, else with_repeats(mode)"""
    Hp = 3
    refs = [np.tile([[0.0, 0.0]], (Hp, 1)), np.tile([[4.0, 0.0]], (Hp, 1)), np.tile([[0.0, 4.0]], (Hp, 1))]
    c, s = turned(3, Hp, (1.0, 0.0))
    c[1], s[1] = 0.0, -1.0
    obst = [box(HL, -0.125, 1.0, 0.125), box(HL + STEP, -0.125, 1.0, 0.125), box(4.0 - HW - 0.5, HL, 4.0 - HW, 1.0),
            np.array([[0.25, 0.625, 0.625], [0.5, 0.5, 0.125]]), np.array([[0.0, 0.5, 0.5], [0.5, 0.5, 0.0]]),
            X.arr(X.ngon(8, 0.5, 0.2, 4.5, 0.5)), X.arr(X.ngon(8, 0.5, 0.2, 5.0, 1.0)), np.array([[-1.0, 1.0], [-0.5, 0.5]])]
    dyn = [[box(3.5, -0.75 + 0.25 * k, 4.5, -0.625 + 0.25 * k) for k in range(Hp)]]
    rep = lambda P: P if mode == 0 else with_repeats(P, mode)
    return Case("zero-length edges", refs, full(3), (c, s), [rep(o) for o in obst], [[rep(p) for p in row] for row in dyn], lattice=False)


def last_vehicle(reverse):
    """five vehicles far apart and an obstacle under the last one only (reverse: under the first): the reference's outer loop never
    reaches the last vehicle"""
    Hp, n = 4, 5
    refs = [np.stack([10.0 * v + np.arange(Hp) / 16.0, np.zeros(Hp)], axis=1) for v in range(n)]
    if reverse:
        refs = refs[::-1]
    return Case("last vehicle", refs, full(n), turned(n, Hp, (1.0, 0.0)), [box(39.75, -0.125, 40.5, 0.125)], expected=[Hp if reverse and v == 0 else 0 for v in range(n)])


def couples(n, Hp, pairs, coincident):
    """n vehicles, vehicle v on the spot of `coincident[v]` (spots 8 m apart on a 32-wide grid), every vehicle moving 2^-4 east per step.
    Closed form: Hp for every listed pair of vehicles on one spot."""
    spot = np.asarray(coincident)
    refs = [np.stack([8.0 * (spot[v] % 32) + np.arange(Hp) / 16.0, np.full(Hp, 8.0 * (spot[v] // 32))], axis=1) for v in range(n)]
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    expected = np.zeros(n, dtype=np.int64)
    same = spot[pairs[:, 0]] == spot[pairs[:, 1]]
    np.add.at(expected, pairs[same, 0], Hp)
    np.add.at(expected, pairs[same, 1], Hp)
    return refs, pairs, expected


def pair_index(n, a, b):
    """the position of (a, b), a < b, in the ascending list of all pairs of n vehicles"""
    return a * n - a * (a + 1) // 2 + (b - a - 1)


def stride_tail(n=512, Hp=10):
    """full coupling of 256 coincident couples (2 v, 2 v + 1): n (n - 1) / 2 pairs x Hp items, every count Hp"""
    refs, pairs, expected = couples(n, Hp, full(n), np.arange(n) // 2)
    return Case("stride tail", refs, pairs, turned(n, Hp, (1.0, 0.0)), expected=expected.tolist())


def stride_edge(n_pairs, Hp=16, n=512, obstacle=False):
    """the first n_pairs pairs of the full coupling of n vehicles; coincident: (0, 1), a pair in the middle of the list and the last
    listed pair; obstacle: one static box under vehicle 0 (its items follow the pair items)"""
    pairs = full(n)[:n_pairs]
    spot = np.arange(n)
    for a, b in ((0, 1), tuple(pairs[n_pairs // 2]), tuple(pairs[-1])):
        spot[b] = spot[a]
    refs, pairs, expected = couples(n, Hp, pairs, spot)
    obst = [box(-0.25, -0.125, 2.0, 0.125)] if obstacle else []
    if obstacle:
        assert spot[0] == spot[1] == 0 and (spot[2:] != 0).all()
        expected[:2] += Hp
    return Case("stride edge", refs, pairs, turned(n, Hp, (1.0, 0.0)), obst, expected=expected.tolist())


def one_counter_boxes(n_boxes=2000, Hp=2):
    """n_boxes static lattice boxes of every size over vehicle 0 of 2 (some only touch it): n_boxes x Hp hits on one counter"""
    refs = [np.zeros((Hp, 2)), np.tile([[16.0, 0.0]], (Hp, 1))]
    obst = [box(-HL - (i % 7) * STEP, HW - (i % 5) * 0.125, HL + (i % 3) * 0.25, HW + 0.5 + i * STEP) for i in range(n_boxes)]
    return Case("one counter", refs, full(2), turned(2, Hp, (1.0, 0.0)), obst, expected=[n_boxes * Hp, 0])


def one_counter_vehicles(n=128, Hp=2):
    refs, pairs, expected = couples(n, Hp, full(n), np.zeros(n, dtype=np.int64))
    return Case("one counter", refs, pairs, turned(n, Hp, (1.0, 0.0)), expected=expected.tolist())


# ---- general position


def _traffic(rng, n, Hp, side):
    """bent reference trajectories, dense enough that footprints meet (tests/test_fca_priorities.py::_traffic)"""
    refs = []
    for _ in range(n):
        x0, y0 = rng.uniform(0, side, 2)
        a = rng.uniform(-math.pi, math.pi)
        t = np.arange(Hp) * rng.uniform(0.02, 0.08)
        bend = rng.uniform(-0.3, 0.3) * t * t
        refs.append(np.stack([x0 + math.cos(a) * t - math.sin(a) * bend, y0 + math.sin(a) * t + math.cos(a) * bend], axis=1))
    return refs


def _convex(rng, side, m):
    """a convex polygon of m vertices: points of an ellipse in clockwise order, turned by a random angle"""
    t = np.sort(rng.uniform(0, 2 * math.pi, m))[::-1]
    a, b, turn = rng.uniform(0.05, 0.25), rng.uniform(0.05, 0.25), rng.uniform(0, math.pi)
    x, y = a * np.cos(t), b * np.sin(t)
    cx, cy = rng.uniform(0, side, 2)
    return np.stack([cx + math.cos(turn) * x - math.sin(turn) * y, cy + math.sin(turn) * x + math.cos(turn) * y])


def general_position(n, Hp=6, seed=11, shift=0.0, n_obst=6, n_rows=2):
    """random traffic with the headings of calculate_yaw, random convex obstacles and rows, distance coupling; shift: the scene moved"""
    import fca_reference as F

    rng = np.random.default_rng(seed)
    side = max(0.6, math.sqrt(n) * 0.35)
    refs = [r + shift for r in _traffic(rng, n, Hp, side)]
    p = np.array([r[0] for r in refs])
    A = (np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]) <= 0.8).astype(np.int64)
    np.fill_diagonal(A, 0)
    sizes = iter((3 + rng.permutation(n_obst + n_rows * Hp) % 10).tolist())  # 3 to 12 vertices, every size if there are ten polygons
    obst = [_convex(rng, side, next(sizes)) + shift for _ in range(n_obst)]
    dyn = [[_convex(rng, side, next(sizes)) + shift for _ in range(Hp)] for _ in range(n_rows)]
    return Case("general position" if shift == 0.0 else "general position, far", refs, fca_pairs(A), F.headings_of(refs), obst, dyn, sizes=GENERAL_SIZES, lattice=False)
