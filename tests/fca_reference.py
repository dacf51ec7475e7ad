"""The future collision assessment in exact arithmetic: the reference csrc/fca_kernel.hip, csrc/fca.cpp and
pdmpc.prioritizer.fca_priorities are checked against.

Doubles are exact rationals, so nothing here rounds: the footprints are `fractions.Fraction` points built from the doubles as given
(cos and sin of the heading included), and whether two closed convex sets share a point is decided by sign tests on integers.  Nothing
comes from include/pdmpc_geometry.h or from pdmpc.prioritizer; the point type and `cross` are tests/exact_geometry.py's.

`counts` follows the loop structure of FcaPrioritizer.m:24-89 and says, per vehicle, whether every test that contributes to its count
was *decided*: one whose outcome the float separating-axis test cannot get wrong for a reason other than a bug.

* A test between two *lattice-exact* polygons is always decided, touching included.  A footprint is lattice-exact if its heading is a
  quarter turn, (c, s) in {(1,0), (0,1), (-1,0), (0,-1)}, and its reference point and half sizes are multiples of 2^-10; any other
  polygon, if its coordinates are multiples of 2^-10 and every edge of non-zero length is parallel to an axis.  Every float operation
  of the float test is exact on two such polygons (an axis-parallel edge has an exact norm and an exact unit normal), and touching
  counts as a collision (intersect_sat.m separates on a strict `> 0`).
* Any other test is decided when |margin| >= 2^-30 R, R the largest absolute coordinate of the two polygons.  The float test's
  projection error is a few rounding steps of R (about 2^-50 R), so the band is wide on purpose.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from exact_geometry import cross

LATTICE = 1 << 10  # lattice-exact coordinates are multiples of 1 / LATTICE
BAND_BITS = 30  # a test off the lattice is decided when |margin| >= 2^-BAND_BITS * R
QUARTER_TURNS = ((1, 0), (0, 1), (-1, 0), (0, -1))


class Margin(namedtuple("Margin", "sign square")):
    """An exact signed distance: `sign` in {-1, 0, 1} and the exact `square` of its magnitude (a Fraction).  Positive: the separation
    along the best axis; negative: the penetration depth; zero: the sets touch.  float() is for classification only."""

    __slots__ = ()

    def __float__(self):
        return self.sign * math.sqrt(self.square)


def points(a):
    """(2, m) array of doubles -> list of Fraction points as given: nothing dropped, a repeated vertex stays"""
    a = np.asarray(a, dtype=np.float64).reshape(2, -1)
    return [(Fraction(x), Fraction(y)) for x, y in zip(a[0].tolist(), a[1].tolist())]


def footprint(c, s, x, y, length, width, offset):
    """The four exact corners of FcaPrioritizer.m:21-22: (±(length/2 + offset), ±(width/2 + offset)) in the order
    [-1,-1,1,1], [-1,1,1,-1], rotated by (c, s) and moved to (x, y).  Every argument is taken as the rational it is."""
    c, s, x, y = Fraction(c), Fraction(s), Fraction(x), Fraction(y)
    hl = Fraction(length) / 2 + Fraction(offset)
    hw = Fraction(width) / 2 + Fraction(offset)
    return [(c * px - s * py + x, s * px + c * py + y) for px, py in ((-hl, -hw), (-hl, hw), (hl, hw), (hl, -hw))]


def _on_lattice(v):
    return (Fraction(v) * LATTICE).denominator == 1


def footprint_is_lattice_exact(c, s, x, y, length, width, offset):
    hl = Fraction(length) / 2 + Fraction(offset)
    hw = Fraction(width) / 2 + Fraction(offset)
    # the float half sizes have to be the exact ones too
    exact_halves = Fraction(float(length) / 2 + float(offset)) == hl and Fraction(float(width) / 2 + float(offset)) == hw
    return (c, s) in QUARTER_TURNS and exact_halves and all(_on_lattice(v) for v in (x, y, hl, hw))


def polygon_is_lattice_exact(P):
    """coordinates on the lattice and every edge of non-zero length (the closing one included) parallel to an axis"""
    if not all(_on_lattice(p[0]) and _on_lattice(p[1]) for p in P):
        return False
    return all(P[i][0] == P[(i + 1) % len(P)][0] or P[i][1] == P[(i + 1) % len(P)][1] for i in range(len(P)))


# ---- the separating-axis test on integers


def _scaled(D, P):
    return [(int(p[0] * D), int(p[1] * D)) for p in P]


def _common_denominator(*polys):
    return math.lcm(1, *{c.denominator for P in polys for p in P for c in p})


def _edge_vectors(P):
    """the edges of non-zero length, the closing one included (a repeated vertex contributes none)"""
    out = []
    for i in range(len(P)):
        a, b = P[i], P[(i + 1) % len(P)]
        ex, ey = b[0] - a[0], b[1] - a[1]
        if ex or ey:
            out.append((ex, ey))
    return out


def _is_flat(edges):
    """no area: a point, a segment, or collinear points"""
    return not edges or all(edges[0][0] * e[1] - edges[0][1] * e[0] == 0 for e in edges[1:])


def _axes(A, B, edges_a=None, edges_b=None):
    """The candidate separating axes of two convex sets: the normals of the edges of both.  The boundary of A - B has no other edge
    directions, so these decide it whenever A - B has an area.  If both sets are flat (points, segments) A - B may have none; then the
    directions of the segments and the line through the first points are candidates too, which decides the remaining cases."""
    ea = _edge_vectors(A) if edges_a is None else edges_a
    eb = _edge_vectors(B) if edges_b is None else edges_b
    axes = [(-ey, ex) for ex, ey in ea] + [(-ey, ex) for ex, ey in eb]
    if _is_flat(ea) and _is_flat(eb):
        axes += ea[:1] + eb[:1]
        d = (B[0][0] - A[0][0], B[0][1] - A[0][1])
        if d != (0, 0):
            axes += [d, (-d[1], d[0])]
    return axes


def _meet(A, B, axes):
    """integer polygons -> (g |g|, n · n) of the best axis n: g / |n| is the largest signed gap over the axes, max(min A - max B,
    min B - max A) of the projections; without any axis (two equal points) (0, 1)"""
    bn, bd = None, 1
    for nx, ny in axes:
        pa = [nx * p[0] + ny * p[1] for p in A]
        pb = [nx * p[0] + ny * p[1] for p in B]
        g = max(min(pa) - max(pb), min(pb) - max(pa))
        num, den = g * abs(g), nx * nx + ny * ny
        if bn is None or num * bd > bn * den:
            bn, bd = num, den
    return (0, 1) if bn is None else (bn, bd)


def closed_convex_meet(A, B):
    """Do the closed convex hulls of the point lists A and B share a point?  -> (meets, margin).

    A and B are lists of Fraction points in convex position in either orientation: polygons (repeated vertices allowed: an edge of zero
    length contributes no axis), two-point segments, one-point polygons.  A separating-axis test without normalisation: for the normal
    n of every edge of both, the projections n · p are compared exactly.  margin (a Margin) is the largest signed gap over the axes
    divided by |n|: the separation if positive, minus the penetration depth if negative, zero if the sets touch; meets = margin <= 0."""
    D = _common_denominator(A, B)
    a, b = _scaled(D, A), _scaled(D, B)
    num, den = _meet(a, b, _axes(a, b))
    return num <= 0, Margin((num > 0) - (num < 0), Fraction(abs(num), den * D * D))


def convex_meet_by_definition(A, B):
    """The same answer from the definition, for polygons with an area (clockwise or not): they share a point iff a vertex of one lies in
    the other (closed) or two edges touch.  An independent check of closed_convex_meet."""
    from exact_geometry import _segments_touch

    def inside(p, P):
        sides = [cross(P[i], P[(i + 1) % len(P)], p) for i in range(len(P))]
        return all(s <= 0 for s in sides) or all(s >= 0 for s in sides)

    if any(inside(p, B) for p in A) or any(inside(p, A) for p in B):
        return True
    return any(_segments_touch(A[i], A[(i + 1) % len(A)], B[j], B[(j + 1) % len(B)]) for i in range(len(A)) for j in range(len(B)))


# ---- the assessment


class Assessment:
    """counts[v]; decided[v]: every test that contributes to counts[v] was decided; tests, undecided: the (vehicle, step, other) tests
    made and those not decided; smallest_ratio: the smallest |margin| / R of a decided test (0.0: a decided touch on the lattice;
    inf: no test)"""

    def __init__(self, n):
        self.counts = [0] * n
        self.decided = [True] * n
        self.tests = 0
        self.undecided = 0
        self.hits = 0
        self.touches = 0
        self.smallest_ratio = math.inf

    @property
    def undecided_share(self):
        return self.undecided / self.tests if self.tests else 0.0

    def compared(self, got):
        """(index, got, want) of the decided vehicles whose count differs"""
        return [(v, int(got[v]), self.counts[v]) for v in range(len(self.counts)) if self.decided[v] and int(got[v]) != self.counts[v]]


class _Shape:
    __slots__ = ("pts", "edges", "exact", "R")

    def __init__(self, D, P, exact):
        self.pts = _scaled(D, P)
        self.edges = _edge_vectors(self.pts)
        self.exact = exact
        self.R = max(max(abs(p[0]), abs(p[1])) for p in self.pts)


def counts(reference_points, pairs, length, width, offset, obstacles=(), dynamic_obstacle_area=(), headings=None, lattice=False):
    """The arguments of backend.fca_collisions_host, `headings` = (cos, sin) per vehicle and step required (the doubles the C ABI
    gets) -> Assessment, under the loop structure of FcaPrioritizer.m:24-89: vehicles 0 .. n-2 against every static obstacle and, at
    step k, polygon k of every dynamic row (polygon r Hp + k of the flat list); every listed pair at every step, a hit counting for
    both.  lattice=True asserts that every test of the call is between lattice-exact polygons (a lattice family)."""
    ref = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in reference_points]
    n, Hp = len(ref), len(ref[0])
    cs, sn = (np.asarray(h, dtype=np.float64).reshape(n, Hp) for h in headings)
    feet_exact = [[footprint(cs[v, k], sn[v, k], ref[v][k, 0], ref[v][k, 1], length, width, offset) for k in range(Hp)] for v in range(n)]
    statics = [points(o) for o in obstacles]
    rows = [[points(p) for p in row] for row in dynamic_obstacle_area]
    assert all(len(row) == Hp for row in rows), "a dynamic row holds Hp polygons"
    D = _common_denominator(*[f for fs in feet_exact for f in fs], *statics, *[p for row in rows for p in row])
    feet = [[_Shape(D, feet_exact[v][k], footprint_is_lattice_exact(cs[v, k], sn[v, k], ref[v][k, 0], ref[v][k, 1], length, width, offset))
             for k in range(Hp)] for v in range(n)]
    statics = [_Shape(D, P, polygon_is_lattice_exact(P)) for P in statics]
    rows = [[_Shape(D, P, polygon_is_lattice_exact(P)) for P in row] for row in rows]
    out = Assessment(n)

    def test(a, b, vehicles):
        num, den = _meet(a.pts, b.pts, _axes(a.pts, b.pts, a.edges, b.edges))
        R = max(a.R, b.R)
        exact = a.exact and b.exact
        assert exact or not lattice, "a lattice family with a test off the lattice"
        out.tests += 1
        # |margin| >= 2^-BAND_BITS R  <=>  |num| / den · 2^(2 BAND_BITS) >= R²  (margin² = |num| / den on the integer grid)
        if exact or (abs(num) << (2 * BAND_BITS)) >= R * R * den:
            if R:
                out.smallest_ratio = min(out.smallest_ratio, math.sqrt(Fraction(abs(num), den * R * R)))
        else:
            out.undecided += 1
            for v in vehicles:
                out.decided[v] = False
        if num <= 0:
            out.hits += 1
            out.touches += num == 0
            for v in vehicles:
                out.counts[v] += 1

    for v in range(n - 1):  # the outer loop of FcaPrioritizer.m:24 stops before the last vehicle
        for k in range(Hp):
            for o in statics:
                test(feet[v][k], o, (v,))
            for row in rows:
                test(feet[v][k], row[k], (v,))
    for a, b in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        assert 0 <= a < b < n
        for k in range(Hp):
            test(feet[a][k], feet[b][k], (a, b))
    return out


def headings_of(reference_points):
    """(cos, sin) as backend.fca_pack builds them without `headings`: calculate_yaw and the host's libm.  Input preparation for the
    general-position families (the reference takes the resulting doubles as given)."""
    from pdmpc.prioritizer import calculate_yaw

    yaw = [calculate_yaw(np.asarray(r, dtype=np.float64)) for r in reference_points]
    return (np.array([[math.cos(float(a)) for a in y] for y in yaw]), np.array([[math.sin(float(a)) for a in y] for y in yaw]))


# ---- the record (profiles/fca_exact_margins.txt)


class Margins:
    """per (family, twin): tests made, undecided, smallest decided |margin| / R, vehicles compared — a record of what the tests saw"""

    def __init__(self):
        self.rows = {}

    def add(self, family, twin, a, got):
        """records the assessment `a` of one case of `family` and returns the decided vehicles whose count in `got` is wrong"""
        t, u, r, c, h = self.rows.get((family, twin), (0, 0, math.inf, 0, 0))
        self.rows[(family, twin)] = (t + a.tests, u + a.undecided, min(r, a.smallest_ratio), c + sum(a.decided), h + a.hits)
        return a.compared(got)

    def share(self, family, twin):
        t, u = self.rows[(family, twin)][:2]
        return u / t if t else 0.0

    def lines(self):
        out = ["%-34s %-7s %9s %10s %10s %12s %9s %9s" % ("family", "twin", "tests", "undecided", "share", "min |m| / R", "hits", "vehicles")]
        for (family, twin), (t, u, r, c, h) in sorted(self.rows.items()):
            out.append("%-34s %-7s %9d %10d %9.4f%% %12.3e %9d %9d" % (family, twin, t, u, 100.0 * u / max(t, 1), r, h, c))
        return out


REPORT_HEADER = """The future collision assessment against exact arithmetic (tests/fca_reference.py), per family and twin: the (vehicle, step, other)
tests made, those not decided and their share, the smallest |margin| / R of a decided test (0: a decided touch on the lattice), the
hits, and the vehicles whose counts were compared (all equal: asserted).  A test off the lattice is decided when |margin| >= 2^-30 R;
asserted: at most 1 % undecided in a general-position family, none in a lattice family.  Written by tests/test_fca_exact.py (python,
host) and tests/test_gpu_fca_limits.py (device, one MI355X, with the module's wall time), each run with PDMPC_FCA_EXACT_REPORT=<this
file>; a run replaces its own section.
"""


def write_report(lines, section):
    """Writes `lines` as section `section` of the file PDMPC_FCA_EXACT_REPORT names, if it names one; other sections stay."""
    import os

    path = os.environ.get("PDMPC_FCA_EXACT_REPORT")
    if not path:
        return None
    sections = {}
    if os.path.exists(path):
        name = None
        for line in open(path).read().splitlines():
            if line.startswith("## "):
                name = line[3:]
                sections[name] = []
            elif name is not None and line:
                sections[name].append(line)
    sections[section] = list(lines)
    with open(path, "w") as f:
        f.write(REPORT_HEADER)
        for name in sorted(sections):
            f.write("\n## %s\n%s\n" % (name, "\n".join(sections[name])))
    return path
