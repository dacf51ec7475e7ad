"""Exact polygon arithmetic in `fractions.Fraction`: the reference the reachable-set geometry is checked against.

Doubles are exact rationals, so nothing here rounds.  Everything follows from the definitions — Sutherland–Hodgman clipping, the
shoelace formula, ear clipping, orientation tests — and nothing from include/pdmpc_geometry.h or pdmpc.reachability.

A polygon is a list of (Fraction, Fraction) points, open (no repeated closing vertex).  The project's polygons are clockwise, so
`area` is positive for a clockwise polygon.  `poly` converts a (2, m) array (open or closed) and `arr` converts back.
"""
import math
from fractions import Fraction

import numpy as np

AREA_THRESHOLD = Fraction(1e-3)  # ReachableSetCoupler.m:48, the double's value


def poly(a):
    """(2, m) array, open or closed by a repeated first vertex -> list of Fraction points, open."""
    a = np.asarray(a, dtype=np.float64).reshape(2, -1)
    pts = [(Fraction(x), Fraction(y)) for x, y in zip(a[0].tolist(), a[1].tolist())]
    if len(pts) > 1 and pts[0] == pts[-1]:
        pts.pop()
    return pts


def arr(P):
    """list of points -> (2, m) float array (exact if the points are doubles)."""
    return np.array([[float(p[0]) for p in P], [float(p[1]) for p in P]], dtype=np.float64).reshape(2, -1)


def cross(o, a, b):
    """> 0: b lies left of the directed line o -> a."""
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def area(P):
    """Signed area, positive for a clockwise polygon (shoelace)."""
    s = 0
    for i in range(len(P)):
        a, b = P[i], P[(i + 1) % len(P)]
        s += a[0] * b[1] - b[0] * a[1]
    return -Fraction(s) / 2


def is_convex_clockwise(P):
    """strictly convex and clockwise: every vertex a strict right turn"""
    m = len(P)
    return m >= 3 and all(cross(P[i], P[(i + 1) % m], P[(i + 2) % m]) < 0 for i in range(m))


def _line_cut(a, b, p, q):
    """the point where the segment a -> b meets the line p -> q (they are not parallel)"""
    ca, cb = cross(p, q, a), cross(p, q, b)
    t = Fraction(ca) / (ca - cb)
    return (a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]))


def _clip(subject, K):
    """Sutherland–Hodgman on coordinates of any exact type (Fraction or int)"""
    out = list(subject)
    for i in range(len(K)):
        p, q = K[i], K[(i + 1) % len(K)]
        src, out = out, []
        if not src:
            break
        side = [cross(p, q, v) for v in src]  # <= 0: inside (right of a clockwise edge, or on it)
        for j in range(len(src)):
            a, b = src[j], src[(j + 1) % len(src)]
            sa, sb = side[j], side[(j + 1) % len(src)]
            if sa <= 0:
                out.append(a)
                if sb > 0 and sa < 0:
                    out.append(_line_cut(a, b, p, q))
            elif sb < 0:
                out.append(_line_cut(a, b, p, q))
    return out


def _integers(*polys):
    """the polygons on a common integer grid -> (D, polygons with every coordinate multiplied by D): the same exact arithmetic, but on
    Python ints wherever no intersection point is involved, which is an order of magnitude faster than Fraction's"""
    D = math.lcm(1, *{c.denominator for P in polys for p in P for c in p})
    return D, [[(int(p[0] * D), int(p[1] * D)) for p in P] for P in polys]


def clip_convex(subject, K):
    """Sutherland–Hodgman: the simple polygon `subject` clipped by the clockwise convex polygon K.  The shoelace area of the result
    is exactly area(subject ∩ K), also when the intersection falls apart (the bridges along ∂K enclose nothing)."""
    D, (s, k) = _integers(subject, K)
    return [(Fraction(p[0]) / D, Fraction(p[1]) / D) for p in _clip(s, k)]


def area_convex_simple(K, L):
    """area(K ∩ L) for a clockwise convex K and a simple clockwise L"""
    D, (k, l) = _integers(K, L)
    return area(_clip(l, k)) / (D * D)


def _boxes(P):
    x = np.array([float(p[0]) for p in P])
    y = np.array([float(p[1]) for p in P])
    x1, y1 = np.roll(x, -1), np.roll(y, -1)
    return np.minimum(x, x1), np.maximum(x, x1), np.minimum(y, y1), np.maximum(y, y1)


def _on_segment(a, b, p):
    """p on the closed segment a -> b, given that the three are collinear"""
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def _segments_touch(a, b, c, d):
    """the closed segments a -> b and c -> d share a point"""
    o1, o2, o3, o4 = cross(a, b, c), cross(a, b, d), cross(c, d, a), cross(c, d, b)
    if ((o1 > 0) != (o2 > 0)) and o1 != 0 and o2 != 0 and ((o3 > 0) != (o4 > 0)) and o3 != 0 and o4 != 0:
        return True
    return (o1 == 0 and _on_segment(a, b, c)) or (o2 == 0 and _on_segment(a, b, d)) or (o3 == 0 and _on_segment(c, d, a)) or (o4 == 0 and _on_segment(c, d, b))


def _segments_cross(a, b, c, d):
    """the open segments cross in one point interior to both"""
    o1, o2, o3, o4 = cross(a, b, c), cross(a, b, d), cross(c, d, a), cross(c, d, b)
    return o1 != 0 and o2 != 0 and o3 != 0 and o4 != 0 and ((o1 > 0) != (o2 > 0)) and ((o3 > 0) != (o4 > 0))


def _edge_pairs(P):
    """pairs of edges i < j whose boxes meet (the coordinates are doubles, so the float comparison is exact; for points that are not, the
    boxes are widened by a rounding step)"""
    x0, x1, y0, y1 = _boxes(P)
    pad = 0.0 if all(p[0].denominator & (p[0].denominator - 1) == 0 and p[1].denominator & (p[1].denominator - 1) == 0 for p in P) else 1e-9
    m = len(P)
    for i in range(m):
        hit = np.nonzero((x0[i + 1 :] <= x1[i] + pad) & (x1[i + 1 :] >= x0[i] - pad) & (y0[i + 1 :] <= y1[i] + pad) & (y1[i + 1 :] >= y0[i] - pad))[0]
        for j in (hit + i + 1).tolist():
            yield i, j


def is_simple(P):
    """Strictly simple: no zero-length edge, neighbouring edges share their common vertex only, all other edges share nothing."""
    m = len(P)
    if m < 3:
        return False
    for i, j in _edge_pairs(P):
        a, b, c, d = P[i], P[(i + 1) % m], P[j], P[(j + 1) % m]
        if a == b or c == d:
            return False
        if j == i + 1 or (i == 0 and j == m - 1):
            # neighbours: the free end of neither may lie on the other
            s, mid, e = (a, b, d) if j == i + 1 else (c, d, b)
            if cross(s, mid, e) == 0 and (mid[0] - s[0]) * (e[0] - mid[0]) + (mid[1] - s[1]) * (e[1] - mid[1]) < 0:
                return False
        elif _segments_touch(a, b, c, d):
            return False
    return True


def has_no_crossing(P, slack=0.0):
    """Weakly simple, the most the boundary of K ∩ L can promise where L touches ∂K: no two edges cross in a point interior to both.
    slack > 0: a crossing counts only if all four ends lie farther than `slack` from the other edge's line (exactly: cross² against
    slack² · length²) — for polygons whose vertices are rounded intersection points, which at a touching point cross by a rounding
    error."""
    m = len(P)
    s2 = Fraction(slack) ** 2
    for i, j in _edge_pairs(P):
        a, b, c, d = P[i], P[(i + 1) % m], P[j], P[(j + 1) % m]
        if _segments_cross(a, b, c, d):
            lab = (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2
            lcd = (d[0] - c[0]) ** 2 + (d[1] - c[1]) ** 2
            if min(cross(a, b, c) ** 2 / lab, cross(a, b, d) ** 2 / lab, cross(c, d, a) ** 2 / lcd, cross(c, d, b) ** 2 / lcd) > s2:
                return False
    return True


def rounding_slack(*polys):
    """64 · eps · R, R the largest coordinate magnitude: a vertex of a bounded set that is an intersection point is l + t · (l1 − l)
    with t = −num / den, a handful of roundings of at most eps · R each"""
    R = max(max(abs(float(p[0])), abs(float(p[1]))) for P in polys for p in P)
    return 64 * float(np.finfo(np.float64).eps) * R


def triangulate(P):
    """Ear clipping of a strictly simple clockwise polygon -> clockwise triangles.  Checks itself: the triangles' areas sum to the
    polygon's area exactly (an AssertionError otherwise: the input was not what the generator promised)."""
    pts = list(P)
    tris = []
    while len(pts) > 3:
        m = len(pts)
        for i in range(m):
            a, b, c = pts[i - 1], pts[i], pts[(i + 1) % m]
            cr = cross(a, b, c)
            if cr == 0:  # b between a and c (the polygon is simple): no area
                pts.pop(i)
                break
            if cr > 0:  # reflex
                continue
            if any(cross(a, b, p) <= 0 and cross(b, c, p) <= 0 and cross(c, a, p) <= 0 for p in pts if p != a and p != b and p != c):
                continue
            tris.append([a, b, c])
            pts.pop(i)
            break
        else:
            raise AssertionError("no ear: the polygon is not simple")
    if cross(*pts) != 0:
        tris.append(pts)
    assert all(cross(*t) < 0 for t in tris) and sum(area(t) for t in tris) == area(P), "triangulation does not cover the polygon"
    return tris


def fan(P, c):
    """The triangles (c, p_i, p_i+1) of a simple clockwise polygon that is star-shaped about c (asserted: none of them turns the
    other way; with the polygon simple, that is star-shapedness) — the cheap triangulation of gears and of their bounded sets."""
    tris = []
    for i in range(len(P)):
        t = [c, P[i], P[(i + 1) % len(P)]]
        o = cross(*t)
        assert o <= 0, "the polygon is not star-shaped about the centre"
        if o < 0:
            tris.append(t)
    return tris


def area_simple_simple(A, B, triangles=None):
    """area(A ∩ B) of two simple clockwise polygons: the sum over an exact triangulation of A of area(B ∩ triangle)"""
    tris = triangulate(A) if triangles is None else triangles
    D, polys = _integers(B, *tris)
    return sum((area(_clip(polys[0], t)) for t in polys[1:]), Fraction(0)) / (D * D)


def coupled(exact_area):
    """ReachableSetCoupler.m:48 on the exact area"""
    return exact_area > AREA_THRESHOLD


def tolerance(ref, area_a, area_b):
    """the project's rule for an overlap area (tests/test_bounded_reachable_sets.py::_check_area)"""
    return 1e-9 * max(abs(float(ref)), 1e-3 * min(float(area_a), float(area_b)))


def error_unit(A, B):
    """eps · (m_a + m_b) · R², R the largest coordinate magnitude: the unit the observed errors are recorded in"""
    R = max(max(abs(float(p[0])), abs(float(p[1]))) for p in list(A) + list(B))
    return np.finfo(np.float64).eps * (len(A) + len(B)) * max(R * R, 1e-300)


def decision_is_safe(exact_area, tol):
    """the 1e-3 decision is compared only where the exact area is farther from the threshold than the tolerance"""
    return abs(exact_area - AREA_THRESHOLD) > tol


# ---- generators (seeded numpy Generators; lattice coordinates are integers times `unit`, a power of two: exact doubles)


def _hull(points):
    """strict convex hull of integer points, clockwise from the smallest (x, y) (Andrew's monotone chain in integers)"""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h

    lower, upper = half(pts), half(pts[::-1])
    ccw = lower[:-1] + upper[:-1]
    return [ccw[0]] + ccw[:0:-1]


def _scaled(pts, unit, dx=0, dy=0):
    return [(Fraction(p[0] + dx) * Fraction(unit), Fraction(p[1] + dy) * Fraction(unit)) for p in pts]


def convex_lattice(rng, g, unit=1.0, k=None):
    """a strictly convex clockwise polygon on the lattice {0 .. g}²"""
    while True:
        k_ = int(rng.integers(3, 9)) if k is None else k
        h = _hull([(int(rng.integers(0, g + 1)), int(rng.integers(0, g + 1))) for _ in range(k_)])
        if len(h) >= 3:
            P = _scaled(h, unit)
            assert is_convex_clockwise(P)
            return P


def star_lattice(rng, g, unit=1.0, k=None):
    """a simple clockwise polygon on the lattice {0 .. g}²: random lattice points in the order of their angle about an off-lattice
    centre; validated, resampled until simple"""
    cx, cy = g / 2 + 1 / 3, g / 2 + 1 / 5
    while True:
        k_ = int(rng.integers(4, 11)) if k is None else k
        pts = {}
        for _ in range(k_):
            p = (int(rng.integers(0, g + 1)), int(rng.integers(0, g + 1)))
            pts[round(math.atan2(p[1] - cy, p[0] - cx), 9)] = p
        order = [pts[a] for a in sorted(pts, reverse=True)]  # descending angle: clockwise
        P = _scaled(order, unit)
        if len(P) >= 3 and is_simple(P) and area(P) > 0:
            return P


def band_lattice(rng, g, unit=1.0):
    """a lanelet-like simple clockwise polygon on the lattice {0 .. g}² (g >= 6): a band of width w that runs out along one side,
    makes a U-turn and runs back — the left boundary, then the reversed right boundary — with extra collinear vertices and bends
    of one lattice step; turned by a multiple of 90°, mirrored or not; validated, resampled until simple."""
    while True:
        w = int(rng.integers(1, max(2, g // 4 + 1)))
        h = int(rng.integers(2 * w + 1, g + 1))
        a = int(rng.integers(2 * w + 1, g + 1))
        outer = [(0, 0)] + [(x, 0) for x in sorted(set(rng.integers(1, a, 2).tolist()))] + [(a, 0), (a, h)]
        outer += [(x, h) for x in sorted(set(rng.integers(1, a, 2).tolist()), reverse=True)] + [(0, h)]
        inner = [(0, w)] + [(x, w) for x in sorted(set(rng.integers(1, a - w, 1).tolist()))] + [(a - w, w), (a - w, h - w)]
        inner += [(x, h - w) for x in sorted(set(rng.integers(1, a - w, 1).tolist()), reverse=True)] + [(0, h - w)]
        pts = outer + inner[::-1]
        for _ in range(int(rng.integers(0, 3))):  # bends
            i = int(rng.integers(len(pts)))
            pts[i] = (pts[i][0] + int(rng.integers(-1, 2)), pts[i][1] + int(rng.integers(-1, 2)))
        turn, mirror = int(rng.integers(4)), bool(rng.integers(2))
        out = []
        for x, y in pts:
            if mirror:
                x = a - x
            for _ in range(turn):
                x, y = -y, x
            out.append((x, y))
        x0, y0 = min(p[0] for p in out), min(p[1] for p in out)
        out = [(p[0] - x0, p[1] - y0) for p in out]
        sx, sy = g - max(p[0] for p in out), g - max(p[1] for p in out)
        if sx < 0 or sy < 0 or len(set(out)) != len(out):
            continue
        P = _scaled(out, unit, int(rng.integers(0, sx + 1)), int(rng.integers(0, sy + 1)))
        if area(P) < 0:
            P = P[::-1]
        if is_simple(P):
            return P


def moved(P, angle, scale, dx, dy):
    """P turned, scaled and moved in doubles (general position): the result's vertices are the rounded ones, taken as exact"""
    c, s = math.cos(angle), math.sin(angle)
    return [(Fraction(scale * (c * float(x) - s * float(y)) + dx), Fraction(scale * (s * float(x) + c * float(y)) + dy)) for x, y in P]


def _quantized(v, bits):
    return Fraction(round(v * (1 << bits)), 1 << bits)


def ngon(M, radius=1.0, phase=0.0, cx=0.0, cy=0.0, bits=24, rng=None, jitter=0.0):
    """a (near-)regular clockwise M-gon, vertex i at the angle phase − 2πi/M, coordinates on a grid of 2^-bits; strict convexity asserted"""
    P = []
    for i in range(M):
        t = phase - 2 * math.pi * i / M
        r = radius * (1.0 + (jitter * float(rng.uniform(-1, 1)) if rng is not None else 0.0))
        P.append((_quantized(cx + r * math.cos(t), bits), _quantized(cy + r * math.sin(t), bits)))
    assert is_convex_clockwise(P), "the M-gon is not strictly convex at this grid"
    return P


def gear(T, r_in=0.9, r_out=1.2, phase=0.0, cx=0.0, cy=0.0, bits=24):
    """the gear: 2T vertices alternating between the radii r_out (teeth, tooth i at the angle phase − 2πi/T) and r_in (valleys, half
    way between the teeth; one radius, or one per valley), clockwise, on a grid of 2^-bits.  Against the aligned T-gon of radius 1
    every tooth sticks out and every valley below radius 1 lies inside (a valley above it stays outside with its two teeth): one chain
    per deep valley, and with all T of them one region of 4T + 1 vertices (entry, valley, exit and a vertex of the T-gon per tooth, and
    the closing one)."""
    P = []
    for i in range(2 * T):
        t = phase - math.pi * i / T
        r = r_out if i % 2 == 0 else (r_in if isinstance(r_in, float) else r_in[i // 2])
        P.append((_quantized(cx + r * math.cos(t), bits), _quantized(cy + r * math.sin(t), bits)))
    return P

def normalized(raw):
    """the clockwise polygon of a raw lanelet polygon: a vertex equal to the one before it dropped, trailing copies of the first
    dropped, the order reversed if it runs counter-clockwise"""
    P = []
    for p in raw:
        if not P or p != P[-1]:
            P.append(p)
    while len(P) > 1 and P[-1] == P[0]:
        P.pop()
    return P[::-1] if area(P) < 0 else P


def raw_variant(rng, P, mode=None):
    """a raw lanelet polygon whose clockwise polygon is a rotation of P: 0 as it is, 1 counter-clockwise, 2 with repeated
    consecutive vertices and a repeated closing vertex, 3 both"""
    mode = int(rng.integers(4)) if mode is None else mode
    k = int(rng.integers(len(P)))
    Q = P[k:] + P[:k]
    if mode & 1:
        Q = Q[::-1]
    if mode & 2:
        out = []
        for p in Q:
            out += [p] * (1 + int(rng.integers(0, 3) == 0))
        Q = out + [Q[0]] * int(rng.integers(1, 3))
    return Q


def boundary_distance(p, P):
    """distance of the point p from the boundary of P, in doubles (for a check to 1e-9, not an exact statement)"""
    px, py = float(p[0]), float(p[1])
    a = arr(P)
    ax, ay = a[0], a[1]
    dx, dy = np.roll(ax, -1) - ax, np.roll(ay, -1) - ay
    t = np.clip(((px - ax) * dx + (py - ay) * dy) / np.maximum(dx * dx + dy * dy, 1e-300), 0.0, 1.0)
    return float(np.min(np.hypot(ax + t * dx - px, ay + t * dy - py)))


class Errors:
    """the worst observed error per (family, twin): absolute, and in units of eps · (m_a + m_b) · R² — a record, not a threshold"""

    def __init__(self):
        self.rows = {}

    def add(self, family, twin, err, unit):
        if not isinstance(twin, str):
            for t in twin:
                self.add(family, t, err, unit)
            return
        n, worst, units = self.rows.get((family, twin), (0, 0.0, 0.0))
        self.rows[(family, twin)] = (n + 1, max(worst, float(err)), max(units, float(err) / unit))

    def lines(self):
        out = ["%-46s %-8s %8s %12s %10s" % ("family", "twin", "cases", "worst abs", "in units")]
        for (family, twin), (n, worst, units) in sorted(self.rows.items()):
            out.append("%-46s %-8s %8d %12.3e %10.4f" % (family, twin, n, worst, units))
        return out


def check_area(errors, family, twin, got, ref, A, B, lattice=False, what=None):
    """the project's tolerance on one area (and 1e-12 absolute on a lattice of up to 8 units); records the error; returns the tolerance"""
    tol = tolerance(ref, area(A), area(B))
    err = abs(Fraction(float(got)) - ref)
    errors.add(family, twin, err, error_unit(A, B))
    assert err <= tol, (family, twin, what, float(got), float(ref), float(err), tol)
    if lattice:
        assert err <= 1e-12, (family, twin, what, float(got), float(ref), float(err))
    return tol


# ---- the search's edge checks (csrc/edge_checks.hpp: InterX, intersect_sat, intersect_lanelet_boundary) from the definitions.
# Operands are (2, n) arrays of doubles as the checks take them (a soup may hold NaN columns).  Doubles are dyadic rationals: all of a case's
# coordinates are put on one integer grid (a power of two times each), and everything below is Python-integer arithmetic, which is exact.

EPS = float(np.finfo(np.float64).eps)


def _grid(*arrays):
    """(2, n) arrays -> lists of integer points on a common grid (None for a column with a NaN), the same order"""
    den = 1
    for a in arrays:
        for v in np.asarray(a, dtype=np.float64).ravel().tolist():
            if v == v:
                den = max(den, v.as_integer_ratio()[1])
    out = []
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).reshape(2, -1)
        pts = []
        for x, y in zip(a[0].tolist(), a[1].tolist()):
            if x != x or y != y:
                pts.append(None)
            else:
                nx, dx = x.as_integer_ratio()
                ny, dy = y.as_integer_ratio()
                pts.append((nx * (den // dx), ny * (den // dy)))
        out.append(pts)
    return den, out


def largest_coordinate(*arrays):
    """R: the largest |coordinate| of the operands, NaN left out"""
    return max([float(np.nanmax(np.abs(a))) for a in arrays if np.size(a) and not np.all(np.isnan(a))] + [0.0])


def interx_slack(*arrays):
    """64 · eps · R² on an orientation value dx·(y − y0) − dy·(x − x0): four products and three differences of numbers up to 2R, each
    rounding at most eps/2 of a magnitude of at most 4R², with a factor of margin"""
    R = largest_coordinate(*arrays)
    return 64 * EPS * R * R


def sat_slack(*arrays):
    """32 · eps · R on the normalised gap of two projections: sum of squares, root, quotient, two products, sum and difference bound the
    error by about 14 · eps · R; the rest is margin"""
    return 32 * EPS * largest_coordinate(*arrays)


def proper_crossing(a, b, c, d):
    """The segments a -> b and c -> d cross properly: both ends of each lie strictly on opposite sides of the other (InterX.m:63-76 with
    `< 0`).  Touching, a shared vertex and collinear overlap are no crossing."""
    return _segments_cross(a, b, c, d)


def interx_exact(shape, soup, slack=None):
    """InterX of the polyline `shape` and the polyline soup `soup` (NaN columns end a polyline) -> (crosses, decided).
    decided: double arithmetic cannot change the answer.  A (shape edge, soup segment) pair is robust if all four orientation values exceed
    the slack in magnitude, or if one of the two sign tests has both values beyond the slack with equal sign (no crossing, whatever the other
    test says); the case is decided if some pair robustly crosses or every pair is robust and none crosses.  slack = 0 (a lattice where
    every operation is exact in doubles): always decided.  slack None: interx_slack of the operands."""
    if slack is None:
        slack = interx_slack(shape, soup)
    den, (P, Q) = _grid(shape, soup)
    s = Fraction(slack) * den * den  # the orientation values below are den² times the real ones
    crosses, all_robust, robust_cross = False, True, False
    for i in range(len(P) - 1):
        a, b = P[i], P[i + 1]
        if a is None or b is None:
            continue
        for j in range(len(Q) - 1):
            c, d = Q[j], Q[j + 1]
            if c is None or d is None:
                continue
            o1, o2, o3, o4 = cross(a, b, c), cross(a, b, d), cross(c, d, a), cross(c, d, b)
            hit = ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0))
            crosses = crosses or hit
            if slack == 0:
                continue
            big = [abs(o) > s for o in (o1, o2, o3, o4)]
            if all(big):
                robust_cross = robust_cross or hit
            elif not ((big[0] and big[1] and (o1 > 0) == (o2 > 0)) or (big[2] and big[3] and (o3 > 0) == (o4 > 0))):
                all_robust = False
    return crosses, (slack == 0 or robust_cross or (all_robust and not crosses))


def _open(pts):
    """the points of a polygon without a repeated closing vertex"""
    return pts[:-1] if len(pts) > 1 and pts[0] == pts[-1] else pts


def _gap_on_grid(P, Q):
    """the largest normalised gap over the edge normals of P and Q as (sign, g², |n|²): the gap is sign · sqrt(g² / |n|²); None without a
    valid axis (fewer than two distinct points in both)"""
    best = None
    for poly_ in (P, Q):
        m = len(poly_)
        for i in range(m):
            a, b = poly_[i], poly_[(i + 1) % m]
            nx, ny = -(b[1] - a[1]), b[0] - a[0]
            n2 = nx * nx + ny * ny
            if n2 == 0:
                continue
            dp = [nx * p[0] + ny * p[1] for p in P]
            dq = [nx * p[0] + ny * p[1] for p in Q]
            g = max(min(dp) - max(dq), min(dq) - max(dp))
            key = (1 if g > 0 else -1 if g < 0 else 0, g * g, n2)
            if best is None or _gap_less(best, key):
                best = key
    return best


def _gap_less(u, v):
    """sign_u · g_u² / n_u² < sign_v · g_v² / n_v², in integers"""
    return u[0] * u[1] * v[2] < v[0] * v[1] * u[2]


def sat_gap_exact(a, b):
    """The exact normalised gap of the polygons a and b ((2, n) arrays, closed or open): for every edge normal of both, the gap between the
    two projections, max(min_a − max_b, min_b − max_a) / |n|; the largest of them.  The polygons are separate iff it is > 0 (touching
    collides).  -> (sign, squared gap as a Fraction), or None if neither has two distinct points.  A segment is a two-point polygon."""
    den, (P, Q) = _grid(a, b)
    best = _gap_on_grid(_open(P), _open(Q))
    if best is None:
        return None
    return best[0], Fraction(best[1], best[2] * den * den)


def gap_value(gap, bits=200):
    """the signed gap of sat_gap_exact as a Fraction good to `bits` bits (the root is the only inexact step)"""
    sign, sq = gap
    num, den = sq.numerator << (2 * bits), sq.denominator
    return sign * Fraction(math.isqrt(num // den), 1 << bits)


def sat_exact(a, b, slack=None):
    """intersect_sat(a, b) -> (collide, decided): collide iff the exact gap is <= 0, decided iff |gap| > slack (sat_slack by default;
    slack = 0, for operands whose axes and projections are exact in doubles: always decided, touching included)"""
    if slack is None:
        slack = sat_slack(a, b)
    sign, sq = sat_gap_exact(a, b)
    return sign <= 0, slack == 0 or sq > Fraction(slack) ** 2


def sat_soup_exact(a, soup, slack=None):
    """any(intersect_sat(a, polygon)) over the polygons of a NaN-separated soup (polygons of one point have no axis of their own and are the
    caller's to leave out) -> (collide, decided): decided if some polygon collides beyond the slack or every polygon is decided"""
    if slack is None:
        slack = sat_slack(a, soup)
    collide, all_decided, robust = False, True, False
    for q in split_soup(soup):
        c, d = sat_exact(a, q, slack)
        collide, all_decided, robust = collide or c, all_decided and d, robust or (c and d)
    return collide, robust or all_decided


def boundary_exact(shape, left, right, slack=None):
    """intersect_lanelet_boundary(shape, left, right) for a convex shape -> (collide, decided): some boundary segment (two real points in a
    row) and the shape have a gap <= 0.  The bounding-box filter in front of it changes nothing in exact arithmetic: a segment strictly
    beyond a side of the box is separate from the shape, and the edge normals of a convex polygon and a segment are a complete set of axes."""
    if slack is None:
        slack = sat_slack(shape, left, right)
    collide, all_decided, robust = False, True, False
    for side in (left, right):
        side = np.asarray(side, dtype=np.float64).reshape(2, -1)
        for j in range(side.shape[1] - 1):
            seg = side[:, j : j + 2]
            if np.isnan(seg).any():
                continue
            c, d = sat_exact(shape, seg, slack)
            collide, all_decided, robust = collide or c, all_decided and d, robust or (c and d)
    return collide, robust or all_decided


def split_soup(soup):
    """the polygons of a NaN-separated soup, in order, empty ones (two separators in a row) left out"""
    soup = np.asarray(soup, dtype=np.float64).reshape(2, -1)
    out, start = [], 0
    nan = np.isnan(soup[0])
    for j in range(soup.shape[1] + 1):
        if j == soup.shape[1] or nan[j]:
            if j > start:
                out.append(soup[:, start:j])
            start = j + 1
    return out


def sat_gap_double(a, b):
    """The same largest gap in double arithmetic, operation by operation as intersect_sat.m:19-34 (Python floats are IEEE doubles and
    math.sqrt rounds correctly) — to record how far doubles stray from the exact gap, not to decide anything."""
    a = np.asarray(a, dtype=np.float64).reshape(2, -1)
    b = np.asarray(b, dtype=np.float64).reshape(2, -1)
    best = None
    for p in (a, b):
        m = p.shape[1]
        for i in range(m):
            k = 0 if i + 1 == m else i + 1
            ax, ay = -(float(p[1, k]) - float(p[1, i])), float(p[0, k]) - float(p[0, i])
            nrm = math.sqrt(ax * ax + ay * ay)
            if nrm == 0:
                continue
            nx, ny = ax / nrm, ay / nrm
            da = [nx * x + ny * y for x, y in zip(a[0].tolist(), a[1].tolist())]
            db = [nx * x + ny * y for x, y in zip(b[0].tolist(), b[1].tolist())]
            g = max(min(da) - max(db), min(db) - max(da))
            best = g if best is None or g > best else best
    return best
