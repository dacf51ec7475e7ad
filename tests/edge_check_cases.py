"""Case families for the search's edge checks (csrc/edge_checks.hpp), shared by tests/test_exact_edge_checks.py (oracle against exact
arithmetic, CPU) and tests/test_gpu_edge_check_limits.py (device against both).  Operands are (2, n) float arrays as the checks take them.

Every family is a list of operand tuples drawn from a seeded numpy Generator; `judge_*` gives the exact verdicts of a family with the
robustness rule of tests/exact_geometry.py (decided from the exact values alone), and `Tally` keeps what the report records.
"""
import math

import numpy as np

import exact_geometry as X
import problems

NAN = np.full((2, 1), np.nan)
UNIT = 0.25  # the lattice: multiples of 2^-2 within +-8
SPAN = 32  # ... i.e. integers within +-32 times UNIT


def closed(p):
    return np.concatenate([p, p[:, :1]], axis=1)


def columns(*parts):
    parts = [np.asarray(p, dtype=np.float64).reshape(2, -1) for p in parts]
    return np.concatenate(parts, axis=1) if parts else np.zeros((2, 0))


# ---- general position


def random_shape(rng, convex, cols=None, irregular=False):
    """A vehicle-area-like polygon near the origin with `cols` columns (default 5 to 7): closed (the last column repeats the first) from 4
    columns on, three open points or a segment below.  convex: on a circle of one radius; irregular: an affine image of such a polygon
    (still convex, edges and angles of any proportion); neither: a star with a radius per vertex."""
    cols = int(rng.integers(5, 8)) if cols is None else cols
    n = cols - 1 if cols >= 4 else cols
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = np.full(n, rng.uniform(0.1, 0.4)) if (convex or irregular) else rng.uniform(0.1, 0.4, n)
    p = np.stack([rad * np.cos(ang), rad * np.sin(ang)])
    if irregular:
        t = rng.uniform(0, 2 * np.pi)
        turn = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
        p = turn @ np.array([[rng.uniform(0.3, 1.5), rng.uniform(-0.8, 0.8)], [0.0, rng.uniform(0.3, 1.5)]]) @ p
    p = p + rng.uniform(-0.5, 0.5, (2, 1))
    return closed(p) if cols >= 4 else p


def random_soup(rng, cols=None):
    """A NaN-separated obstacle soup as vectorize_all_obstacles.m builds it: one to four stars of 2 to 8 columns, a separator behind each"""
    parts = []
    for _ in range(int(rng.integers(1, 5))):
        c = int(rng.integers(2, 9)) if cols is None else cols
        parts += [random_shape(rng, convex=False, cols=c) + rng.uniform(-0.6, 0.6, (2, 1)), NAN]
    return columns(*parts)


def interx_general(rng, n):
    """(shape, soup): stars of 2 to 8 columns against soups of stars of 2 to 8 columns"""
    return [(random_shape(rng, convex=False, cols=int(rng.integers(2, 9))), random_soup(rng)) for _ in range(n)]


def sat_general(rng, n):
    """(a, b): convex polygons of 2 to 8 columns, regular-like or irregular"""
    out = []
    for _ in range(n):
        a = random_shape(rng, convex=True, cols=int(rng.integers(2, 9)), irregular=bool(rng.integers(2)))
        b = random_shape(rng, convex=True, cols=int(rng.integers(2, 9)), irregular=bool(rng.integers(2))) + rng.uniform(-0.5, 0.5, (2, 1))
        out.append((a, b))
    return out


def _apex_at_edge(rng, a, e, inside):
    """the middle of edge e of the convex polygon a (open points), moved by a hundredth of the edge's length outwards or inwards, and the
    outward unit normal there"""
    m = a.shape[1]
    p0, p1 = a[:, e], a[:, (e + 1) % m]
    d = p1 - p0
    n = np.array([d[1], -d[0]]) / np.hypot(*d)
    if n @ ((p0 + p1) / 2 - a.mean(axis=1)) < 0:
        n = -n
    return (p0 + p1) / 2 + (-0.01 if inside else 0.01) * np.hypot(*d) * n, n


def _open_or_closed(rng, cols):
    """a convex polygon of `cols` columns, 3 to 8: closed, or open with `cols` distinct vertices -> (columns, its open points)"""
    if rng.integers(2) and cols >= 4:
        a = random_shape(rng, convex=True, cols=cols, irregular=bool(rng.integers(2)))
        return a, a[:, :-1]
    a = random_shape(rng, convex=True, cols=cols + 1, irregular=bool(rng.integers(2)))[:, :-1]
    return a, a


def sat_vertex_at_edge(rng, n):
    """(a, b): a triangle b whose apex points at the middle of one edge of the convex polygon a, just outside it or just inside — outside,
    the normal of that one edge is the only axis that separates the two, so every edge of a shape of 3 to 8 columns, open (8 distinct
    vertices) or closed, the closing edge among them, decides cases of its own"""
    out = []
    for q in range(n):
        a, pts = _open_or_closed(rng, 3 + q % 6)
        e = (q // 6) % pts.shape[1] if q % 2 else pts.shape[1] - 1 - (q // 6) % 2  # every edge in turn, and the last two again and again
        apex, nrm = _apex_at_edge(rng, pts, e, inside=bool(rng.integers(2)))
        t = np.array([-nrm[1], nrm[0]])
        h, w = rng.uniform(0.2, 0.5), rng.uniform(0.05, 0.15)
        b = np.stack([apex, apex + h * nrm + w * t, apex + rng.uniform(0.3, 0.6) * h * nrm - w * t], axis=1)  # (a base parallel to the edge would separate as well)
        out.append((a, closed(b) if rng.integers(2) else b))
    return out


def boundary_vertex_at_edge(rng, n):
    """(shape, left, right): a boundary of one segment that ends at the middle of one edge of the shape, just outside or just inside, and
    leaves at a right angle — the same for intersect_lanelet_boundary"""
    out = []
    for q in range(n):
        a, pts = _open_or_closed(rng, 3 + q % 6)
        e = (q // 6) % pts.shape[1] if q % 2 else pts.shape[1] - 1 - (q // 6) % 2
        apex, nrm = _apex_at_edge(rng, pts, e, inside=bool(rng.integers(2)))
        seg = np.stack([apex, apex + rng.uniform(0.3, 1.0) * nrm], axis=1)
        out.append((a, seg[:, ::-1] if rng.integers(2) else seg, np.zeros((2, 0))))
    return out


def boundary_general(rng, n):
    """(shape, left, right): a convex shape of 2 to 8 columns on a wobbling corridor"""
    out = []
    for _ in range(n):
        left, right, _ = problems.corridor(rng, x0=-1.0, x1=1.5, half_width=rng.uniform(0.1, 0.5), n=int(rng.integers(4, 30)), wobble=rng.uniform(0, 0.2))
        out.append((random_shape(rng, convex=True, cols=int(rng.integers(2, 9)), irregular=bool(rng.integers(2))), left, right))
    return out


# ---- the lattice: every operation of InterX is exact in doubles (products stay below 2^25 * 2^-8)


def _lattice_points(rng, n, centre, reach, step=1):
    """n lattice points (integers) within `reach` of `centre`, multiples of `step`, clipped to the lattice's span"""
    p = np.asarray(centre).reshape(2, 1) + rng.integers(-reach // step, reach // step + 1, (2, n)) * step
    return np.clip(p, -SPAN, SPAN)


def _lattice_shape(rng, cols):
    """a closed star (or, below 4 columns, open points) on the even lattice, so that the middle of every edge is a lattice point"""
    n = cols - 1 if cols >= 4 else cols
    c = rng.integers(-8, 9, 2) * 2
    p = _lattice_points(rng, n, c, 12, step=2)
    p = p[:, np.argsort(np.arctan2(p[1] - p[1].mean(), p[0] - p[0].mean()), kind="stable")]
    return closed(p) if cols >= 4 else p


def interx_lattice(rng, n):
    """(shape, soup) on the lattice with touching built in.  Per case one of: nothing special; soup vertices that are shape vertices; a
    soup segment lying on a shape edge (inside it, beyond it, equal to it); a soup end in the middle of a shape edge; zero-length edges in
    both; a soup that runs along the whole shape, backwards."""
    out = []
    for q in range(n):
        s = _lattice_shape(rng, int(rng.integers(2, 9)))
        parts = []
        for _ in range(int(rng.integers(1, 4))):
            parts += [_lattice_points(rng, int(rng.integers(2, 7)), (s[:, :1] + rng.integers(-8, 9, (2, 1))).ravel(), 16), NAN]
        o = columns(*parts)
        kind = q % 6
        e = int(rng.integers(0, s.shape[1] - 1))
        p0, p1 = s[:, e], s[:, e + 1]
        if kind == 1:  # shared vertices
            o[:, 0] = p0
            if not np.isnan(o[0, 2]):
                o[:, 2] = p1
        elif kind == 2:  # a segment on the edge's line: t in halves, inside, at the ends and beyond
            t0, t1 = rng.choice([-1.0, 0.0, 0.5, 1.0, 2.0], 2, replace=False)
            o[:, 0] = np.clip(p0 + t0 * (p1 - p0), -SPAN, SPAN)
            o[:, 1] = np.clip(p0 + t1 * (p1 - p0), -SPAN, SPAN)
        elif kind == 3:  # an end in the middle of an edge
            o[:, 1] = (p0 + p1) / 2
        elif kind == 4:  # zero-length edges
            o = np.insert(o, 1, o[:, 1], axis=1)
            if s.shape[1] < 8:
                s = np.insert(s, e, s[:, e], axis=1)
        elif kind == 5:  # the shape itself, run backwards, as a polyline of the soup: every edge lies on an edge
            o = columns(s[:, ::-1], NAN, o)
        out.append((s * UNIT, o * UNIT))
    return out


def sat_boxes(rng, n):
    """(a, b): axis-aligned boxes with dyadic corners, where the axes and projections are exact: overlapping, touching along an edge, touching
    at a corner, or apart by one lattice step — a third of them touch"""
    out = []
    for q in range(n):
        x0, y0 = (int(v) for v in rng.integers(-24, 8, 2))
        w, h = (int(v) for v in rng.integers(1, 12, 2))
        w2, h2 = (int(v) for v in rng.integers(1, 12, 2))
        kind = q % 6
        if kind == 0:  # anywhere
            u0, v0 = x0 + int(rng.integers(-w2 - 2, w + 3)), y0 + int(rng.integers(-h2 - 2, h + 3))
        elif kind == 1:  # touching along an edge
            u0, v0 = x0 + w, y0 + int(rng.integers(-h2 + 1, h))
        elif kind == 2:  # touching at a corner
            u0, v0 = x0 + w, y0 + h
        elif kind == 3:  # one step apart in x
            u0, v0 = x0 + w + 1, y0 + int(rng.integers(-h2, h + 1))
        elif kind == 4:  # touching from below
            u0, v0 = x0 + int(rng.integers(-w2 + 1, w)), y0 - h2
        else:  # one step apart at the corner
            u0, v0 = x0 - w2 - 1, y0 - h2

        def box(x, y, a, b, start, close):
            p = np.array([[x, x, x + a, x + a], [y, y + b, y + b, y]], dtype=np.float64)  # clockwise
            p = np.roll(p, start, axis=1)
            return (closed(p) if close else p) * UNIT

        out.append((box(x0, y0, w, h, int(rng.integers(4)), bool(rng.integers(2))), box(u0, v0, w2, h2, int(rng.integers(4)), bool(rng.integers(2)))))
    return out


def sat_lattice_pairs(rng, n):
    """(a, b): strictly convex polygons on a lattice of 4 or 8 units (exact_geometry.convex_lattice), the second moved by a random lattice
    offset of up to g + 1 units so that both outcomes occur (about 30 % overlap and 7 % touch); open where they have 8 vertices (a shape has at most 8 columns), else open or closed"""
    out = []
    for _ in range(n):
        g = int(rng.choice([4, 8]))
        a, b = X.arr(X.convex_lattice(rng, g, UNIT)), X.arr(X.convex_lattice(rng, g, UNIT))
        b = b + rng.integers(-g - 1, g + 2, (2, 1)) * UNIT
        out.append(tuple(closed(p) if p.shape[1] < 8 and rng.integers(2) else p for p in (a, b)))
    return out


def boundary_boxes(rng, n):
    """(shape, left, right): an axis-aligned dyadic box between two axis-parallel staircase boundaries, where SAT is exact.  Boundary
    vertices lie on the box's bounding lines in a third of the cases: such a segment passes the filter in front of SAT by equality (the
    filter's `<` is strict), and where it then touches the box, they collide."""
    out = []
    for q in range(n):
        x0, y0 = (int(v) for v in rng.integers(-8, 9, 2))
        w, h = (int(v) for v in rng.integers(1, 9, 2))
        s = np.array([[x0, x0, x0 + w, x0 + w], [y0, y0 + h, y0 + h, y0]], dtype=np.float64)
        s = closed(s) if rng.integers(2) else s
        kind = q % 3
        up = y0 + h + (0 if kind == 1 else int(rng.integers(-1, 4)))  # the left boundary's height over the box: on its top line, or anywhere
        dn = y0 - (0 if kind == 2 else int(rng.integers(-1, 4)))
        xs = np.sort(rng.choice(np.arange(-24, 25), int(rng.integers(2, 7)), replace=False)).astype(np.float64)
        if kind == 1:  # a boundary vertex on the box's right line: the segments on both sides of it meet the filter by equality
            xs[int(rng.integers(len(xs)))] = x0 + w
            xs = np.unique(xs)
            if len(xs) < 2:
                xs = np.array([x0 + w, x0 + w + 3.0])
        left = np.stack([xs, np.full(len(xs), float(up))])
        right = np.stack([xs, np.full(len(xs), float(dn))])
        if kind == 2 and len(xs) > 2:  # a step in the right boundary at a vertex: a vertical segment
            right = np.insert(right, 1, [right[0, 1], dn - 2.0], axis=1)
        out.append((s * UNIT, left * UNIT, right * UNIT))
    return out


# ---- verdicts and records


def distinct_points(p):
    p = np.asarray(p, dtype=np.float64).reshape(2, -1)
    p = p[:, ~np.isnan(p).any(axis=0)]
    return len({(x, y) for x, y in zip(p[0].tolist(), p[1].tolist())})


def judge_interx(cases, lattice=False):
    """exact (crosses, decided) per (shape, soup)"""
    return [X.interx_exact(s, o, 0 if lattice else None) for s, o in cases]


def judge_sat(cases, exact_axes=False, tally=None, family=None):
    """exact (collide, decided) per (a, b); None where an operand has fewer than two distinct points (no valid axis: oracle only).
    With a tally: also records |double gap - exact gap| / (eps R) of every judged pair."""
    out = []
    for a, b in cases:
        if distinct_points(a) < 2 or distinct_points(b) < 2:
            out.append(None)
            continue
        out.append(X.sat_exact(a, b, 0 if exact_axes else None))
        if tally is not None:
            tally.gap(family, a, b)
    return out


def judge_boundary(cases, exact_axes=False):
    out = []
    for s, left, right in cases:
        out.append(None if distinct_points(s) < 2 else X.boundary_exact(s, left, right, 0 if exact_axes else None))
    return out


def compare(name, got, verdicts, cap, tally=None, both=True):
    """`got` (bools: the oracle's or the device's answers) against the exact verdicts: equal on every decided case; at most `cap` of the
    judged cases undecided; each outcome between 5 % and 95 % of all cases.  Returns (judged, undecided)."""
    got = np.asarray(got, dtype=bool)
    judged = [i for i, v in enumerate(verdicts) if v is not None]
    decided = [i for i in judged if verdicts[i][1]]
    wrong = [i for i in decided if bool(got[i]) != verdicts[i][0]]
    if tally is not None:
        tally.count(name, len(verdicts), len(judged), len(judged) - len(decided), len(wrong))
    assert not wrong, "%s: %d decided cases differ from exact arithmetic, first %s" % (name, len(wrong), wrong[:10])
    assert len(judged) - len(decided) <= cap * len(judged), "%s: %d of %d undecided" % (name, len(judged) - len(decided), len(judged))
    if both:
        assert 0.05 < got.mean() < 0.95, "%s: %.3f of the cases are true" % (name, got.mean())
    return len(judged), len(judged) - len(decided)


class Tally(X.Errors):
    """exact_geometry.Errors with the rows of the edge checks: per family the cases, the judged and undecided ones, and for SAT families the
    largest |double gap - exact gap| in units of eps · R (the bound behind the SAT slack is about 14 of them)"""

    def __init__(self):
        super().__init__()
        self.counts = {}

    def count(self, family, cases, judged, undecided, wrong):
        self.counts[family] = (cases, judged, undecided, wrong)

    def gap(self, family, a, b):
        exact = X.sat_gap_exact(a, b)
        R = X.largest_coordinate(a, b)
        if exact is None or R == 0:
            return
        err = abs(X.Fraction(X.sat_gap_double(a, b)) - X.gap_value(exact))
        self.add("edge checks: " + family + ", double gap", "python", err, X.EPS * R)

    def lines(self):
        out = super().lines() if self.rows else []
        out.append("%-58s %8s %8s %10s %8s" % ("edge-check family", "cases", "judged", "undecided", "wrong"))
        for family, row in sorted(self.counts.items()):
            out.append("%-58s %8d %8d %10d %8d" % ((family,) + row))
        return out

    def worst_gap_units(self):
        return max([units for (family, _), (_, _, units) in self.rows.items() if family.endswith("double gap")] + [0.0])
