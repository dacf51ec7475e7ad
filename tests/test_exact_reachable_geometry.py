"""The reachable-set geometry against exact arithmetic, without a GPU.

The convex overlap (pdmpc_clip_edge), the overlap of two simple polygons (pdmpc_edge_inside_fraction) and the lanelet bounding
(pdmpc_bound_region) are algorithms of this project, and the Python twin, the C++ host twin and the kernels share one header: a
mistake in a rule would be the same mistake three times.  Here the Python twin (pdmpc.reachability) and the host twin (the *_host
calls) meet tests/exact_geometry.py — Sutherland–Hodgman, shoelace and ear clipping in fractions.Fraction, written from the
definitions — on lattice polygons, where collinear edges, shared vertices and touching are the common case, on polygons in general
position, on automaton hulls and on gears at the sizes the ABI declares.

What the families found is pinned here too: edges collinear up to rounding (the two tests of section 2b; pdmpc_orient was added for
them) and the pinched intersection (test_pinched_intersection).  A bounded set must be strictly simple by exact orientation tests,
except where the exact K ∩ L is itself pinched — decided exactly from K and L (reachable_geometry_checks.pinch_vertices) — where it
must have no two edges that cross by more than 64 eps R; the pinched cases are counted and their share is bounded per family.

Tolerance: the project's rule for an overlap area, 1e-9 · max(|ref|, 1e-3 · min(area A, area B)); on a lattice of up to 8 units,
where every cross product is a small integer, 1e-12 absolute as well.  The 1e-3 coupling decision is compared wherever the exact
area is farther from the threshold than that tolerance (asserted: at least 99 % of every family).  Every test prints the worst
error of its families; with PDMPC_EXACT_GEOMETRY_REPORT=<file> the last test writes them into that file's section of this module (profiles/exact_geometry_errors.txt).
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_geometry as X
from reachable_geometry_checks import Decisions, Pinches, bits as _bits, chains_case, check_bounded_set, count_chains, gear_case, pinch_vertices, write_report
from pdmpc import reachability as R
from pdmpc.backend import BackendError, bound_reachable_sets_call, polygon_set_coupling_call, reachable_set_coupling_call
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.mpa import get_mpa

ERRORS = X.Errors()
Z2 = np.zeros(2)


def _report(*families):
    for line in ERRORS.lines():
        if line.startswith("family") or any(line.startswith(f) for f in families):
            print(line)


# ---- 1. convex overlap (overlap_area, pdmpc_clip_edge)


def _sq(x0, y0, x1, y1):
    return [(Fraction(x0), Fraction(y0)), (Fraction(x0), Fraction(y1)), (Fraction(x1), Fraction(y1)), (Fraction(x1), Fraction(y0))]


def _convex_special_cases():
    sq = _sq(0, 0, 2, 2)
    tri = [(Fraction(1), Fraction(2)), (Fraction(0), Fraction(4)), (Fraction(2), Fraction(4))]  # a vertex on the middle of sq's top edge
    return [
        ("identical", sq, list(sq)),
        ("identical, other start", sq, sq[2:] + sq[:2]),
        ("boxes touch", sq, _sq(2, 0, 4, 2)),
        ("corners touch", sq, _sq(2, 2, 3, 3)),
        ("nested", _sq(0, 0, 8, 8), _sq(2, 3, 4, 5)),
        ("nested, shared corner", _sq(0, 0, 8, 8), _sq(0, 0, 4, 5)),
        ("shared edge, same direction", sq, _sq(0, 0, 1, 4)),
        ("shared edge, opposite direction", sq, _sq(-1, 0, 0, 2)),
        ("shared edge part, opposite direction", sq, _sq(-1, 1, 0, 5)),
        ("vertex on an edge from outside", sq, tri),
        ("vertex on an edge from inside", sq, [(Fraction(1), Fraction(2)), (Fraction(2), Fraction(0)), (Fraction(0), Fraction(0))]),
        ("edge through two vertices", sq, [(Fraction(-1), Fraction(-1)), (Fraction(3), Fraction(3)), (Fraction(3), Fraction(-1))]),
    ]


def _overlap_twins(a, b):
    """(area, bit) of the Python twin and of the host twin (the whole coupler: box test included) for one pair"""
    got = R.overlap_area(a, b)
    adj, area = reachable_set_coupling_call([[a], [b]], Z2, Z2, Z2, [1, 2])
    return (got, got > R.COUPLING_AREA_THRESHOLD), (float(area[0, 1]), int(adj[0, 1]))


def test_convex_overlap_against_exact_clipping():
    rng = np.random.default_rng(101)
    cases = []  # (family, lattice of up to 8 units, what, A, B)
    for g, count in ((4, 150), (6, 150), (8, 300), (9, 100), (1000, 100)):
        fam = "convex lattice %d" % g
        for k in range(count):
            unit = 1.0 if k % 3 else 0.125
            cases.append((fam, g <= 8, k, X.convex_lattice(rng, g, unit), X.convex_lattice(rng, g, unit)))
    for name, A, B in _convex_special_cases():
        cases.append(("convex special", True, name, A, B))
    mpa = get_mpa(Config(scenario_type=ScenarioType.commonroad, Hp=8, mpa_type=MpaType.single_speed))
    L = mpa.local_reachable_sets_conv
    for k in range(120):
        a = R.reachable_sets_at_pose(L, rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-3, 3), int(rng.integers(1, mpa.n_trims + 1)))
        b = R.reachable_sets_at_pose(L, rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-3, 3), int(rng.integers(1, mpa.n_trims + 1)))
        q = int(rng.integers(len(a)))
        cases.append(("convex automaton hulls", False, k, X.poly(a[q]), X.poly(b[-1])))
    dec = {}
    positive = 0
    for fam, lattice, what, A, B in cases:
        assert X.is_convex_clockwise(A) and X.is_convex_clockwise(B), (fam, what)
        ref = X.area_convex_simple(A, B)
        assert ref == X.area_convex_simple(B, A), (fam, what)  # (the reference against itself)
        positive += ref > 0
        for P, Q, order in ((A, B, "a, b"), (B, A, "b, a")):
            (gp, bp), (gh, bh) = _overlap_twins(X.arr(P), X.arr(Q))
            tol = X.check_area(ERRORS, fam, "python", gp, ref, P, Q, lattice, (what, order))
            X.check_area(ERRORS, fam, "host", gh, ref, P, Q, lattice, (what, order))
            d = dec.setdefault(fam, Decisions())
            d.check(bp, ref, tol, (fam, what, order, "python"))
            d.check(bh, ref, tol, (fam, what, order, "host"))
    for d in dec.values():
        d.assert_share()
    assert positive > len(cases) // 3, positive
    # the special cases' exact answers, so that the reference is pinned too
    want = [4, 4, 0, 0, 4, 20, 2, 0, 0, 0, 2, 2]
    assert [X.area_convex_simple(A, B) for _, A, B in _convex_special_cases()] == want
    _report("convex")


# ---- 2. simple x simple overlap (polygon_overlap_area, pdmpc_edge_inside_fraction)


def _polygon_twins(a, b):
    got = R.polygon_overlap_area(a, b)
    adj, area = polygon_set_coupling_call([a, b])
    return (got, got > R.COUPLING_AREA_THRESHOLD), (float(area[0, 1]), int(adj[0, 1]))


def _simple_lattice(rng, g, unit=1.0):
    return X.band_lattice(rng, g, unit) if g >= 6 and rng.integers(2) else X.star_lattice(rng, g, unit)


def _general_position(rng, P):
    """P turned, scaled and moved so that nothing is aligned any more; areas of a pair stay well away from 1e-3"""
    return X.moved(P, rng.uniform(-math.pi, math.pi), rng.uniform(0.3, 0.6), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5))


def test_simple_polygon_overlap_against_exact_triangulation():
    rng = np.random.default_rng(202)
    cases = []
    for g, count in ((4, 60), (6, 80), (8, 150), (9, 40), (1000, 40)):
        for k in range(count):
            cases.append(("simple lattice %d" % g, g <= 8, k, _simple_lattice(rng, g), _simple_lattice(rng, g)))
    for k in range(100):
        A, B = _general_position(rng, _simple_lattice(rng, 8)), _general_position(rng, _simple_lattice(rng, 8))
        assert X.is_simple(A) and X.is_simple(B) and X.area(A) > 0 and X.area(B) > 0
        cases.append(("simple general position", False, k, A, B))
    sq = _sq(0, 0, 4, 4)
    notch = [(Fraction(0), Fraction(0)), (Fraction(0), Fraction(4)), (Fraction(2), Fraction(2)), (Fraction(4), Fraction(4)), (Fraction(4), Fraction(0))]
    comb = [(Fraction(x), Fraction(y)) for x, y in ((0, 0), (0, 4), (1, 4), (1, 1), (2, 1), (2, 4), (3, 4), (3, 1), (4, 1), (4, 4), (5, 4), (5, 0))]
    for name, A, B in (("identical", notch, list(notch)), ("shares edges", sq, notch), ("comb in square", sq, comb), ("comb and notch", comb, notch),
                       ("touching from outside", notch, _sq(4, 0, 6, 4)), ("tooth tips on an edge", comb, _sq(0, 4, 5, 6)),
                       ("identical comb", comb, comb[3:] + comb[:3])):
        cases.append(("simple special", True, name, A, B))
    dec = {}
    positive = 0
    for fam, lattice, what, A, B in cases:
        ref = X.area_simple_simple(A, B)
        assert ref == X.area_simple_simple(B, A), (fam, what)
        positive += ref > 0
        for P, Q, order in ((A, B, "a, b"), (B, A, "b, a")):
            (gp, bp), (gh, bh) = _polygon_twins(X.arr(P), X.arr(Q))
            tol = X.check_area(ERRORS, fam, "python", gp, ref, P, Q, lattice, (what, order))
            X.check_area(ERRORS, fam, "host", gh, ref, P, Q, lattice, (what, order))
            d = dec.setdefault(fam, Decisions())
            d.check(bp, ref, tol, (fam, what, order, "python"))
            d.check(bh, ref, tol, (fam, what, order, "host"))
    for d in dec.values():
        d.assert_share()
    assert positive > len(cases) // 3, positive
    _report("simple")


def test_convex_against_simple_overlap_with_both_references():
    rng = np.random.default_rng(303)
    dec = Decisions()
    for k in range(300):
        g = (6, 8, 9)[k % 3]
        K, S = X.convex_lattice(rng, g), _simple_lattice(rng, g)
        if k % 2:
            K, S = _general_position(rng, K), _general_position(rng, S)
            assert X.is_convex_clockwise(K) and X.is_simple(S)
        ref = X.area_convex_simple(K, S)
        assert ref == X.area_simple_simple(S, K) == X.area_simple_simple(K, S), k  # clipping and triangulation agree exactly
        fam = "convex x simple " + ("general position" if k % 2 else "lattice")
        for P, Q in ((K, S), (S, K)):
            (gp, bp), (gh, bh) = _polygon_twins(X.arr(P), X.arr(Q))
            tol = X.check_area(ERRORS, fam, "python", gp, ref, P, Q, k % 2 == 0 and g <= 8, k)
            X.check_area(ERRORS, fam, "host", gh, ref, P, Q, k % 2 == 0 and g <= 8, k)
            dec.check(bp, ref, tol, (k, "python"))
            dec.check(bh, ref, tol, (k, "host"))
    dec.assert_share()
    _report("convex x simple")


# ---- 2b. edges that are collinear up to rounding (pdmpc_orient)


def test_overlap_of_hulls_with_the_same_heading_one_behind_the_other():
    """Two vehicles with the same trim and heading, the second displaced along an edge of the first one's hull: two hull edges are
    collinear up to the rounding of cos, sin and the offsets, the determinants of the orientation tests are +-1e-17.  Before
    pdmpc_orient took such values for 0, about one in sixteen such evaluations missed the tolerance, by up to 3.8e-3 m^2 (the coupling threshold
    is 1e-3 m^2)."""
    mpa = get_mpa(Config(scenario_type=ScenarioType.commonroad, Hp=8, mpa_type=MpaType.single_speed))
    L = mpa.local_reachable_sets_conv
    rng = np.random.default_rng(606)
    dec = Decisions()
    for k in range(100):
        yaw, trim = rng.uniform(-3, 3), int(rng.integers(1, mpa.n_trims + 1))
        x0, y0 = rng.uniform(-2, 2), rng.uniform(-2, 2)
        a = R.reachable_sets_at_pose(L, x0, y0, yaw, trim)[-1]
        e = int(rng.integers(a.shape[1] - 1))
        d = (a[:, e + 1] - a[:, e]) * rng.uniform(0.2, 1.5)
        b = R.reachable_sets_at_pose(L, x0 + d[0], y0 + d[1], yaw, trim)[-1]
        A, B = X.poly(a), X.poly(b)
        ref = X.area_convex_simple(A, B)
        for P, Q in ((A, B), (B, A)):
            for fam, twins in (("convex, same heading", _overlap_twins), ("simple, same heading", _polygon_twins)):
                (gp, bp), (gh, bh) = twins(X.arr(P), X.arr(Q))
                tol = X.check_area(ERRORS, fam, "python", gp, ref, P, Q, False, k)
                X.check_area(ERRORS, fam, "host", gh, ref, P, Q, False, k)
                dec.check(bp, ref, tol, (fam, k, "python"))
                dec.check(bh, ref, tol, (fam, k, "host"))
    dec.assert_share()
    _report("convex, same heading", "simple, same heading")


def test_overlap_of_bounded_sets_that_share_collinear_edges():
    """Vehicles on one spot at yaw 0, their 8- and 12-gons moved by multiples of 1/16 (so edges of different hulls are collinear) and
    cut by gears about their own centres: the bounded sets' edges along those hull edges end in rounded entry and exit points, collinear
    up to 1e-17.  Before pdmpc_orient, the pair of a 12-gon and a neighbour's bounded set gave 2.6242 and, in the other order, 2.6057
    for an exact 2.6095."""
    rng = np.random.default_rng(707)
    n = 24
    x = rng.integers(-4, 5, n) / 16.0
    y = rng.integers(-4, 5, n) / 16.0
    hulls = [X.ngon((8, 12)[int(rng.integers(2))]) for _ in range(n)]
    lan = [None if v % 4 == 0 else X.arr(X.raw_variant(rng, X.gear((8, 12)[v % 2], 0.9, 1.2, 0.0, float(x[v]), float(y[v])))) for v in range(n)]
    sets, _ = bound_reachable_sets_call([[X.arr(h)] for h in hulls], x, y, np.zeros(n), np.arange(1, n + 1), lan, True)
    sets = [s[0] for s in sets]
    P = [X.poly(s) for s in sets]
    fans = [X.fan(P[v], (Fraction(float(x[v])), Fraction(float(y[v])))) for v in range(n)]
    adj_h, area_h = polygon_set_coupling_call(sets)
    adj_p, area_p = R.polygon_set_coupling(sets)
    assert np.array_equal(adj_h, adj_p) and np.array_equal(_bits(area_h), _bits(area_p))
    dec = Decisions()
    for i in range(n):
        for j in range(i + 1, n):
            ref = X.area_simple_simple(P[i], P[j], fans[i])
            tol = X.check_area(ERRORS, "simple, bounded sets on one spot", ("python", "host"), area_h[i, j], ref, P[i], P[j], False, (i, j))
            dec.check(adj_h[i, j], ref, tol, (i, j))
            got = R.polygon_overlap_area(sets[j], sets[i])  # the other order
            X.check_area(ERRORS, "simple, bounded sets on one spot", "python", got, ref, P[j], P[i], False, (j, i))
    dec.assert_share()
    _report("simple, bounded sets")


# ---- 3. bounding (bound_reachable_set, pdmpc_bound_region)


def _bound_twins(Ks, raws):
    """the bounded sets and flags of the Python twin and of the host twin (one call for the batch) for the pairs (Ks[i], raws[i])"""
    py = []
    for K, raw in zip(Ks, raws):
        r, f = R.bound_reachable_sets([X.arr(K)], X.arr(raw))
        py.append((r[0], f[0]))
    n = len(Ks)
    sets, flags = bound_reachable_sets_call([[X.arr(K)] for K in Ks], np.zeros(n), np.zeros(n), np.zeros(n), np.arange(1, n + 1), [X.arr(q) for q in raws], True)
    return py, [(sets[v][0], int(flags[v, 0])) for v in range(n)]


def _check_family(fam, lattice, Ks, raws, pinch_cap):
    py, host = _bound_twins(Ks, raws)
    counts = {0: 0, R.BOUND_RESTORED: 0, R.BOUND_MULTIPLE: 0}
    pinches = Pinches()
    for i, K in enumerate(Ks):
        assert X.arr(X.normalized(raws[i])).tolist() == R.normalize_lanelet_polygon(X.arr(raws[i])).tolist(), (fam, i)
        Ln = X.normalized(raws[i])
        tris = X.triangulate(Ln)
        (rp, fp), (rh, fh) = py[i], host[i]
        if fh == fp and rh.shape == rp.shape and np.array_equal(_bits(rh), _bits(rp)):  # the same bits: one verdict for both
            check_bounded_set(ERRORS, fam, ("python", "host"), rp, fp, K, Ln, lattice, i, tris, pinches=pinches)
        else:
            check_bounded_set(ERRORS, fam, "python", rp, fp, K, Ln, lattice, i, tris, pinches=pinches)
            check_bounded_set(ERRORS, fam, "host", rh, fh, K, Ln, lattice, i, tris)
        counts[fh] += 1
    pinches.assert_share(pinch_cap)
    print(fam, "pinched:", pinches.pinched, "of", pinches.n)
    counts["pinched"] = pinches.pinched
    return counts


def test_bounding_on_the_lattice_of_8_against_exact_clipping():
    rng = np.random.default_rng(404)
    Ks, Ls, raws = [], [], []
    for k in range(1500):
        Ks.append(X.convex_lattice(rng, 8))
        Ls.append(_simple_lattice(rng, 8))
        raws.append(X.raw_variant(rng, Ls[-1]))
    counts = _check_family("bounding lattice 8", True, Ks, raws, 0.1)
    print(counts)
    assert counts[0] >= 750 and counts[R.BOUND_MULTIPLE] >= 100 and counts[R.BOUND_RESTORED] >= 40 and counts["pinched"] >= 5, counts
    _report("bounding lattice 8")


def test_bounding_on_other_lattices_in_general_position_and_on_special_cases():
    rng = np.random.default_rng(505)
    total = {0: 0, R.BOUND_RESTORED: 0, R.BOUND_MULTIPLE: 0}
    for g, count in ((4, 150), (6, 200), (9, 150), (1000, 150)):
        Ks = [X.convex_lattice(rng, g, 0.25 if k % 2 else 1.0) for k in range(count)]
        Ls = [_simple_lattice(rng, g, 0.25 if k % 2 else 1.0) for k in range(count)]
        c = _check_family("bounding lattice %d" % g, g <= 8, Ks, [X.raw_variant(rng, L) for L in Ls], 0.1 if g < 1000 else 0.01)
        for f in total:
            total[f] += c[f]
    Ks, Ls = [], []
    for k in range(300):
        K, L = _general_position(rng, X.convex_lattice(rng, 8)), _general_position(rng, _simple_lattice(rng, 8))
        assert X.is_convex_clockwise(K) and X.is_simple(L)
        Ks.append(K)
        Ls.append(L)
    c = _check_family("bounding general position", False, Ks, [X.raw_variant(rng, L) for L in Ls], 0.0)
    for f in total:
        total[f] += c[f]
    # K and L built on each other: L = K, L ⊂ K with shared edges, K ⊂ L with shared edges, one touching vertex, an L vertex on a K edge
    sq = _sq(0, 0, 4, 4)
    special = [
        (sq, list(sq), 0), (sq, sq[1:] + sq[:1], 0), (sq, _sq(0, 0, 2, 4), 0), (sq, _sq(0, 0, 4, 8), 0), (sq, _sq(-2, 0, 6, 4), 0),
        (sq, _sq(4, 4, 6, 6), R.BOUND_RESTORED), (sq, _sq(4, 0, 6, 4), R.BOUND_RESTORED), (sq, _sq(1, 1, 3, 3), 0), (sq, _sq(-1, -1, 5, 5), 0),
        (sq, [(Fraction(2), Fraction(4)), (Fraction(1), Fraction(6)), (Fraction(3), Fraction(6))], R.BOUND_RESTORED),
        (sq, [(Fraction(2), Fraction(0)), (Fraction(1), Fraction(6)), (Fraction(3), Fraction(6))], 0),
        (sq, [(Fraction(x), Fraction(y)) for x, y in ((-1, 1), (-1, 3), (5, 3), (5, 1), (3, 1), (3, 2), (1, 2), (1, 1))], 0),
        (sq, [(Fraction(x), Fraction(y)) for x, y in ((-1, 0), (-1, 1), (5, 1), (5, 3), (-1, 3), (-1, 4), (6, 4), (6, 0))], R.BOUND_MULTIPLE),
        (sq, [(Fraction(x), Fraction(y)) for x, y in ((-1, -1), (-1, 1), (5, 1), (5, 3), (-1, 3), (-1, 5), (6, 5), (6, -1))], R.BOUND_MULTIPLE),
    ]
    Ks, Ls = [s[0] for s in special], [s[1] for s in special]
    py, host = _bound_twins(Ks, Ls)
    assert [f for _, f in py] == [s[2] for s in special] == [f for _, f in host], [f for _, f in py]
    c = _check_family("bounding special", True, Ks, Ls, 0.0)
    for f in total:
        total[f] += c[f]
    print(total)
    assert total[0] >= 400 and total[R.BOUND_MULTIPLE] >= 10 and total[R.BOUND_RESTORED] >= 100, total
    _report("bounding lattice 4", "bounding lattice 6", "bounding lattice 9", "bounding lattice 1000", "bounding general", "bounding special")


def test_pinched_intersection():
    """A finding of the lattice families, pinned: where a vertex of L lies on ∂K with both its edges inside K, the chain runs on through
    it (pdmpc_geometry.h: e's part ends at t = 1, e + 1's starts at t = 0).  If ∂K comes back to that vertex, the exact K ∩ L is two
    regions that touch in it; the bounded set is their union, flag 0, pinched there — as a point set exactly K ∩ L, but not a simple
    polygon, and with the neighbouring entry point rounded (20/3 here) its edges cross by 7.6e-17.  About 2 in 1 000 lattice cases."""
    K = [(Fraction(0), Fraction(8)), (Fraction(8), Fraction(8)), (Fraction(8), Fraction(2))]
    L = [(Fraction(x), Fraction(y)) for x, y in ((4, 6), (4, 5), (6, 5), (6, 6), (6, 8), (8, 8), (8, 7), (8, 6), (8, 3), (2, 3), (2, 4), (2, 6), (2, 8), (4, 8))]
    assert X.is_simple(L) and X.cross(K[2], K[0], L[1]) == 0  # (4, 5) lies on K's edge (8, 2) -> (0, 8)
    assert pinch_vertices(K, L) == [1]
    py, host = _bound_twins([K], [L])
    for r, f in (py[0], host[0]):
        P = X.poly(r)
        assert f == 0 and X.area_convex_simple(K, L) == Fraction(95, 6) and abs(X.area(P) - Fraction(95, 6)) <= 1e-12
        assert not X.is_simple(P) and not X.has_no_crossing(P) and X.has_no_crossing(P, 1e-15)
        assert P.count(L[1]) == 1


# ---- 4. gears: the sizes the ABI declares


@pytest.mark.parametrize("T,drop,count,thorough", [(8, None, 33, True), (64, None, 257, True), (65, None, 261, True), (128, None, 513, False), (256, 7, 1024, False)])
def test_gear_against_the_aligned_polygon_gives_one_region_of_4t_plus_1_vertices(T, drop, count, thorough):
    K, G = gear_case(T, drop=drop)
    assert X.is_simple(G) and X.area(G) > 0
    centre = (Fraction(0), Fraction(0))
    tris = X.fan(G, centre)
    py, host = _bound_twins([K], [G])
    for twin, (r, f) in (("python", py[0]), ("host", host[0])):
        assert f == 0 and r.shape[1] == count, (twin, f, r.shape)
    assert np.array_equal(_bits(py[0][0]), _bits(host[0][0]))  # the same bits: one verdict for both
    pinches = Pinches()
    check_bounded_set(ERRORS, "bounding gear", ("python", "host"), py[0][0], 0, K, X.normalized(G), False, T, tris, thorough, pinches)
    assert pinches.pinched == 0
    _report("bounding gear")


def test_gear_of_256_teeth_overflows_the_bounded_set_limit_on_the_host_twin():
    K, G = gear_case(256)
    r, f = R.bound_reachable_set(X.arr(K), R.normalize_lanelet_polygon(X.arr(G)))
    assert f == 0 and r.shape[1] == 1025  # one more than PDMPC_BOUNDED_MAX_COLS
    with pytest.raises(BackendError, match="status -4"):
        bound_reachable_sets_call([[X.arr(K)]], [0.0], [0.0], [0.0], [1], [X.arr(G)], True)
    # ... and the same call with one vertex fewer in K is served (the test above), so the limit is exactly 1024


@pytest.mark.parametrize("chains", [1, 2, 63, 64, 65, 255])
def test_gear_with_a_given_number_of_chains(chains):
    K, G = chains_case(chains)
    Ln = X.normalized(G)
    assert X.is_simple(Ln)
    if chains <= 65:  # (above, the vertex count below pins the number of chains; the exact count costs 10 s)
        assert count_chains(K, Ln) == chains, (chains, count_chains(K, Ln))
    tris = X.fan(Ln, (Fraction(0), Fraction(0)))
    py, host = _bound_twins([K], [G])
    for twin, (r, f) in (("python", py[0]), ("host", host[0])):
        assert f == 0 and r.shape[1] == 3 * chains + len(K) + 1, (twin, f, r.shape)
    assert np.array_equal(_bits(py[0][0]), _bits(host[0][0]))
    pinches = Pinches()
    check_bounded_set(ERRORS, "bounding gear chains", ("python", "host"), py[0][0], 0, K, Ln, False, chains, tris, chains < 255, pinches)
    assert pinches.pinched == 0


def test_zz_write_the_error_record():
    """Not a check: writes this module's section of profiles/exact_geometry_errors.txt where PDMPC_EXACT_GEOMETRY_REPORT says (the
    suite's conftest offers no hook for it)."""
    write_report(ERRORS, "python and host twin")
