"""The search's edge checks on the device at their kernels' limits (csrc/edge_checks.hpp through pdmpc_debug_edge_check,
pdmpc_debug_interx_soups and pdmpc_debug_sincos), one wavefront per case.

Every case asserts two things.  The device equals the oracle, and its code is 0 or 1, never 2 or 3: the wave-wide form (a lane per segment
or axis: interx_check, sat_pair_wave, sat_soup_wave, sat_boundary_wave) and the per-lane form of the graph search's check items
(interx_segment_n, sat_pair_lane, sat_boundary_segment_lane) agree.  Where exact arithmetic decides the case (tests/exact_geometry.py, the
rule of tests/test_exact_edge_checks.py), the device equals the exact answer.

Besides that module's families: shapes of 2, 3, 7 and 8 columns against second operands of 0 to 1024 columns, one decisive segment or
polygon at every position around the 64-lane rounds, NaN separators at the rounds' ends, all three soups of the InterX check with the
only crossing in each in turn, the smallest lanelet boundaries, and the refusals of sizes outside the declared ones.  The last part holds
the device compile of pdmpc_sincos to the host compile's bits.  With PDMPC_EXACT_GEOMETRY_REPORT=<file> the last test writes this module's
section of profiles/exact_geometry_errors.txt."""
import numpy as np
import pytest

from pdmpc.backend import BackendError, Handle

import edge_check_cases as E
import exact_geometry as X
import problems
import sincos_cases as S
from reachable_geometry_checks import write_report

pytestmark = pytest.mark.gpu

TALLY = E.Tally()
EMPTY = np.zeros((2, 0))
NAN = E.NAN
SHAPE_COLUMNS = (2, 3, 7, 8)
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024)
INTERX, SAT, BOUNDARY, SAT_SOUP = 0, 1, 2, 3


@pytest.fixture(scope="module")
def handle():
    options = problems.make_options("interx", Hp=6)
    options.max_vehicles = 4
    options.max_nodes = 1 << 12
    h = Handle(options)
    yield h
    h.close()


# ---- the oracle's side, composed from its three calls, and the exact side


def oracle_answer(mode, a, b):
    from oracle import oracle

    if mode == INTERX:
        return oracle.interx(a, b)
    if mode == SAT:
        return oracle.intersect_sat(a, b)
    if mode == BOUNDARY:  # every run of real points is a boundary of its own (left and right are such runs)
        return any(oracle.intersect_lanelet_boundary(a, run, EMPTY) for run in X.split_soup(b))
    return any(oracle.intersect_sat(a, q) for q in X.split_soup(b))


def exact_answer(mode, a, b, exact_ops=False):
    """(answer, decided), or None where an operand has fewer than two distinct points"""
    slack = 0 if exact_ops else None
    if mode == INTERX:
        return X.interx_exact(a, b, slack)
    if E.distinct_points(a) < 2:
        return None
    if mode == SAT:
        return None if E.distinct_points(b) < 2 else X.sat_exact(a, b, slack)
    if mode == BOUNDARY:
        return X.boundary_exact(a, b, EMPTY, slack)
    if any(E.distinct_points(q) < 2 for q in X.split_soup(b)):
        return None
    return X.sat_soup_exact(a, b, slack)


def run(handle, name, mode, cases, cap=0.01, exact=True, exact_ops=False, both=True):
    """device == oracle on every case, codes 0 / 1 only; device == exact where decided (E.compare: caps and both outcomes)"""
    codes = handle.edge_check_raw(mode, [a for a, _ in cases], [b for _, b in cases])
    assert ((codes == 0) | (codes == 1)).all(), "%s: the wave-wide and the per-lane form disagree in cases %s" % (name, np.flatnonzero(codes > 1)[:10])
    want = np.array([oracle_answer(mode, a, b) for a, b in cases], dtype=bool)
    assert np.array_equal(codes == 1, want), "%s: device != oracle in cases %s" % (name, np.flatnonzero((codes == 1) != want)[:10])
    if exact:
        E.compare(name, codes == 1, [exact_answer(mode, a, b, exact_ops) for a, b in cases], cap, TALLY, both)
    elif both:
        assert 0.05 < want.mean() < 0.95, (name, want.mean())
    return codes == 1


def boundary_soup(left, right):
    return E.columns(left, NAN, right, NAN)


# ---- refusals


def test_sizes_outside_the_declared_ones_are_refused(handle):
    nine, big = np.zeros((2, 9)), np.zeros((2, 1025))
    ok, soup = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.zeros((2, 1024))
    for mode in (INTERX, SAT, BOUNDARY, SAT_SOUP):
        for a, b in ((nine, ok), (ok, big)):
            with pytest.raises(BackendError) as e:
                handle.edge_check_raw(mode, [ok, a], [ok, b])
            assert e.value.status == -1  # PDMPC_ERR_INVALID
        assert handle.edge_check_raw(mode, [ok[:, :2]] * 2, [ok, soup]).shape == (2,)  # ... and the largest declared one is served
    for mode in (-1, 4):
        with pytest.raises(BackendError) as e:
            handle.edge_check_raw(mode, [ok], [ok])
        assert e.value.status == -1
    with pytest.raises(BackendError) as e:
        handle.interx_soups([nine], [nine], [(ok, ok, ok)])
    assert e.value.status == -1
    with pytest.raises(BackendError) as e:
        handle.interx_soups([ok], [ok], [(np.zeros((2, 400)), np.zeros((2, 400)), np.zeros((2, 225)))])
    assert e.value.status == -1
    assert handle.interx_soups([ok], [ok], [(np.zeros((2, 400)), np.zeros((2, 400)), np.zeros((2, 224)))]).tolist() == [0]


# ---- the families of tests/test_exact_edge_checks.py on the device, and ten times as many cases against the oracle alone


def test_interx_families(handle):
    run(handle, "device interx lattice", INTERX, E.interx_lattice(np.random.default_rng(21), 1500), 0.0, exact_ops=True)
    run(handle, "device interx general position", INTERX, E.interx_general(np.random.default_rng(22), 1000))
    run(handle, "interx, oracle only", INTERX, E.interx_general(np.random.default_rng(23), 6000) + E.interx_lattice(np.random.default_rng(24), 4000), exact=False)


def test_sat_families(handle):
    run(handle, "device sat boxes", SAT, E.sat_boxes(np.random.default_rng(25), 900), 0.0, exact_ops=True)
    run(handle, "device sat lattice pairs", SAT, E.sat_lattice_pairs(np.random.default_rng(26), 900), 0.10)
    run(handle, "device sat general position", SAT, E.sat_general(np.random.default_rng(27), 900))
    more = E.sat_general(np.random.default_rng(28), 6000) + E.sat_lattice_pairs(np.random.default_rng(29), 2000) + E.sat_boxes(np.random.default_rng(30), 2000)
    run(handle, "sat, oracle only", SAT, more, exact=False)


def test_lanelet_boundary_families(handle):
    general = [(s, boundary_soup(left, right)) for s, left, right in E.boundary_general(np.random.default_rng(31), 600)]
    boxes = [(s, boundary_soup(left, right)) for s, left, right in E.boundary_boxes(np.random.default_rng(32), 900)]
    run(handle, "device lanelet boundary general position", BOUNDARY, general)
    run(handle, "device lanelet boundary boxes", BOUNDARY, boxes, 0.0, exact_ops=True)
    more = [(s, boundary_soup(left, right)) for s, left, right in E.boundary_general(np.random.default_rng(33), 5000) + E.boundary_boxes(np.random.default_rng(34), 3000)]
    run(handle, "lanelet boundary, oracle only", BOUNDARY, more, exact=False)


def test_every_edge_of_the_shape_decides(handle):
    """a vertex of the other operand at the middle of one edge of the shape, just outside or inside: that edge's normal alone separates —
    for every edge of shapes of 3 to 8 columns, open (8 distinct vertices: the last register of sat_pick) or closed"""
    run(handle, "device sat vertex at an edge", SAT, E.sat_vertex_at_edge(np.random.default_rng(36), 1200))
    run(handle, "device sat soup vertex at an edge", SAT_SOUP, [(a, E.columns(NAN, b, NAN)) for a, b in E.sat_vertex_at_edge(np.random.default_rng(37), 600)])
    cases = [(s, boundary_soup(left, right)) for s, left, right in E.boundary_vertex_at_edge(np.random.default_rng(38), 1200)]
    run(handle, "device lanelet boundary vertex at an edge", BOUNDARY, cases)


def test_degenerate_operands(handle):
    """one point, one point repeated, a shape of two equal columns: no exact verdict, the device follows the oracle"""
    rng = np.random.default_rng(35)
    single, soups = [], []
    for _ in range(400):
        s = E.random_shape(rng, convex=True, cols=int(rng.integers(2, 9)))
        p = s.mean(axis=1, keepdims=True) + rng.uniform(-0.5, 0.5, (2, 1))
        single += [(s, p), (s, np.repeat(p, 3, axis=1)), (np.repeat(p, 2, axis=1), s)]
        soups += [(s, E.columns(p, NAN, p + 0.01, NAN)), (s, E.columns(NAN, p)), (s, E.columns(p + 5.0, NAN, NAN, np.repeat(p, 2, axis=1)))]
    assert all(exact_answer(SAT, a, b) is None for a, b in single) and all(exact_answer(SAT_SOUP, a, b) is None for a, b in soups)
    run(handle, "degenerate", SAT, single, exact=False)
    run(handle, "degenerate", SAT_SOUP, single + soups, exact=False)
    run(handle, "degenerate", INTERX, single + soups, exact=False, both=False)


# ---- every shape size against every size of the second operand


def soup_of_size(rng, nb, convex, reach):
    """exactly nb columns: polygons of 2 to 8 columns (now and then one of 65 to 200: it straddles a round of 64), a separator behind each,
    cut off at nb — so the last polygon may lack its separator or its last columns"""
    parts, n = [], 0
    while n < nb:
        if rng.integers(12) == 0:
            m = int(rng.integers(65, 201))
            t = -np.linspace(0, 2 * np.pi, m, endpoint=False)
            p = rng.uniform(0.1, 0.4) * np.stack([np.cos(t), np.sin(t)]) + rng.uniform(-0.5, 0.5, (2, 1))
        else:
            p = E.random_shape(rng, convex=convex, cols=int(rng.integers(2, 9)), irregular=convex and bool(rng.integers(2)))
        parts += [p + rng.uniform(-reach, reach, (2, 1)), NAN]
        n += p.shape[1] + 1
    return E.columns(*parts)[:, :nb]


@pytest.mark.parametrize("mode", [INTERX, BOUNDARY, SAT_SOUP])
def test_every_shape_size_against_every_operand_size(handle, mode):
    rng = np.random.default_rng(40 + mode)
    cases = []
    for cols in SHAPE_COLUMNS:
        for nb in SIZES:
            for rep in range(8):
                s = E.random_shape(rng, convex=mode != INTERX, cols=cols, irregular=mode != INTERX and rep % 2 == 1)
                reach = 0.8 + 0.35 * np.sqrt(nb / 4.0) * rng.uniform(0.7, 1.6)  # as many polygons per area at every size
                o = soup_of_size(rng, nb, mode != INTERX, reach)
                if mode == BOUNDARY and nb > 2:  # a boundary is polylines: far fewer separators
                    o[:, np.flatnonzero(np.isnan(o[0]))[1::2]] = o[:, np.flatnonzero(np.isnan(o[0]))[1::2] - 1] + 0.01
                assert o.shape[1] == nb
                cases.append((s, o))
    got = run(handle, "device %s, every size" % ("interx", "", "lanelet boundary", "sat soup")[mode], mode, cases, both=False)
    by_size = got.reshape(len(SHAPE_COLUMNS), len(SIZES), 8)
    assert not by_size[:, 0].any() and (mode == SAT_SOUP or not by_size[:, 1].any())  # nothing to hit in 0 columns, or in 1 but for a polygon of one point
    for i, nb in enumerate(SIZES[3:]):
        assert 0.05 < by_size[:, 3 + i].mean() < 0.95, (nb, by_size[:, 3 + i].mean())


def test_one_polygon_of_every_size(handle):
    """intersect_sat against one convex polygon of 1 to 1024 columns: sat_pair_wave's rounds over V1 + V2 axes"""
    rng = np.random.default_rng(44)
    cases = []
    for cols in SHAPE_COLUMNS:
        for nb in SIZES[2:]:
            for rep in range(6 if nb < 1000 else 2):  # (the exact gap of a 1024-gon is a million integer products)
                s = E.random_shape(rng, convex=True, cols=cols, irregular=rep % 2 == 1)
                t = rng.uniform(0, 2 * np.pi) - np.linspace(0, 2 * np.pi, nb, endpoint=False)
                r = rng.uniform(0.3, 0.6)
                centre = s.mean(axis=1, keepdims=True) + (r + rng.uniform(-0.3, 0.5)) * np.array([[np.cos(t[0])], [np.sin(t[0])]])
                cases.append((s, r * np.stack([np.cos(t), np.sin(t)]) + centre))
    run(handle, "device sat, one polygon of every size", SAT, cases)


# ---- one decisive element at every position


def far_polyline(n, direction, k0=0):
    """n columns far away in `direction` (a unit vector along an axis): a zigzag whose segments are a hundred shapes away"""
    k = np.arange(k0, k0 + n, dtype=np.float64)
    u = np.asarray(direction, dtype=np.float64).reshape(2, 1)
    perp = np.array([[-u[1, 0]], [u[0, 0]]])
    return 100.0 * u + perp * (k * 0.03125 - 10.0) + u * (0.5 * (k % 2))


def across_first_edge(s, reach=1.0):
    """a segment that crosses the shape's first edge in its middle, at a right angle, `reach` to either side (1.0: more than the widest
    shape of random_shape, so both ends lie outside)"""
    p0, p1 = s[:, 0], s[:, 1]
    d = (p1 - p0) / np.hypot(*(p1 - p0))
    n = np.array([-d[1], d[0]])
    m = (p0 + p1) / 2
    return np.stack([m - reach * n, m + 1.01 * reach * n], axis=1)


def positions(count):
    return sorted({j for j in (0, 1, 62, 63, 64, 65, count - 2, count - 1) if 0 <= j < count})


def with_decisive_segment(mode, s, nb, j):
    """A polyline of nb columns, all far away but segment j, which crosses the shape — and its neighbours j - 1 and j + 1, which lead
    there and back, do not: the far end lies in the first of four directions for which exact arithmetic says so."""
    q = across_first_edge(s)
    for direction in ((-1, 0), (1, 0), (0, 1), (0, -1)):
        o = far_polyline(nb, direction)
        o[:, j : j + 2] = q
        near = [exact_answer(mode, s, o[:, k : k + 2]) for k in range(max(j - 1, 0), min(j + 2, nb - 1))]
        if all(d for _, d in near) and [h for h, _ in near] == [k == j for k in range(max(j - 1, 0), min(j + 2, nb - 1))]:
            return o, far_polyline(nb, direction)
    raise AssertionError("no direction keeps the neighbours of segment %d clear" % j)


@pytest.mark.parametrize("mode", [INTERX, BOUNDARY])
def test_one_decisive_segment_at_every_position(handle, mode):
    """exactly one segment of the second operand, at position j, crosses the shape; the same operand without it is the control"""
    rng = np.random.default_rng(50 + mode)
    hits, controls = [], []
    for cols in SHAPE_COLUMNS:
        for nb in SIZES[2:]:
            s = E.random_shape(rng, convex=mode != INTERX, cols=cols)
            for j in positions(nb - 1):
                o, control = with_decisive_segment(mode, s, nb, j)
                hits.append((s, o))
            controls.append((s, control))
    assert run(handle, "device %s, one decisive segment" % ("interx" if mode == INTERX else "lanelet boundary"), mode, hits, 0.0, both=False).all()
    assert not run(handle, "device %s, no decisive segment" % ("interx" if mode == INTERX else "lanelet boundary"), mode, controls, 0.0, both=False).any()


def sat_soup_with_decisive_polygon(s, nb, t, hit=True):
    """nb columns of far segments, a separator behind each, and one triangle beginning at column t: about the shape's middle (it overlaps a
    convex shape) or, for the control, far away as well.  Columns that fit no whole segment are separators (two or three in a row)."""
    o = np.full((2, nb), np.nan)
    far = far_polyline(nb, (1, 0))
    c = s[:, :-1].mean(axis=1, keepdims=True) if s.shape[1] >= 4 else s.mean(axis=1, keepdims=True)
    tri = c + 0.05 * np.array([[0.0, 1.0, -1.0], [1.0, -0.6, -0.7]])
    o[:, t : t + 3] = tri if hit else far[:, t : t + 3] + np.array([[0.0, 3.0, 0.0], [0.0, 0.0, 0.0]])
    for a in range(t - 3, -1, -3):  # [segment, NaN] in front of it, from its separator backwards
        o[:, a : a + 2] = far[:, a : a + 2]
    for a in range(t + 4, nb - 1, 3):  # ... and behind it; a last segment may end the soup without a separator
        o[:, a : a + 2] = far[:, a : a + 2]
    return o


def test_one_decisive_polygon_at_every_position(handle):
    rng = np.random.default_rng(53)
    hits, controls = [], []
    for cols in SHAPE_COLUMNS:
        for nb in SIZES[3:]:
            s = E.random_shape(rng, convex=True, cols=cols, irregular=True)
            for t in sorted({t for t in (0, 1, 62, 63, 64, 65, nb - 4, nb - 3) if 0 <= t <= nb - 3}):
                hits.append((s, sat_soup_with_decisive_polygon(s, nb, t)))
                if t in (0, 63, nb - 3):
                    controls.append((s, sat_soup_with_decisive_polygon(s, nb, t, hit=False)))
    assert len(X.split_soup(hits[-1][1])) > 300 and hits[-1][1].shape[1] == 1024
    assert run(handle, "device sat soup, one decisive polygon", SAT_SOUP, hits, 0.0, both=False).all()
    assert not run(handle, "device sat soup, no decisive polygon", SAT_SOUP, controls, 0.0, both=False).any()


# ---- NaN separators at the rounds' ends


SEPARATORS = ((), (0,), (63,), (64,), (65,), (129,), (0, 1), (63, 64), (64, 65), (62, 63, 64), (128, 129), (0, 64, 129), (100,), (31, 95))


@pytest.mark.parametrize("mode", [INTERX, SAT_SOUP])
def test_separators_at_the_ends_of_a_round(handle, mode):
    """a convex 130-gon near the shape, cut by separators at columns 0, 63, 64, 65 and the last, two and three in a row, none at all (one
    polygon of 130 columns, which straddles two rounds of the ballot) and none at the end"""
    rng = np.random.default_rng(60 + mode)
    cases = []
    for cols in SHAPE_COLUMNS:
        for seps in SEPARATORS:
            for rep in range(6):
                s = E.random_shape(rng, convex=True, cols=cols, irregular=rep % 2 == 1)
                t = rng.uniform(0, 2 * np.pi) - np.linspace(0, 2 * np.pi, 130, endpoint=False)
                t0 = rng.uniform(0, 2 * np.pi)
                o = 0.5 * np.stack([np.cos(t), np.sin(t)]) + s.mean(axis=1, keepdims=True) + rng.uniform(0.2, 1.6) * np.array([[np.cos(t0)], [np.sin(t0)]])
                o[:, list(seps)] = np.nan
                cases.append((s, o))
    run(handle, "device %s, separators" % ("interx" if mode == INTERX else "sat soup"), mode, cases)


# ---- InterX on its three soups


def isolated(n_columns, at, q, k0):
    """a far polyline of n_columns columns; `at` >= 0: columns at, at + 1 are the segment q, cut off from the rest by separators"""
    o = far_polyline(n_columns, (0, 1), k0)
    if at >= 0:
        o[:, at : at + 2] = q
        if at > 0:
            o[:, at - 1] = np.nan
        if at + 2 < n_columns:
            o[:, at + 2] = np.nan
    return o


def three_soup_cases(rng):
    """(A, B, (vehicle soup, HDV soup, boundary), want): segment counts (n0, n1, n2) with zeros in every place and totals at the ends of
    the rounds; the only crossing in each soup in turn — of A, of B only, of A only — or in none"""
    out = []
    for total in (63, 64, 65, 128, 129):
        a, b = int(rng.integers(1, total - 1)), 0
        b = int(rng.integers(1, total - a))
        for counts in ((total, 0, 0), (0, total, 0), (0, 0, total), (a, total - a, 0), (a, 0, total - a), (0, a, total - a), (a, b, total - a - b)):
            for cols in SHAPE_COLUMNS:
                while True:  # B = A grown about its middle (below 4 columns: and moved aside), until each of the two short segments crosses its own shape only
                    A = E.random_shape(rng, convex=False, cols=cols)
                    c = (A[:, :-1] if cols >= 4 else A).mean(axis=1, keepdims=True)
                    B = c + 1.75 * (A - c) + (0.0 if cols >= 4 else 0.1 * np.diff(across_first_edge(A, 1.0), axis=1))
                    only_a, only_b = across_first_edge(A, 0.02), across_first_edge(B, 0.02)
                    if [X.interx_exact(P, q) for P in (A, B) for q in (only_a, only_b)] == [(True, True), (False, True), (False, True), (True, True)]:
                        break
                for where in (-1, 0, 1, 2):
                    if where >= 0 and counts[where] == 0:
                        continue
                    for q, which in ((only_a, "A"), (only_b, "B")):
                        soups = []
                        for i, n in enumerate(counts):
                            cols_i = n + 1 if n or rng.integers(2) else 0  # no segments: one column or none
                            at = int(rng.choice([0, n - 1, rng.integers(0, n)])) if i == where else -1
                            soups.append(isolated(cols_i, at, q, 40 * i))
                        want = where >= 0 and (which == "A") == (where < 2)  # A meets the two obstacle soups, B the boundary
                        out.append((A, B, tuple(soups), want))
                        if where < 0:
                            break
    return out


def test_interx_on_three_soups(handle):
    from oracle import oracle

    cases = three_soup_cases(np.random.default_rng(70))
    codes = handle.interx_soups([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert ((codes == 0) | (codes == 1)).all(), np.flatnonzero(codes > 1)[:10]
    want = np.array([oracle.interx(A, v) or oracle.interx(A, h) or oracle.interx(B, l) for A, B, (v, h, l), _ in cases])
    assert np.array_equal(codes == 1, want), np.flatnonzero((codes == 1) != want)[:10]
    verdicts = []
    for A, B, (v, h, l), w in cases:
        parts = [X.interx_exact(A, v), X.interx_exact(A, h), X.interx_exact(B, l)]
        verdicts.append((any(x for x, _ in parts), all(d for _, d in parts)))
        assert verdicts[-1] == (w, True)
    E.compare("device interx, three soups", codes == 1, verdicts, 0.0, TALLY)
    totals = {sum(max(s.shape[1] - 1, 0) for s in c[2]) for c in cases}
    assert totals == {63, 64, 65, 128, 129}


def test_interx_on_three_random_soups(handle):
    """... and in general position: three soups of stars about the shape, B = A grown by a half"""
    from oracle import oracle

    rng = np.random.default_rng(71)
    cases = []
    for _ in range(1500):
        A = E.random_shape(rng, convex=False, cols=int(rng.integers(2, 9)))
        c = A.mean(axis=1, keepdims=True)
        B = c + 1.5 * (A - c)
        soups = tuple(soup_of_size(rng, int(rng.integers(0, 90)), False, 1.6) + np.array([[0.0], [0.0]]) for _ in range(3))
        cases.append((A, B, soups))
    codes = handle.interx_soups([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert ((codes == 0) | (codes == 1)).all(), np.flatnonzero(codes > 1)[:10]
    want = np.array([oracle.interx(A, v) or oracle.interx(A, h) or oracle.interx(B, l) for A, B, (v, h, l) in cases])
    assert np.array_equal(codes == 1, want), np.flatnonzero((codes == 1) != want)[:10]
    verdicts = []
    for A, B, (v, h, l) in cases[:600]:
        parts = [X.interx_exact(A, v), X.interx_exact(A, h), X.interx_exact(B, l)]
        verdicts.append((any(x for x, _ in parts), any(x and d for x, d in parts) or all(d for _, d in parts)))
    E.compare("device interx, three random soups", (codes == 1)[:600], verdicts, 0.01, TALLY)
    only_b = np.array([oracle.interx(B, l) and not (oracle.interx(A, v) or oracle.interx(A, h) or oracle.interx(A, l)) for A, B, (v, h, l) in cases])
    assert only_b.sum() > 30 and (codes[only_b] == 1).all()  # a boundary crossing that only shape B has


# ---- the smallest lanelet boundaries


def test_smallest_lanelet_boundaries(handle):
    """M = 0, 1 and 2 columns, a separator first, and separators only"""
    rng = np.random.default_rng(80)
    cases = []
    for cols in SHAPE_COLUMNS:
        for rep in range(40):
            s = E.random_shape(rng, convex=True, cols=cols, irregular=rep % 2 == 1)
            c = s.mean(axis=1, keepdims=True)
            seg = c + rng.uniform(-0.7, 0.7, (2, 2))
            more = c + rng.uniform(-0.7, 0.7, (2, 3))
            cases += [(s, EMPTY), (s, seg[:, :1]), (s, seg), (s, E.columns(NAN, seg)), (s, E.columns(NAN, seg, NAN, more, NAN)), (s, E.columns(seg[:, :1], NAN, seg[:, 1:])),
                      (s, E.columns(NAN, NAN)), (s, E.columns(NAN, seg[:, :1], NAN))]
    got = run(handle, "device lanelet boundary, smallest", BOUNDARY, cases, both=False).reshape(-1, 8)
    assert not got[:, [0, 1, 5, 6, 7]].any() and 0.05 < got[:, 2].mean() < 0.95 and np.array_equal(got[:, 2], got[:, 3])


# ---- pdmpc_sincos: the device compile against the host compile


def test_sincos_device_bits_equal_host_bits(handle):
    """include/pdmpc_math.h is one implementation compiled twice; on the whole set — the libm test's, every double nearest a multiple of
    pi/2 below 2^20 * pi/2 with its neighbours and their negatives (three reduction stages), arguments of exactly two stages, +-0,
    denormals, 2^-27, 2^-28, inf and NaN — the two compiles give the same bits, no tolerance"""
    from oracle import oracle

    two = S.second_stage(np.random.default_rng(5), 200000)
    assert (S.reduction_stage(two) == 2).sum() > 150000
    x = np.concatenate([S.libm_set(), S.near_multiples(), two, S.specials()])
    assert x.size > 6 * (S.N_MAX - 1)
    s_dev, c_dev = handle.debug_sincos(x)
    s_host, c_host = oracle.sincos(x)
    for name, dev, host in (("sin", s_dev, s_host), ("cos", c_dev, c_host)):
        differ = np.flatnonzero(dev.view(np.uint64) != host.view(np.uint64))
        print("%s: %d of %d arguments differ in bits" % (name, differ.size, x.size), [(float(x[i]), hex(int(dev.view(np.uint64)[i])), hex(int(host.view(np.uint64)[i]))) for i in differ[:5]])
        assert differ.size == 0, (name, differ.size, x[differ[:10]])


def test_report(handle):
    """Not a check: writes this module's section of profiles/exact_geometry_errors.txt where PDMPC_EXACT_GEOMETRY_REPORT says."""
    assert TALLY.counts, "run with the tests above"
    write_report(TALLY, "edge checks, device")
