"""The future collision assessment against exact arithmetic, without a GPU: the host twin
(pdmpc_fca_collisions_host) and the Python twin (pdmpc.prioritizer.fca_priorities) against tests/fca_reference.py on the families of
tests/fca_cases.py, and the reference against itself and against the definition.  The device's half is
tests/test_gpu_fca_limits.py.

A count is compared where every test behind it is decided (tests/fca_reference.py says when).  Asserted, not measured: at most 1 % of
the tests of a general-position family are undecided, and none of a lattice family.  With PDMPC_FCA_EXACT_REPORT=<file> the last
test writes what the module saw into that file's section (profiles/fca_exact_margins.txt)."""
from fractions import Fraction

import numpy as np
import pytest

import exact_geometry as X
import fca_cases as C
import fca_reference as F

MARGINS = F.Margins()
UNDECIDED_CAP = C.UNDECIDED_CAP


def check(case):
    return C.check(case, MARGINS)


# ---- the reference against itself


def _variants(rng, P):
    """the same closed convex set: a cyclic shift, the reversed order, a vertex repeated, closed by its first vertex"""
    k = int(rng.integers(len(P)))
    i = int(rng.integers(len(P)))
    return [P[k:] + P[:k], P[::-1], P[: i + 1] + P[i:], P + P[:1]]


def test_closed_convex_meet_is_symmetric_and_blind_to_order_and_repeats():
    rng = np.random.default_rng(21)
    seen = {"apart": 0, "touch": 0, "overlap": 0}
    for _ in range(300):
        A = X.convex_lattice(rng, 4, 0.25)
        dx, dy = (Fraction(int(d), 4) for d in rng.integers(-4, 5, 2))
        B = [(p[0] + dx, p[1] + dy) for p in X.convex_lattice(rng, 4, 0.25)]
        if rng.integers(4) == 0:
            B = B[: int(rng.integers(1, 3))]  # a point or a segment
        meets, margin = F.closed_convex_meet(A, B)
        assert meets == (margin.sign <= 0)
        seen["apart" if margin.sign > 0 else "touch" if margin.sign == 0 else "overlap"] += 1
        assert F.closed_convex_meet(B, A) == (meets, margin)
        for A2 in _variants(rng, A):
            for B2 in _variants(rng, B):
                assert F.closed_convex_meet(A2, B2) == (meets, margin), (A, B, A2, B2)
    assert min(seen.values()) >= 20, seen


def test_closed_convex_meet_equals_the_definition():
    """on a coarse lattice, where touching is common: a vertex of one in the other, or two edges with a common point"""
    rng = np.random.default_rng(22)
    touches = 0
    for _ in range(400):
        A = X.convex_lattice(rng, 5)
        dx, dy = (int(d) for d in rng.integers(-5, 6, 2))
        B = [(p[0] + dx, p[1] + dy) for p in X.convex_lattice(rng, 5)]
        meets, margin = F.closed_convex_meet(A, B)
        assert meets == F.convex_meet_by_definition(A, B), (A, B)
        touches += margin.sign == 0
    assert touches >= 20


def test_margin_is_the_distance_in_known_cases():
    sq = [(Fraction(0), Fraction(0)), (Fraction(0), Fraction(1)), (Fraction(1), Fraction(1)), (Fraction(1), Fraction(0))]
    shifted = lambda dx, dy: [(p[0] + Fraction(dx), p[1] + Fraction(dy)) for p in sq]
    assert F.closed_convex_meet(sq, shifted(1.5, 0)) == (False, F.Margin(1, Fraction(1, 4)))
    assert F.closed_convex_meet(sq, shifted(1, 1)) == (True, F.Margin(0, Fraction(0)))  # a common corner
    assert F.closed_convex_meet(sq, shifted(0.75, 0.5)) == (True, F.Margin(-1, Fraction(1, 16)))
    assert float(F.closed_convex_meet(sq, shifted(0.75, 0.5))[1]) == -0.25
    pt = lambda x, y: [(Fraction(x), Fraction(y))]
    assert F.closed_convex_meet(sq, pt(0.5, 1))[1].sign == 0 and F.closed_convex_meet(sq, pt(0.5, 0.5))[0]
    assert F.closed_convex_meet(pt(0.5, 1.25), sq) == (False, F.Margin(1, Fraction(1, 16)))
    # flat against flat: collinear segments apart and abutting, a point on and off a segment, two points
    seg = lambda x0, x1: [(Fraction(x0), Fraction(0)), (Fraction(x1), Fraction(0))]
    assert F.closed_convex_meet(seg(0, 1), seg(2, 3)) == (False, F.Margin(1, Fraction(1)))
    assert F.closed_convex_meet(seg(0, 1), seg(1, 3))[1].sign == 0
    assert F.closed_convex_meet(seg(0, 1), pt(0.5, 0))[0] and not F.closed_convex_meet(seg(0, 1), pt(1.5, 0))[0]
    assert F.closed_convex_meet(pt(1, 2), pt(1, 2))[0] and F.closed_convex_meet(pt(1, 2), pt(4, 6)) == (False, F.Margin(1, Fraction(25)))
    # an X of two segments
    assert F.closed_convex_meet([(Fraction(-1), Fraction(-1)), (Fraction(1), Fraction(1))], [(Fraction(-1), Fraction(1)), (Fraction(1), Fraction(-1))])[0]


def test_footprint_is_the_reference_box():
    P = F.footprint(0.0, 1.0, 2.0, 3.0, C.LENGTH, C.WIDTH, C.OFFSET)  # a quarter turn: the half sizes change places
    assert P == [(Fraction(2.25), Fraction(2.625)), (Fraction(1.75), Fraction(2.625)), (Fraction(1.75), Fraction(3.375)), (Fraction(2.25), Fraction(3.375))]
    assert F.footprint_is_lattice_exact(0.0, 1.0, 2.0, 3.0, C.LENGTH, C.WIDTH, C.OFFSET) and F.polygon_is_lattice_exact(P)
    assert not F.footprint_is_lattice_exact(0.6, 0.8, 2.0, 3.0, C.LENGTH, C.WIDTH, C.OFFSET)
    assert not F.footprint_is_lattice_exact(1.0, 0.0, 2.0 + 2.0 ** -11, 3.0, C.LENGTH, C.WIDTH, C.OFFSET)
    assert not F.footprint_is_lattice_exact(1.0, 0.0, 2.0, 3.0, 0.22, 0.1, 0.01)
    c, s = 0.6, 0.8  # doubles: c² + s² is not exactly 1, and the corners are those of the doubles
    Q = F.footprint(c, s, 0.1, 0.2, 0.22, 0.1, 0.01)
    hl, hw = Fraction(0.22) / 2 + Fraction(0.01), Fraction(0.1) / 2 + Fraction(0.01)
    assert Q[2] == (Fraction(c) * hl - Fraction(s) * hw + Fraction(0.1), Fraction(s) * hl + Fraction(c) * hw + Fraction(0.2))
    assert Q[0][0] + Q[2][0] == 2 * Fraction(0.1) and Q[1][1] + Q[3][1] == 2 * Fraction(0.2)


# ---- the twins against the reference


@pytest.mark.parametrize("heading", C.HEADINGS)
def test_abutting_grid_counts_every_touch(heading):
    for alternate in (False, True):
        a = check(C.abutting_grid(heading, alternate=alternate))
        assert a.touches == a.hits > 0
        a = check(C.abutting_grid(heading, gap=C.STEP, alternate=alternate))
        assert a.hits == 0


@pytest.mark.parametrize("Hp", [2, 16])
def test_horizon_limits_on_the_grid(Hp):
    check(C.abutting_grid((0.0, 1.0), Hp=Hp, side=3))


def test_one_and_two_vehicles():
    one = C.abutting_grid((1.0, 0.0), side=1)
    one.obstacles = [C.box(-0.25, -0.125, 0.5, 0.125)]  # under the only vehicle, which is the last one
    one.expected = [0]
    check(one)
    two = C.abutting_grid((-1.0, 0.0), side=2)
    two.refs, two.pairs, two.headings = two.refs[:2], C.full(2), tuple(h[:2] for h in two.headings)
    two.expected = [two.Hp, two.Hp]
    check(two)


@pytest.mark.parametrize("origin", [(2.0 ** 10, 2.0 ** 10), (2.0 ** 20, -(2.0 ** 20))])
def test_grid_far_from_the_origin(origin):
    check(C.abutting_grid((0.0, -1.0), origin=origin))
    check(C.abutting_grid((1.0, 0.0), origin=origin, gap=C.STEP))


def test_points_segments_and_polygons_of_every_size():
    case = C.polygon_zoo()
    assert sorted({o.shape[1] for o in case.obstacles}) == [1, 2, 3, 4, 5, 8, 17, 64]
    a = check(case)
    assert a.undecided == 0 and a.touches >= 2 * 5  # the points and segments on the boundary, at both steps
    assert a.counts[2] == 0 and min(a.counts[:2]) > 0


def test_dynamic_rows_are_read_row_by_row_with_their_own_vertex_counts():
    case = C.dynamic_rows()
    a = check(case)
    assert a.undecided == 0
    # what makes a fixed vertex count show: the first four vertices of a polygon of five or more miss the footprint
    feet = [[F.footprint(1.0, 0.0, *case.refs[v][k], *case.sizes) for k in range(case.Hp)] for v in range(3)]
    sizes = set()
    for r, row in enumerate(case.dynamic):
        for k, P in enumerate(row):
            assert P.shape[1] == 3 + ((2 * r + 3 * k) % 7)
            sizes.add(P.shape[1])
            assert F.closed_convex_meet(feet[r][k], F.points(P))[0]
            if P.shape[1] >= 5:
                assert not F.closed_convex_meet(feet[r][k], F.points(P)[:4])[0]
    assert sizes == set(range(3, 10))
    # ... and a transposed index: read as polygon k n_rows + r, (r, k) hits at three of fifteen (row, step) only
    flat = [P for row in case.dynamic for P in row]
    transposed = sum(F.closed_convex_meet(feet[r][k], F.points(flat[k * 3 + r]))[0] for r in range(3) for k in range(case.Hp))
    assert transposed == 3


def test_zero_length_edges_change_nothing():
    base = check(C.zero_length_edges(0))
    assert base.hits > 0 and base.undecided == 0
    for mode in (1, 2, 3):
        case = C.zero_length_edges(mode)
        assert all(o.shape[1] > b.shape[1] for o, b in zip(case.obstacles, C.zero_length_edges(0).obstacles))
        a = check(case)
        assert a.counts == base.counts and a.tests == base.tests


@pytest.mark.parametrize("reverse", [False, True])
def test_last_vehicle_skips_the_obstacles(reverse):
    check(C.last_vehicle(reverse))


def test_one_counter_takes_every_hit():
    check(C.one_counter_boxes(200))


@pytest.mark.parametrize("n, seed, shift", [(32, 11, 0.0), (24, 12, 0.0), (24, 13, 1e4)])
def test_general_position(n, seed, shift):
    case = C.general_position(n, seed=seed, shift=shift)
    a = check(case)
    assert np.array_equal(case.python_twin(with_headings=False), case.python_twin())  # calculate_yaw and libm give the headings passed
    assert a.hits > 20 and a.undecided_share <= UNDECIDED_CAP, (a.hits, a.undecided, a.tests)
    assert sum(a.decided) >= 0.9 * n


def test_undecided_shares_and_report():
    """The condition on the reference: no undecided test in a lattice family, at most 1 % in the others.  Not a check of the twins;
    writes this module's section of profiles/fca_exact_margins.txt where PDMPC_FCA_EXACT_REPORT says."""
    for (family, twin), row in MARGINS.rows.items():
        cap = UNDECIDED_CAP if family.startswith("general position") else 0.0
        assert MARGINS.share(family, twin) <= cap, (family, twin, row)
    if MARGINS.rows:  # empty when this test runs alone
        F.write_report(MARGINS.lines(), "python and host (tests/test_fca_exact.py)")
