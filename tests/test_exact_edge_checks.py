"""The oracle's collision primitives (oracle.interx, oracle.intersect_sat, oracle.intersect_lanelet_boundary) against exact arithmetic
(tests/exact_geometry.py: proper crossings and the exact normalised gap, written from the definitions) — the CPU twin of
tests/test_gpu_edge_check_limits.py, which holds the device to both.

The oracle restates the reference's MATLAB lines and the device restates them again; this module is the one place where either is held to
geometry that shares nothing with those lines.  A case counts where double arithmetic cannot change its answer, which the exact values
alone decide (exact_geometry.interx_exact / sat_exact: 64 eps R^2 on an orientation value, 32 eps R on a normalised gap, 0 where every
operation is exact in doubles); at most 1 % of a general-position family and 10 % of a lattice SAT family may stay undecided, and every
family must show both outcomes.  With PDMPC_EXACT_GEOMETRY_REPORT=<file> the last test writes this module's section of
profiles/exact_geometry_errors.txt."""
import numpy as np
import pytest

from oracle import oracle

import edge_check_cases as E
import exact_geometry as X
from reachable_geometry_checks import write_report

TALLY = E.Tally()
EMPTY = np.zeros((2, 0))


def test_the_reference_itself_on_known_answers():
    """the exact reference on cases whose answers are plain: crossing, touching, shared vertex, collinear overlap; gaps of boxes"""
    sq = np.array([[0, 0, 1, 1, 0], [0, 1, 1, 0, 0]], dtype=np.float64)
    assert X.interx_exact(sq, np.array([[0.5, 0.5], [-1, 0.5]]), 0) == (True, True)  # through the bottom edge
    assert X.interx_exact(sq, np.array([[0.5, 0.5], [-1, 0.0]]), 0) == (False, True)  # an end on the edge
    assert X.interx_exact(sq, np.array([[0.0, -1.0], [0.0, -1.0]]), 0) == (False, True)  # a shared vertex
    assert X.interx_exact(sq, np.array([[0.25, 0.75], [0.0, 0.0]]), 0) == (False, True)  # lying on the edge
    assert X.interx_exact(sq, np.array([[-1.0, 2.0], [0.0, 0.0]]), 0) == (False, True)  # collinear, longer than the edge
    assert X.interx_exact(sq, np.array([[0.5, np.nan, 0.5], [-1, np.nan, 0.5]]), 0) == (False, True)  # the separator ends both segments
    assert X.interx_exact(sq, np.array([[0.5, 0.5], [-1, 0.5]])) == (True, True)
    assert X.interx_exact(sq, np.array([[0.5, 0.5], [-1, 1e-17]])) == (True, False)  # crosses by less than the slack
    assert X.sat_gap_exact(sq, sq + np.array([[1.0], [0.0]])) == (0, 0)  # touching along an edge
    assert X.sat_gap_exact(sq, sq + np.array([[1.0], [1.0]])) == (0, 0)  # ... at a corner
    assert X.sat_gap_exact(sq, sq + np.array([[1.25], [0.5]])) == (1, X.Fraction(1, 16))
    assert X.sat_gap_exact(sq, sq + np.array([[0.5], [0.25]])) == (-1, X.Fraction(1, 4))
    assert X.sat_gap_exact(sq, np.array([[2.0, 1.0], [1.0, 2.0]])) == (1, X.Fraction(1, 2))  # a segment across the corner: the gap is on its own normal
    assert X.sat_exact(sq, sq + np.array([[1.0], [0.0]]), 0) == (True, True) and X.sat_exact(sq, sq + np.array([[1.0], [0.0]])) == (True, False)
    assert X.sat_gap_exact(sq[:, :1], sq[:, 2:3]) is None  # two points: no axis
    assert [p.shape[1] for p in X.split_soup(np.array([[np.nan, 1, 2, np.nan, np.nan, 3], [np.nan, 1, 2, np.nan, np.nan, 3]]))] == [2, 1]
    assert X.boundary_exact(sq, np.array([[1.0, 2.0], [0.5, 0.5]]), EMPTY, 0) == (True, True)  # a boundary vertex on the box's right line
    assert X.boundary_exact(sq, np.array([[1.25, 2.0], [0.5, 0.5]]), EMPTY, 0) == (False, True)


def test_interx_on_the_lattice_is_exact():
    """multiples of 2^-2 within +-8: every product and difference of InterX is exact in doubles, so the oracle equals the exact answer in
    every case — shared vertices, a segment lying on an edge, an end in the middle of an edge, zero-length edges"""
    cases = E.interx_lattice(np.random.default_rng(11), 3000)
    assert max(X.largest_coordinate(s, o) for s, o in cases) <= 8.0
    got = [oracle.interx(s, o) for s, o in cases]
    assert E.compare("interx lattice", got, E.judge_interx(cases, lattice=True), 0.0, TALLY) == (3000, 0)


def test_interx_in_general_position():
    cases = E.interx_general(np.random.default_rng(12), 1500)
    assert {s.shape[1] for s, _ in cases} == set(range(2, 9))
    got = [oracle.interx(s, o) for s, o in cases]
    E.compare("interx general position", got, E.judge_interx(cases), 0.01, TALLY)


def test_sat_on_axis_aligned_boxes_touching_collides():
    """dyadic boxes: axes (+-1, 0), (0, +-1) and projections are exact, so every case counts, and boxes that touch along an edge or at a corner
    collide (intersect_sat.m:33-40: an axis separates only if its gap is > 0)"""
    cases = E.sat_boxes(np.random.default_rng(13), 1200)
    got = [oracle.intersect_sat(a, b) for a, b in cases]
    verdicts = E.judge_sat(cases, exact_axes=True, tally=TALLY, family="sat boxes")
    touching = [i for i, (a, b) in enumerate(cases) if X.sat_gap_exact(a, b)[0] == 0]
    assert len(touching) >= 300 and all(got[i] for i in touching)
    assert E.compare("sat boxes", got, verdicts, 0.0, TALLY) == (1200, 0)


def test_sat_on_lattice_convex_pairs():
    """convex polygons on lattices of 4 and 8 units, one of them moved: the undecided pairs are exactly the touching ones (the smallest other
    gap on such a lattice, about unit / 12, is far above the slack).  A touching pair may come out either way in doubles, in the reference's
    MATLAB as here (a corner on a diagonal edge can have a double gap of +1.1e-16 and is then reported separate), which is why touching
    pairs count as undecided outside the families whose axes are exact."""
    cases = E.sat_lattice_pairs(np.random.default_rng(14), 1500)
    got = [oracle.intersect_sat(a, b) for a, b in cases]
    verdicts = E.judge_sat(cases, tally=TALLY, family="sat lattice pairs")
    for i, (a, b) in enumerate(cases):
        touching = X.sat_gap_exact(a, b)[0] == 0
        assert touching == (not verdicts[i][1]), i
    E.compare("sat lattice pairs", got, verdicts, 0.10, TALLY)


def test_sat_in_general_position():
    cases = E.sat_general(np.random.default_rng(15), 1500)
    assert {a.shape[1] for a, _ in cases} == set(range(2, 9))
    got = [oracle.intersect_sat(a, b) for a, b in cases]
    E.compare("sat general position", got, E.judge_sat(cases, tally=TALLY, family="sat general position"), 0.01, TALLY)


def test_every_edge_of_the_shape_decides():
    """a vertex of the other operand just outside or inside the middle of one edge: only that edge's normal separates, for every edge of
    shapes of 3 to 8 columns, open or closed"""
    cases = E.sat_vertex_at_edge(np.random.default_rng(18), 1200)
    assert {(a.shape[1], bool((a[:, 0] == a[:, -1]).all())) for a, _ in cases} >= {(3, False), (8, False), (8, True)}
    got = [oracle.intersect_sat(a, b) for a, b in cases]
    E.compare("sat vertex at an edge", got, E.judge_sat(cases, tally=TALLY, family="sat vertex at an edge"), 0.01, TALLY)
    cases = E.boundary_vertex_at_edge(np.random.default_rng(19), 1200)
    got = [oracle.intersect_lanelet_boundary(s, left, right) for s, left, right in cases]
    E.compare("lanelet boundary vertex at an edge", got, E.judge_boundary(cases), 0.01, TALLY)


def test_lanelet_boundary_in_general_position():
    cases = E.boundary_general(np.random.default_rng(16), 1000)
    got = [oracle.intersect_lanelet_boundary(s, left, right) for s, left, right in cases]
    E.compare("lanelet boundary general position", got, E.judge_boundary(cases), 0.01, TALLY)


def test_lanelet_boundary_on_the_bounding_box():
    """boxes between axis-parallel boundaries (exact axes): a boundary vertex on one of the box's bounding lines passes the filter in front
    of SAT by equality (intersect_lanelet_boundary.m:20,40 rejects with a strict `<`), and a boundary that touches the box collides"""
    cases = E.boundary_boxes(np.random.default_rng(17), 1200)
    got = [oracle.intersect_lanelet_boundary(s, left, right) for s, left, right in cases]
    assert E.compare("lanelet boundary boxes", got, E.judge_boundary(cases, exact_axes=True), 0.0, TALLY) == (1200, 0)
    on_line = [i for i, (s, left, right) in enumerate(cases) if left[1, 0] == s[1].max() or right[1, 0] == s[1].min() or np.isin(s[0].max(), left[0])]
    assert len(on_line) >= 400 and 0.05 < np.mean([got[i] for i in on_line]) < 0.95


def test_degenerate_operands_follow_the_oracle_only():
    """fewer than two distinct points: no valid axis, so there is no exact verdict to hold the oracle to; what it answers is pinned here
    (a NaN axis separates nothing, so a point collides with whatever the other operand's own axes do not separate from it)"""
    sq = np.array([[0, 0, 1, 1, 0], [0, 1, 1, 0, 0]], dtype=np.float64)
    inside, outside = np.array([[0.5], [0.5]]), np.array([[2.0], [0.5]])
    assert E.judge_sat([(sq, inside), (inside, sq), (sq, np.repeat(outside, 3, axis=1))]) == [None, None, None]
    assert oracle.intersect_sat(sq, inside) and not oracle.intersect_sat(sq, outside)
    assert oracle.intersect_sat(inside, outside)  # two points: no axis at all
    assert not oracle.interx(sq, inside) and not oracle.interx(inside, sq)


def test_sat_slack_bound_holds_and_report():
    """The term-by-term bound behind the SAT slack, about 14 eps R, against the largest |double gap - exact gap| recorded above (the
    double gap is the same operations in Python floats); then, not a check, this module's section of the report."""
    assert TALLY.rows, "run with the tests above"
    assert TALLY.worst_gap_units() <= 14.0, "the bound behind the SAT slack is wrong: %.2f eps R seen" % TALLY.worst_gap_units()
    write_report(TALLY, "edge checks, oracle")
