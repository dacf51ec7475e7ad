"""The grouped future collision assessment on the MI355X (pdmpc_fca_collisions_grouped, csrc/fca_kernel.hip):
in every case the grouped call against the ungrouped DEVICE call on every group alone, against the host twin, and against the case's
closed form.  The shapes are the smallest at which the grouped kernels can go wrong: groups of 0 to 3 vehicles, groups on top of
each other, sizes / obstacles / rows that differ per group, and group boundaries next to the boundaries of the flat item index.

Where a group boundary can lie: every range of items of a group -- n_pairs Hp, (n - 1) Hp S, (n - 1) Hp R -- is a multiple of Hp, so
a boundary between two groups lies at a multiple of Hp of the flat index.  "One item before and after" a boundary b of the index is
therefore b - Hp and b + Hp: the last lanes before (the first after) b belong to the other group than in the case with the boundary at b."""
import numpy as np
import pytest

import fca_cases as C
from pdmpc.backend import BackendError, Handle, fca_collisions_grouped_call, fca_collisions_host
from pdmpc.config import Config, MpaType, ScenarioType

from test_fca_grouped import alone, assert_groups_alone, empty_group, general_groups, group_of
from test_gpu_fca_limits import FIRST_STRIDE, _constant
from test_sweep import ERR_CAPACITY

pytestmark = pytest.mark.gpu

BLOCK = _constant("PDMPC_FCA_BLOCK")
SIZES = (C.LENGTH, C.WIDTH, C.OFFSET)


@pytest.fixture(scope="module")
def handle():
    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=10, mpa_type=MpaType.single_speed, max_vehicles=1024, max_nodes=1 << 12))
    yield h
    h.close()


def pile(n, Hp, S=0, R=0, pairs=None, at=(0.0, 0.0), sizes=SIZES):
    """n vehicles on one spot `at` that move 4 m east per step together (footprints of two steps never meet), heading east; S static
    boxes over the whole way; R dynamic rows whose polygon of step k lies on the step-k point only, with 4 to 6 vertices (repeated
    ones).  pairs: the coupled pairs, all by default.  Closed form: every listed pair meets at every step; every vehicle but the last
    meets every static box and every row at every step.  -> (group, expected counts)"""
    pairs = C.full(n) if pairs is None else np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    refs = [np.stack([at[0] + 4.0 * np.arange(Hp), np.full(Hp, at[1])], axis=1) for _ in range(n)]
    obst = [C.box(at[0] - 0.25 - i * C.STEP, at[1] - 0.125, at[0] + 4.0 * Hp, at[1] + 0.125 + i * C.STEP) for i in range(S)]
    dyn = [[C.with_repeats(C.box(at[0] + 4.0 * k - 0.125, at[1] - 0.0625 * (r + 1), at[0] + 4.0 * k + 0.125, at[1] + 0.0625), (r + k) % 4) for k in range(Hp)]
           for r in range(R)]
    expected = np.zeros(n, dtype=np.int64)
    np.add.at(expected, pairs[:, 0], Hp)
    np.add.at(expected, pairs[:, 1], Hp)
    expected[: n - 1] += Hp * (S + R)
    g = dict(reference_points=refs, pairs=pairs, length=sizes[0], width=sizes[1], offset=sizes[2], obstacles=obst, dynamic_obstacle_area=dyn,
             headings=C.turned(n, Hp, (1.0, 0.0)))
    return g, expected.tolist()


def check(handle, groups, expected=None, ctx="", heavy=False):
    """grouped device call = ungrouped device call per group = host twins (= the closed forms); -> the grouped counts per group
    (heavy: the ungrouped comparison of a large group runs once, on the device; the grouped host twin covers the host)"""
    got = handle.fca_collisions_grouped(groups)
    assert handle.fca_kernel_ms() > 0.0 or not any(len(g["reference_points"]) for g in groups), ctx
    assert_groups_alone(got, groups, handle.fca_collisions, ctx + " (ungrouped device call)")
    if not heavy:
        assert_groups_alone(got, groups, fca_collisions_host, ctx + " (host twin)")
    twin = fca_collisions_grouped_call(groups)
    for g, ((c, p), (c1, p1)) in enumerate(zip(got, twin)):
        assert np.array_equal(c, c1) and np.array_equal(p, p1), (ctx, "grouped host twin, group %d" % g)
    if expected is not None:
        assert [c.tolist() for c, _ in got] == [list(e) for e in expected], (ctx, "closed form")
    return [c.tolist() for c, _ in got]


def test_groups_of_no_one_two_and_three_vehicles(handle):
    """every vehicle sits on a static obstacle of its group, no pairs: the last vehicle of each group counts 0, the first vehicle of the
    next group does not, a group of one vehicle counts 0"""
    Hp = 3
    made = [pile(n, Hp, S=1, pairs=[], at=(0.0, 8.0 * i)) for i, n in enumerate((2, 1, 3, 1, 2, 3))]
    groups = [g for g, _ in made]
    groups.insert(2, empty_group(Hp))
    expected = [e for _, e in made]
    expected.insert(2, [])
    assert expected == [[Hp, 0], [0], [], [Hp, Hp, 0], [0], [Hp, 0], [Hp, Hp, 0]]
    check(handle, groups, expected)
    # ... with the pairs: the groups of two and three count them too
    made = [pile(n, Hp, S=1, at=(0.0, 8.0 * i)) for i, n in enumerate((0, 3, 1, 2))]
    assert [e for _, e in made] == [[], [3 * Hp, 3 * Hp, 2 * Hp], [0], [2 * Hp, Hp]]
    check(handle, [g for g, _ in made], [e for _, e in made])
    # only empty groups, and none
    assert [c.tolist() for c, _ in handle.fca_collisions_grouped([empty_group(Hp)] * 3, Hp=Hp)] == [[], [], []]
    assert handle.fca_collisions_grouped([], Hp=Hp) == []


def test_groups_at_the_same_coordinates_do_not_see_each_other(handle):
    """A and B on one spot with full pair lists; A's three obstacles lie on B's vehicles too; B has none (NULL) and counts only its pairs"""
    Hp = 4
    (a, ea), (b, eb) = pile(4, Hp, S=3, R=2), pile(5, Hp)
    assert ea == [6 * Hp + 2 * Hp] * 3 + [3 * Hp] and eb == [4 * Hp] * 5
    for groups, expected in (([a, b], [ea, eb]), ([b, a], [eb, ea]), ([b, a, b], [eb, ea, eb])):
        check(handle, groups, expected)
    # (what dropping the restriction to the group would count: the nine vehicles as one group)
    both = dict(a, reference_points=a["reference_points"] + b["reference_points"], pairs=C.full(9), headings=C.turned(9, Hp, (1.0, 0.0)))
    assert alone(both, handle.fca_collisions)[0].tolist() == [8 * Hp + 5 * Hp] * 8 + [8 * Hp]


def test_every_group_has_its_own_vehicle_sizes(handle):
    """two vehicles side by side, 0.5 apart, and two behind each other, 1.0 apart: they touch (a hit) with half sizes (0.5, 0.25) and
    miss with anything smaller"""
    Hp = 2
    refs = [np.tile([[0.0, 0.0]], (Hp, 1)), np.tile([[0.0, 0.5]], (Hp, 1)), np.tile([[16.0, 0.0]], (Hp, 1)), np.tile([[17.0, 0.0]], (Hp, 1))]
    pairs = [[0, 1], [2, 3]]
    g = lambda length, width, offset: dict(reference_points=refs, pairs=pairs, length=length, width=width, offset=offset, headings=C.turned(4, Hp, (1.0, 0.0)))  # noqa: E731
    groups = [g(0.75, 0.25, 0.125), g(0.75, 0.25, 0.125 - C.STEP), g(0.5, 0.375, 0.0625), g(1.0, 0.5, 0.0), g(1.0 - 2 * C.STEP, 0.5 - 2 * C.STEP, 0.0)]
    expected = [[Hp] * 4, [0] * 4, [Hp, Hp, 0, 0], [Hp] * 4, [0] * 4]
    check(handle, groups, expected)
    check(handle, groups[::-1], expected[::-1])


def test_dynamic_rows_of_no_one_and_three_rows_are_the_groups_own(handle):
    """step k reads polygon r Hp + k of ITS group's rows: the groups stand 64 m apart and the steps 4 m, so that a polygon of another
    group, row or step misses; the rows' polygons have 4, 5 and 6 vertices"""
    Hp = 5
    made = [pile(3, Hp, R=R, S=S, at=(0.0, 64.0 * i)) for i, (R, S) in enumerate(((0, 2), (1, 0), (3, 1), (0, 0), (3, 0)))]
    assert sorted({p.shape[1] for g, _ in made for row in g["dynamic_obstacle_area"] for p in row}) == [4, 5, 6]
    check(handle, [g for g, _ in made], [e for _, e in made])
    assert [e for _, e in made][2] == [Hp * 4 + 2 * Hp] * 2 + [2 * Hp]
    # and in general position, as the CPU test has them (rows of 3 to 12 vertices, obstacle and row counts of 0 among them)
    groups = general_groups()
    assert sum(sum(c) for c in check(handle, groups)) > 50


def first_pairs(n, count):
    pairs = C.full(n)[:count]
    assert len(pairs) == count
    return pairs


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_group_boundary_at_a_workgroup_boundary(handle, d):
    """Hp 2: the first group's items end at BLOCK + 2 d -- in the pair range, in the static range and in the dynamic range"""
    Hp = 2
    units = BLOCK // Hp + d
    tail = lambda i: pile(3, Hp, S=2, R=1, at=(0.0, 64.0 * (i + 1)))  # noqa: E731
    # pair range: `units` pairs of 17 vehicles, then a group whose pair items begin at BLOCK + 2 d
    made = [pile(17, Hp, pairs=first_pairs(17, units)), tail(0)]
    check(handle, [g for g, _ in made], [e for _, e in made], "pair range")
    # static range (no pairs anywhere: the static range starts at item 0): (n - 1) S = units
    n, S = {-1: (128, 1), 0: (65, 2), 1: (44, 3)}[d]
    assert (n - 1) * S == units
    made = [pile(n, Hp, S=S, pairs=[]), pile(3, Hp, S=2, pairs=[], at=(0.0, 64.0)), pile(2, Hp, S=1, pairs=[], at=(0.0, 128.0))]
    check(handle, [g for g, _ in made], [e for _, e in made], "static range")
    # dynamic range (no pairs, no static obstacles): (n - 1) R = units
    made = [pile(n, Hp, R=S, pairs=[]), pile(3, Hp, R=2, pairs=[], at=(0.0, 64.0)), pile(2, Hp, R=1, pairs=[], at=(0.0, 128.0))]
    check(handle, [g for g, _ in made], [e for _, e in made], "dynamic range")


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_group_boundary_at_the_end_of_the_first_trip_of_the_item_loop(handle, d):
    """Hp 16: the first group's pair items end at PDMPC_FCA_MAX_BLOCKS PDMPC_FCA_BLOCK + 16 d (tests/fca_cases.py: stride_edge, 512 vehicles
    with the first pairs of their full coupling); the second group's pair items and both groups' obstacle items take the second trip"""
    Hp = 16
    assert FIRST_STRIDE % Hp == 0
    case = C.stride_edge(FIRST_STRIDE // Hp + d, Hp, obstacle=True)
    assert len(case.pairs) * Hp == FIRST_STRIDE + Hp * d
    (b, eb), (c, ec) = pile(5, Hp, S=2, R=1, at=(0.0, -64.0)), pile(2, Hp, S=1, at=(0.0, -128.0))
    check(handle, [group_of(case), b, c], [case.expected, eb, ec], heavy=True)


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_group_boundary_in_the_static_range_at_the_end_of_the_first_trip(handle, d):
    """no pairs; the first group's (n - 1) Hp S static items end at the first trip's end + 16 d"""
    Hp = 16
    n, S = {-1: (256, 257), 0: (257, 256), 1: (2, 65537)}[d]
    assert (n - 1) * S * Hp == FIRST_STRIDE + Hp * d
    made = [pile(n, Hp, S=S, pairs=[]), pile(3, Hp, S=2, pairs=[], at=(0.0, 64.0)), pile(2, Hp, R=2, pairs=[], at=(0.0, 128.0))]
    check(handle, [g for g, _ in made], [e for _, e in made], heavy=True)


def test_one_counter_takes_every_hit_of_its_group(handle):
    """2000 boxes x 2 steps on vehicle 0 of the middle group (tests/fca_cases.py: one_counter_boxes); its neighbours, on the same spot
    without obstacles and pairs, stay 0"""
    case = C.one_counter_boxes(2000, 2)
    quiet = lambda: pile(2, 2, pairs=[])[0]  # noqa: E731
    check(handle, [quiet(), group_of(case), quiet()], [[0, 0], [4000, 0], [0, 0]])
    crowd = C.one_counter_vehicles(128, 2)
    check(handle, [quiet(), group_of(crowd), quiet()], [[0, 0], [127 * 2] * 128, [0, 0]])


def test_a_smaller_call_after_a_large_one_sees_nothing_stale(handle):
    Hp = 4
    large = [pile(60, Hp, S=3, R=2, at=(0.0, 64.0 * i)) for i in range(4)]
    check(handle, [g for g, _ in large], [e for _, e in large])
    # the same buffers again: fewer vehicles at other places, a group without pairs where the counts were largest
    small = [pile(3, Hp, pairs=[], at=(4.0, 64.0)), pile(2, Hp, S=1, at=(0.0, 0.0))]
    assert [e for _, e in small] == [[0, 0, 0], [2 * Hp, Hp]]
    check(handle, [g for g, _ in small], [e for _, e in small])
    # ... and the ungrouped call after the grouped one, and back
    g, e = pile(4, Hp, S=1)
    assert alone(g, handle.fca_collisions)[0].tolist() == e
    check(handle, [g for g, _ in small], [e for _, e in small])


@pytest.mark.parametrize("Hp", [2, 16])
def test_horizon_limits(handle, Hp):
    grid = C.abutting_grid((0.0, 1.0), Hp=Hp)
    made = [pile(3, Hp, S=1, R=2, at=(0.0, 64.0)), pile(2, Hp, at=(0.0, 128.0))]
    check(handle, [made[0][0], group_of(grid), made[1][0]], [made[0][1], grid.expected, made[1][1]])


def test_max_vehicles_is_accepted_and_one_more_refused():
    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=10, mpa_type=MpaType.single_speed, max_vehicles=8, max_nodes=1 << 12))
    try:
        Hp = 3
        made = [pile(3, Hp, S=1), pile(5, Hp, R=1, at=(0.0, 64.0))]
        check(h, [g for g, _ in made], [e for _, e in made])
        more = [pile(3, Hp, S=1), pile(6, Hp, R=1, at=(0.0, 64.0))]
        with pytest.raises(BackendError, match="status %d" % ERR_CAPACITY):
            h.fca_collisions_grouped([g for g, _ in more])
        with pytest.raises(BackendError, match="status -1.*group 1"):
            h.fca_collisions_grouped([made[0][0], dict(made[1][0], pairs=[[1, 0]])])
        with pytest.raises(BackendError, match="status -1"):
            h.fca_collisions_grouped([pile(2, 1)[0]])  # Hp < 2
        check(h, [g for g, _ in made], [e for _, e in made], "after the refusals")
    finally:
        h.close()
