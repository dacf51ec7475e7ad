"""The future collision assessment on the MI355X at its kernel's limits (csrc/fca_kernel.hip): every case against
the exact counts of tests/fca_reference.py where they are decided (or the family's closed form where the exact reference would take
minutes), and against the host twin bit for bit.  The families are tests/fca_cases.py's; the CPU half is tests/test_fca_exact.py.

What the cases reach that equal boxes in random traffic do not: vertex counts from 1 to 64 and the dynamic index r Hp + k, touching
footprints, zero-length edges, the second trip through the item pass's grid-stride loop, thousands of hits on one counter, Hp 2 and
16, coordinates of 2^20 m, and the last vehicle's skipped obstacles.  With PDMPC_FCA_EXACT_REPORT=<file> the last test writes the
device's rows and the module's wall time into that file (profiles/fca_exact_margins.txt)."""
import os
import re
import time

import numpy as np
import pytest

import fca_cases as C
import fca_reference as F
from pdmpc.backend import Handle, fca_collisions_host
from pdmpc.config import Config, MpaType, ScenarioType

pytestmark = pytest.mark.gpu

MARGINS = F.Margins()
STARTED = []


def _constant(name):
    """a #define of csrc/pdmpc_device.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "p-dmpc_amd", "csrc", "pdmpc_device.h")
    return int(re.search(r"^#define %s (\d+)\b" % name, open(path).read(), re.M).group(1))


FIRST_STRIDE = _constant("PDMPC_FCA_MAX_BLOCKS") * _constant("PDMPC_FCA_BLOCK")  # items of one trip through the item pass's loop


@pytest.fixture(scope="module")
def handle():
    STARTED.append(time.perf_counter())
    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=10, mpa_type=MpaType.single_speed, max_vehicles=512))
    yield h
    h.close()


def exact(handle, case):
    return C.check(case, MARGINS, python=False, device=handle)


def closed_form(handle, case):
    """the families too large for the exact reference: device = closed form = host twin"""
    want = np.asarray(case.expected, dtype=np.int64)
    got = np.asarray(case.call(handle.fca_collisions), dtype=np.int64)
    assert np.array_equal(got, want), (case.family, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    assert np.array_equal(np.asarray(case.call(fca_collisions_host), dtype=np.int64), want), case.family
    return got


@pytest.mark.parametrize("heading", C.HEADINGS)
def test_abutting_grid_counts_every_touch(handle, heading):
    for alternate in (False, True):
        a = exact(handle, C.abutting_grid(heading, alternate=alternate))
        assert a.touches == a.hits > 0
        assert exact(handle, C.abutting_grid(heading, gap=C.STEP, alternate=alternate)).hits == 0


def test_points_segments_and_polygons_of_every_size(handle):
    case = C.polygon_zoo()
    assert sorted({o.shape[1] for o in case.obstacles}) == [1, 2, 3, 4, 5, 8, 17, 64]
    a = exact(handle, case)
    assert a.undecided == 0 and a.touches >= 10 and a.counts[2] == 0 and min(a.counts[:2]) > 0


def test_dynamic_rows_are_read_row_by_row_with_their_own_vertex_counts(handle):
    """tests/test_fca_exact.py shows of the same case that a transposed index or a fixed vertex count would change these counts"""
    a = exact(handle, C.dynamic_rows())
    assert a.undecided == 0 and a.counts == [5, 5, 5, 0]


def test_zero_length_edges_change_nothing(handle):
    base = exact(handle, C.zero_length_edges(0))
    assert base.hits > 0
    for mode in (1, 2, 3):
        assert exact(handle, C.zero_length_edges(mode)).counts == base.counts


@pytest.mark.parametrize("shift", [0.0, 1e4])
def test_general_position(handle, shift):
    case = C.general_position(64, seed=17, shift=shift)
    a = exact(handle, case)
    assert a.hits > 50 and a.undecided_share <= C.UNDECIDED_CAP and sum(a.decided) >= 58, (a.hits, a.undecided, a.tests, sum(a.decided))
    assert {o.shape[1] for o in case.obstacles + [p for row in case.dynamic for p in row]} == set(range(3, 13))


def test_stride_tail_takes_a_second_trip_through_the_item_loop(handle):
    n, Hp = 512, 10
    case = C.stride_tail(n, Hp)
    assert len(case.pairs) * Hp == 1308160 > FIRST_STRIDE
    # Pass 2 of fca_kernel.hip numbers the pair items t = p Hp + k, p the pair's place in the list (the stride-edge test below holds
    # the kernel to that at the very item where the first trip ends).  From it: which couples' items lie beyond the first stride
    first_item = np.array([C.pair_index(n, 2 * v, 2 * v + 1) * Hp for v in range(n // 2)])
    assert all(tuple(case.pairs[C.pair_index(n, 2 * v, 2 * v + 1)]) == (2 * v, 2 * v + 1) for v in (0, 100, 145, 255))
    beyond = first_item >= FIRST_STRIDE
    straddling = (first_item < FIRST_STRIDE) & (first_item + Hp > FIRST_STRIDE)
    assert beyond.sum() == 114 and not straddling.any() and beyond[145:].all()  # 2 v >= 284; the couples with 2 v >= 290 among them
    got = closed_form(handle, case)
    assert (got[np.repeat(beyond, 2)] == Hp).all() and got.tolist() == [Hp] * n


def test_stride_edge_items_fill_the_first_trip_exactly(handle):
    Hp = 16
    assert FIRST_STRIDE % Hp == 0
    case = C.stride_edge(FIRST_STRIDE // Hp, Hp)
    assert len(case.pairs) * Hp == FIRST_STRIDE and sum(case.expected) == 6 * Hp
    a, b = case.pairs[-1]
    assert case.expected[a] >= Hp and case.expected[b] >= Hp  # the last item of the trip is a hit
    closed_form(handle, case)
    case = C.stride_edge(FIRST_STRIDE // Hp, Hp, obstacle=True)  # the obstacle's items are the first of the second trip
    assert case.expected[:2] == [2 * Hp, 2 * Hp]
    closed_form(handle, case)
    closed_form(handle, C.stride_edge(FIRST_STRIDE // Hp + 1, Hp))
    closed_form(handle, C.stride_edge(FIRST_STRIDE // Hp - 1, Hp, obstacle=True))


def test_one_counter_takes_every_hit(handle):
    case = C.one_counter_boxes(2000, 2)
    assert case.expected == [4000, 0]
    exact(handle, case)
    case = C.one_counter_vehicles(128, 2)
    assert case.expected == [127 * 2] * 128
    closed_form(handle, case)


@pytest.mark.parametrize("Hp", [2, 16])
def test_horizon_limits_on_the_grid(handle, Hp):
    exact(handle, C.abutting_grid((0.0, 1.0), Hp=Hp))


def test_one_vehicle_launches_no_items_and_clears_the_counts(handle):
    before = exact(handle, C.abutting_grid((1.0, 0.0), side=2))
    assert min(before.counts) > 0  # what the handle's count buffer holds now
    one = C.abutting_grid((1.0, 0.0), side=1)
    one.obstacles, one.expected = [C.box(-0.25, -0.125, 0.5, 0.125)], [0]  # under the only vehicle, which is the last: no item at all
    exact(handle, one)
    two = C.abutting_grid((-1.0, 0.0), side=2)
    two.refs, two.pairs, two.headings = two.refs[:2], C.full(2), tuple(h[:2] for h in two.headings)
    two.expected = [two.Hp, two.Hp]
    exact(handle, two)  # (two vehicles: no static polygon, no dynamic row)
    none = C.abutting_grid((1.0, 0.0), side=1)  # one vehicle and nothing else: no pair, no obstacle item
    assert none.expected == [0] and not none.obstacles and not len(none.pairs)
    exact(handle, none)
    exact(handle, _three_with_one_polygon_and_one_row())


def _three_with_one_polygon_and_one_row():
    """three standing vehicles 4 apart at Hp 2, ONE static polygon (under vehicle 0: a hit at both steps) and ONE dynamic row (under
    vehicle 1 at step 0, far away at step 1); vehicle 2, the last, has no obstacle item: the smallest call with an entry in every list"""
    refs = [np.tile([[4.0 * v, 0.0]], (2, 1)) for v in range(3)]
    row = [C.box(3.75, -0.125, 4.25, 0.125), C.box(100.0, 100.0, 101.0, 101.0)]
    return C.Case("one polygon, one row", refs, C.full(3), C.turned(3, 2, (1.0, 0.0)), [C.box(-0.25, -0.125, 0.25, 0.125)], [row], expected=[2, 1, 0])


def _as_group(case):
    return dict(reference_points=case.refs, pairs=case.pairs, length=case.sizes[0], width=case.sizes[1], offset=case.sizes[2], obstacles=case.obstacles,
                dynamic_obstacle_area=case.dynamic, headings=case.headings)


def test_polygon_sets_that_do_not_start_at_vertex_zero(handle):
    """pdmpc_fca_collisions on polygon sets whose offset[0] is 3: the three vertices in front belong to no polygon (they lie where they
    would turn every count if the call read its polygons from vertex 0 on)"""
    import ctypes

    from pdmpc import abi
    from pdmpc.backend import fca_pack, load_library

    case = _three_with_one_polygon_and_one_row()
    args, (coll, prio), keep = fca_pack(case.refs, case.pairs, *case.sizes, case.obstacles, case.dynamic, headings=case.headings)
    arrays = []

    def behind_three_vertices(ps):
        n, tot = ps.n_polygons, ps.offset[ps.n_polygons]
        off = np.array([ps.offset[p] + 3 for p in range(n + 1)], dtype=np.int32)
        x = np.array([1e3, 1e3 + 1, 1e3] + [ps.x[i] for i in range(tot)])
        y = np.array([1e3, 1e3, 1e3 + 1] + [ps.y[i] for i in range(tot)])
        arrays.extend([off, x, y])
        return abi.PolygonSet(n_polygons=n, offset=off.ctypes.data_as(abi.c_int32_p), x=x.ctypes.data_as(abi.c_double_p), y=y.ctypes.data_as(abi.c_double_p))

    obst, dyn = behind_three_vertices(keep.refs[-2]), behind_three_vertices(keep.refs[-1])
    args[8], args[9] = ctypes.byref(obst), ctypes.byref(dyn)
    L = load_library()
    assert L.pdmpc_fca_collisions(handle.h, *args) == 0
    assert coll.tolist() == case.expected and prio.tolist() == [1, 2, 3]
    coll[:] = -1
    assert L.pdmpc_fca_collisions_host(*args) == 0
    assert coll.tolist() == case.expected


def test_small_ungrouped_call_directly_behind_a_larger_grouped_one(handle):
    """both entry points stage through one body: what the grouped call left in the staging block and in the group tables -- three
    groups, 29 vehicles, polygons and rows -- is not read by the ungrouped calls behind it"""
    big = [C.abutting_grid((1.0, 0.0), Hp=5), C.dynamic_rows(), C.abutting_grid((0.0, 1.0), Hp=5, side=3)]
    got = handle.fca_collisions_grouped([_as_group(c) for c in big])
    assert [g[0].tolist() for g in got] == [list(c.expected) for c in big]
    exact(handle, _three_with_one_polygon_and_one_row())
    got = handle.fca_collisions_grouped([_as_group(c) for c in big])
    one = C.abutting_grid((1.0, 0.0), side=1)
    exact(handle, one)
    assert [g[0].tolist() for g in got] == [list(c.expected) for c in big]


@pytest.mark.parametrize("origin", [(2.0 ** 10, 2.0 ** 10), (2.0 ** 20, -(2.0 ** 20))])
def test_grid_far_from_the_origin(handle, origin):
    near = exact(handle, C.abutting_grid((0.0, -1.0)))
    assert exact(handle, C.abutting_grid((0.0, -1.0), origin=origin)).counts == near.counts
    assert exact(handle, C.abutting_grid((1.0, 0.0), origin=origin, gap=C.STEP)).hits == 0


@pytest.mark.parametrize("reverse", [False, True])
def test_last_vehicle_skips_the_obstacles(handle, reverse):
    assert exact(handle, C.last_vehicle(reverse)).counts == [4 if reverse and v == 0 else 0 for v in range(5)]


def test_undecided_shares_and_report(handle):
    """The condition on the reference (none undecided on the lattice, at most 1 % off it) for this module's cases; writes the device's
    section of profiles/fca_exact_margins.txt, with the module's wall time, where PDMPC_FCA_EXACT_REPORT says."""
    for (family, twin), row in MARGINS.rows.items():
        assert MARGINS.share(family, twin) <= (C.UNDECIDED_CAP if family.startswith("general position") else 0.0), (family, twin, row)
    if MARGINS.rows:
        wall = "wall time of the module up to here, handle creation and exact references included: %.1f s" % (time.perf_counter() - STARTED[0])
        F.write_report(MARGINS.lines() + [wall], "device (tests/test_gpu_fca_limits.py)")
