"""Future collision assessment for several independent sets of vehicles in one call (pdmpc_fca_collisions_grouped_host) and as ONE
step-preparation call of a sweep (pdmpc_sweep_last_prep_calls) without a GPU: the grouped host twin returns
the ungrouped twin's counts and priorities group by group, refuses what it must, and a sweep with FCA members leaves every member
where its own steps leave it.  The device half is tests/test_gpu_fca_grouped.py and tests/test_gpu_sweep_fca.py."""
import ctypes as C

import numpy as np
import pytest

import fca_cases as F
from pdmpc import abi
from pdmpc.backend import BackendError, FcaGroup, fca_collisions_grouped_call, fca_collisions_host, load_library
from pdmpc.native_controller import NativeSweep

from test_choice import assert_concatenated_batch, assert_same_choice, solo_explorative_step
from test_native_controller import assert_same_problem
from test_sweep import ERR_INVALID, assert_same_state, assert_sweep_problem, circle, road


def group_of(case, **over):
    """a case of tests/fca_cases.py as one group of a grouped call"""
    g = dict(reference_points=case.refs, pairs=case.pairs, length=case.sizes[0], width=case.sizes[1], offset=case.sizes[2], obstacles=case.obstacles,
             dynamic_obstacle_area=case.dynamic, headings=case.headings)
    g.update(over)
    return g


def alone(group, call=fca_collisions_host):
    """the ungrouped call on one group -> (collisions, priorities)"""
    return call(group["reference_points"], group["pairs"], group["length"], group["width"], group["offset"], group.get("obstacles", ()),
                group.get("dynamic_obstacle_area", ()), headings=group.get("headings"))


def empty_group(Hp):
    return dict(reference_points=[], pairs=np.zeros((0, 2), np.int32), length=1.0, width=1.0, offset=0.0, headings=(np.zeros((0, Hp)), np.zeros((0, Hp))))


def assert_groups_alone(got, groups, call=fca_collisions_host, ctx=""):
    """every group's slices are what the ungrouped `call` returns for that group alone; -> the counts"""
    assert len(got) == len(groups), ctx
    total = 0
    for g, ((coll, prio), G) in enumerate(zip(got, groups)):
        n = len(G["reference_points"])
        assert coll.shape == prio.shape == (n,), (ctx, g)
        if n == 0:
            continue
        want, want_prio = alone(G, call)
        assert np.array_equal(coll, want), (ctx, "counts of group %d" % g, coll.tolist(), np.asarray(want).tolist())
        assert np.array_equal(prio, want_prio), (ctx, "priorities of group %d" % g)
        assert sorted(prio.tolist()) == list(range(1, n + 1)), (ctx, g)
        total += int(coll.sum())
    return total


def general_groups(Hp=6):
    """general-position traffic of different n, obstacle counts and row counts (0 of either among them), one group of one vehicle"""
    shapes = [(9, 6, 2), (1, 3, 1), (14, 0, 3), (5, 4, 0), (2, 0, 0), (20, 11, 1)]
    return [group_of(F.general_position(n, Hp=Hp, seed=30 + i, n_obst=S, n_rows=R)) for i, (n, S, R) in enumerate(shapes)]


def test_grouped_twin_is_the_ungrouped_twin_group_by_group():
    groups = general_groups()
    hits = assert_groups_alone(fca_collisions_grouped_call(groups), groups)
    assert hits > 50
    # ... in another order, and a group alone
    back = groups[::-1]
    assert assert_groups_alone(fca_collisions_grouped_call(back), back) == hits
    assert_groups_alone(fca_collisions_grouped_call(groups[:1]), groups[:1])


def test_a_group_without_vehicles_between_two_others_writes_nothing():
    a, b = general_groups()[0], general_groups()[3]
    groups = [a, empty_group(6), b]
    got = fca_collisions_grouped_call(groups)
    assert got[1][0].shape == (0,) and got[1][1].shape == (0,)
    assert assert_groups_alone(got, groups) > 0
    # only groups without vehicles, and no group at all
    assert [c.shape for c, _ in fca_collisions_grouped_call([empty_group(6)] * 2, Hp=6)] == [(0,), (0,)]
    assert fca_collisions_grouped_call([], Hp=6) == []


def raw_status(n_groups, groups, Hp, arrays, out):
    """pdmpc_fca_collisions_grouped_host as it is called from C: the status"""
    L = load_library()
    arr = (FcaGroup * max(len(groups), 1))(*groups)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return L.pdmpc_fca_collisions_grouped_host(n_groups, arr if groups else None, Hp, *[p(a, abi.c_double_p) for a in arrays], *[p(a, abi.c_int32_p) for a in out])


def test_every_refusal_of_the_grouped_twin():
    Hp = 4
    pairs = np.array([[0, 1], [0, 2], [1, 2]], dtype=np.int32)
    arrays = [np.zeros(5 * Hp) for _ in range(4)]
    out = [np.zeros(5, np.int32), np.zeros(5, np.int32)]

    def group(n, pr=None, **kw):
        pr = pairs if pr is None else np.ascontiguousarray(pr, dtype=np.int32)
        keep.append(pr)
        return FcaGroup(n=n, n_pairs=len(pr), pairs=pr.ctypes.data_as(abi.c_int32_p) if len(pr) else None, length=1.0, width=0.5, offset=0.0, **kw)

    keep = []
    good = [group(3), group(2, [[0, 1]])]
    assert raw_status(2, good, Hp, arrays, out) == 0
    assert raw_status(-1, good, Hp, arrays, out) == ERR_INVALID          # n_groups < 0
    assert raw_status(2, [], Hp, arrays, out) == ERR_INVALID             # groups announced, none given
    assert raw_status(2, good, 1, arrays, out) == ERR_INVALID            # Hp < 2
    for i in range(4):                                                   # a null array with N > 0
        assert raw_status(2, good, Hp, arrays[:i] + [None] + arrays[i + 1 :], out) == ERR_INVALID
    assert raw_status(2, good, Hp, arrays, [None, out[1]]) == ERR_INVALID
    assert raw_status(2, good, Hp, arrays, [out[0], None]) == ERR_INVALID
    assert raw_status(1, [group(0, [])], Hp, [None] * 4, [None] * 2) == 0  # ... is legal with N = 0
    assert raw_status(0, [], Hp, [None] * 4, [None] * 2) == 0
    # what pdmpc_fca_check_args refuses, in the second group
    assert raw_status(2, [good[0], group(-1, [])], Hp, arrays, out) == ERR_INVALID
    assert raw_status(2, [good[0], group(2, [[0, 2]])], Hp, arrays, out) == ERR_INVALID        # a pair beyond ITS group (vehicle 2 exists in the call)
    assert raw_status(2, [good[0], group(2, [[1, 0]])], Hp, arrays, out) == ERR_INVALID        # not a < b
    assert raw_status(2, [group(3, [[0, 2], [0, 1]]), good[1]], Hp, arrays, out) == ERR_INVALID  # not ascending
    assert raw_status(2, [group(3, [[0, 1], [0, 1]]), good[1]], Hp, arrays, out) == ERR_INVALID  # a repeat
    bad_pairs = FcaGroup(n=2, n_pairs=1, pairs=None, length=1.0, width=0.5, offset=0.0)
    assert raw_status(2, [good[0], bad_pairs], Hp, arrays, out) == ERR_INVALID
    off = np.array([0, 3, 3], dtype=np.int32)  # an empty polygon
    xy = np.zeros(3)
    empty_poly = abi.PolygonSet(n_polygons=2, offset=off.ctypes.data_as(abi.c_int32_p), x=xy.ctypes.data_as(abi.c_double_p), y=xy.ctypes.data_as(abi.c_double_p))
    assert raw_status(2, [good[0], group(2, [[0, 1]], obstacles=C.pointer(empty_poly))], Hp, arrays, out) == ERR_INVALID
    off3 = np.array([0, 1, 2, 3], dtype=np.int32)  # 3 dynamic polygons: no multiple of Hp 4
    rows = abi.PolygonSet(n_polygons=3, offset=off3.ctypes.data_as(abi.c_int32_p), x=xy.ctypes.data_as(abi.c_double_p), y=xy.ctypes.data_as(abi.c_double_p))
    assert raw_status(2, [good[0], group(2, [[0, 1]], dynamic_rows=C.pointer(rows))], Hp, arrays, out) == ERR_INVALID
    assert raw_status(2, [good[0], group(2, [[0, 1]], obstacles=C.pointer(rows))], Hp, arrays, out) == 0
    with pytest.raises(BackendError, match="status -1"):
        fca_collisions_grouped_call([general_groups()[0], dict(general_groups()[3], pairs=[[1, 0]])])


# ---- a sweep with FCA members, without a handle


def fca_members(**kw):
    """three members with FCA priorities (two road networks whose vehicles meet within the first steps: their priorities differ from the
    vehicle order; the circle with a static obstacle of its own, whose vehicles meet at step 8) and one with colouring"""
    c = circle("full", **kw)
    c.kw["priority_strategy"] = "fca"
    c.scenario.obstacles = [F.box(3.5, 1.8, 3.7, 1.96)]  # a scenario obstacle of this member alone, on the way of its vehicle 2
    return [
        road(8, 4, "distance", priority_strategy="fca", **kw),
        road(6, 2, "distance", priority_strategy="coloring", max_num_CLs=2, **kw),
        road(6, 5, "distance", priority_strategy="fca", **kw),
        c,
    ]


def assert_same_priorities(a, b, ctx, fca):
    pa, pb = a.priorities(), b.priorities()
    assert pa == pb, (ctx, pa, pb)
    if fca:
        assert sorted(pa[0]) == list(range(1, a.n + 1)) and len(pa[1]) == a.n, (ctx, pa)
    return sum(pa[1])


def test_sweep_assesses_all_its_fca_members_in_one_call():
    from oracle import oracle

    members = fca_members()
    is_fca = [m.kw.get("priority_strategy") == "fca" for m in members]
    assert sum(is_fca) == 3
    solo = [m.make() for m in members]
    swept = [m.make() for m in members]
    sweep = NativeSweep(swept)
    hits, reordered = 0, 0
    try:
        for k in range(1, 9):
            problems, records = [], []
            for m, c in zip(members, solo):
                c.build_step()
                p = c.problem()
                recs, _ = oracle.plan_step(m.options, m.mpa, p)
                c.apply(recs)
                problems.append(p)
                records.append(recs)
            sweep.build()
            assert sweep.prep_calls() == [0, 0, 0, 1], k
            sp = sweep.problem()
            assert_sweep_problem(sp, problems, "step %d" % k)
            for i, (a, b, p) in enumerate(zip(solo, swept, problems)):
                assert_same_problem(b.problem(), p, "step %d, member %d's own problem" % (k, i))
                hits += assert_same_priorities(a, b, "step %d member %d" % (k, i), is_fca[i])
                reordered += is_fca[i] and b.priorities()[0] != list(range(1, b.n + 1))
            sweep.apply(np.concatenate(records)[[sp["member_slot"][s] + sum(len(r) for r in records[: sp["member"][s]]) for s in range(sweep.n)]])
            for i, (a, b) in enumerate(zip(solo, swept)):
                assert_same_state(a.state(), b.state(), "step %d member %d" % (k, i))
                assert a.seeds() == b.seeds(), (k, i)
        assert hits > 0 and reordered > 0, "the assessment never counted a collision"
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()


def test_sweep_without_fca_members_makes_no_assessment_call():
    members = [road(6, 1, "distance"), road(5, 2, "distance", priority_strategy="coloring", max_num_CLs=2)]
    cs = [m.make() for m in members]
    sweep = NativeSweep(cs)
    try:
        sweep.build()
        assert sweep.prep_calls() == [0, 0, 0, 0]
        assert cs[0].priorities() == (list(range(1, 7)), []) and cs[1].priorities() == ([], [])
    finally:
        sweep.close()
        for c in cs:
            c.close()


def test_explorative_sweep_with_fca_members():
    members = fca_members()
    is_fca = [m.kw.get("priority_strategy") == "fca" for m in members]
    solo = [m.make() for m in members]
    swept = [m.make() for m in members]
    sweep = NativeSweep(swept)
    hits = 0
    try:
        for k in range(1, 5):
            steps = [solo_explorative_step(m, c, k, 3) for m, c in zip(members, solo)]
            sweep.explore_build(3)
            assert sweep.prep_calls() == [0, 0, 0, 1], k
            assert_concatenated_batch(sweep.explore_problem(), [s[0] for s in steps], "step %d" % k)
            for i, (a, b) in enumerate(zip(solo, swept)):
                hits += assert_same_priorities(a, b, "step %d member %d" % (k, i), is_fca[i])
            sweep.explore_apply(np.concatenate([s[1] for s in steps]))
            for i, (a, b, s) in enumerate(zip(solo, swept, steps)):
                ctx = "step %d member %d" % (k, i)
                assert_same_state(a.state(), b.state(), ctx)
                assert a.seeds() == b.seeds(), ctx
                assert_same_choice(b.explore_result(), s[2:], ctx)
        assert hits > 0
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
