"""Centralized control natively on the GPU: pdmpc_controller_centralized_step / _run and centralized members of a sweep (ONE
pdmpc_plan_joint per lock-step) against the Python twin, the reference joint search (tests/joint_reference.py) and each member's solo
run; and the joint kernel's one-LDS-copy-per-distinct-soup rule (joint_kernel.hip's prologue, layout_joint, pack.cpp).

Sizes as in tests/test_gpu_joint.py: two vehicles at Hp <= 5; three vehicles at Hp <= 4 and from a moving start (63 769 nodes a step)."""
import numpy as np
import pytest

from pdmpc import abi
from pdmpc.backend import BackendError, Handle
from pdmpc.centralized import CentralizedController, centralized_mpa
from pdmpc.iteration_data import info_from_record
from pdmpc.native_controller import NativeSweep
from pdmpc.optimizer import GraphSearchHip

import centralized_cases as cc
import joint_reference as jr
from test_joint_reference import assert_records_equal

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_CAPACITY = -1, -4


def handle_for(Hp, **kw):
    options = cc.circle_options(2, Hp, **kw)
    h = Handle(options)
    h.upload_mpa(cc.centralized_mpa(options))
    return h


def test_closed_loop_equals_the_twin_and_the_reference():
    """Config_systemtests_centralized.json on the circle: 2 vehicles, Hp 5, all 20 steps.  centralized_run in one call, a second
    controller stepped one step at a time, and the twin driven by run_optimizer_joint: state, records and n_expanded at every step;
    the first three steps also against the reference search."""
    options = cc.circle_options(2, 5)
    mpa = centralized_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    gpu = GraphSearchHip(options)
    seen = []

    def plan(iters):
        seen.append(iters)
        return gpu.run_optimizer_joint(iters, mpa)

    twin = CentralizedController(options, cc.rotated_circle(options), mpa, plan)
    stepped = cc.native_on_circle(2, 5, handle=h)
    for k in range(1, 21):
        infos = twin.step()
        recs = stepped.centralized_step()
        assert h.stats()["kernel"] == 4
        for v in range(2):
            want = infos[v]
            got = info_from_record(recs[v], options.Hp)
            assert np.array_equal(got.y_predicted, want.y_predicted) and np.array_equal(got.predicted_trims, want.predicted_trims), "step %d vehicle %d" % (k, v)
            assert np.array_equal(got.tree_path, want.tree_path) and got.n_expanded == want.n_expanded, "step %d vehicle %d" % (k, v)
            assert all(np.array_equal(a, b) for a, b in zip(got.shapes, want.shapes)), "step %d vehicle %d" % (k, v)
        if k <= 3:
            assert_records_equal(recs, jr.plan_joint(options, mpa, [seen[-1]]), "step %d against the reference" % k)
        cc.assert_same_state(stepped.state(), cc.state_of_twin(twin), k, "after step %d" % k)
    timing = stepped.last_timing()
    assert timing["build"] > 0 and timing["pack"] > 0 and timing["wait_and_read_back"] > 0 and timing["choose"] == 0
    ran = cc.native_on_circle(2, 5, handle=h)
    ms = ran.centralized_run(20)
    assert len(ms) == 20 and (ms > 0).all()
    cc.assert_same_native_state(ran, stepped, "centralized_run(20)")
    assert_records_equal(ran.records(), stepped.records(), "the last step's records")
    for c in (ran, stepped):
        c.close()
    gpu.handle.close()
    h.close()


def sweep_members(h, cases):
    return [cc.native_on_circle(n, 4, angle, h, obstacles, moving) for n, angle, obstacles, moving in cases]


def test_sweep_members_equal_their_solo_runs_with_one_launch_per_step():
    """1, 2, 2 and 3 vehicles on circles turned against each other, the three-vehicle member from a moving start, at Hp 4: six
    lock-steps, each ONE launch of the joint kernel (the arena is large enough that nothing is planned twice), every member byte
    for byte where its solo controller is."""
    h = handle_for(4, max_nodes=1 << 17)
    cases = [(1, 0.0, (), False), (2, 0.3, (), False), (2, 1.1, (), False), (3, 0.7, (), True)]
    members, solo = sweep_members(h, cases), sweep_members(h, cases)
    sweep = NativeSweep(members, h)
    for step in range(1, 7):
        assert sweep.centralized_step() == [0, 0, 0, 0]
        st = h.stats()
        assert st["kernel"] == 4 and st["n_launches"] == 1, st
        assert st["n_vehicles"] == 8
        for m, (a, b) in enumerate(zip(members, solo)):
            want = b.centralized_step()
            assert_records_equal(a.records(), want, "step %d member %d" % (step, m))
            cc.assert_same_native_state(a, b, "step %d member %d" % (step, m))
    assert h.arena_nodes()[0] == 1 << 17, "the arena grew: a step was planned twice"
    timing = sweep.last_timing()
    assert timing["build"] > 0 and timing["wait_and_read_back"] > 0
    # a member can be taken out and stepped alone
    sweep.close()
    assert_records_equal(members[1].centralized_step(), solo[1].centralized_step(), "after the sweep")
    for c in members + solo:
        c.close()
    h.close()


def test_a_boxed_in_member_is_retired_and_the_others_run_on():
    """Scenario obstacles around a standing vehicle (test_gpu_joint.py's boxed-in problem as a scenario): the member's search runs
    empty in step 1 with the reference's tree size, it is retired, and the other members equal their solo runs over the next steps.
    A sweep with no live member left returns PDMPC_EXHAUSTED."""
    h = handle_for(4)
    options = cc.circle_options(2, 4)
    start = cc.rotated_circle(options, 0.5).vehicles[0]
    box = [cc.rectangle(start.x_start, start.y_start, 0.3, 0.3)]
    cases = [(2, 0.0, (), False), (2, 0.5, box, False), (1, 0.9, (), False)]
    members, solo = sweep_members(h, cases), sweep_members(h, cases)
    probe = cc.native_on_circle(2, 4, 0.5, None, box)
    probe.centralized_build()
    want = jr.plan_joint(options, centralized_mpa(options), [probe.centralized_problem()], max_nodes=h.arena_nodes()[0])
    assert (want["status"] == abi.EXHAUSTED).all() and want["n_expanded"][0] > 1
    sweep = NativeSweep(members, h)
    for step in range(1, 4):
        assert sweep.centralized_step() == [0, 1, 0]
        assert h.stats()["n_vehicles"] == (5 if step == 1 else 3)
        for m in (0, 2):
            assert_records_equal(members[m].records(), solo[m].centralized_step(), "step %d member %d" % (step, m))
            cc.assert_same_native_state(members[m], solo[m], "step %d member %d" % (step, m))
        assert_records_equal(members[1].records(), want, "the retired member's records")
        retired = members[1].state()
        assert retired["k"] == 1 and (retired["speed"] == 0).all()
    with pytest.raises(BackendError) as e:
        solo[1].centralized_step()
    assert e.value.status == abi.EXHAUSTED
    assert_records_equal(solo[1].records(), want, "the solo run of the boxed-in member")
    cc.assert_same_native_state(members[1], solo[1], "the boxed-in member")
    sweep.close()
    alone = NativeSweep([members[1]], h)
    with pytest.raises(BackendError, match="every member") as e:
        alone.centralized_run(3)  # step 2 of this member: retired at once, then nobody is left
    assert e.value.status == abi.EXHAUSTED
    assert alone.centralized_status() == [2] and members[1].state()["k"] == 2
    alone.close()
    for c in members + solo + [probe]:
        c.close()
    h.close()


def test_sweep_on_a_small_arena_grows_it_and_changes_nothing():
    """max_nodes 512: the two-vehicle members' first steps have 5 672 nodes, so the call is planned again with larger arenas for all
    problems; the members equal solo runs on a handle that never grows."""
    small, big = handle_for(4, max_nodes=512), handle_for(4, max_nodes=1 << 15)
    cases = [(1, 0.0, (), False), (2, 0.3, (), False), (2, 1.1, (), False)]
    members, solo = sweep_members(small, cases), sweep_members(big, cases)
    sweep = NativeSweep(members, small)
    launches = []
    for step in range(1, 4):
        assert sweep.centralized_step() == [0, 0, 0]
        launches.append(small.stats()["n_launches"])
        for m, (a, b) in enumerate(zip(members, solo)):
            assert_records_equal(a.records(), b.centralized_step(), "step %d member %d" % (step, m))
            cc.assert_same_native_state(a, b, "step %d member %d" % (step, m))
    assert launches[0] > 1 and launches[-1] == 1, launches
    assert small.arena_nodes()[0] > 512 and big.arena_nodes()[0] == 1 << 15
    sweep.close()
    for c in members + solo:
        c.close()
    small.close()
    big.close()


def test_a_soup_shared_by_two_vehicles_is_staged_once():
    """Two vehicles at Hp 3 from a moving start and R convex rectangles far from both, R chosen from layout_joint's budget so that one
    copy of the soup (15 columns a rectangle: 5 columns at each of 3 steps) fits 160 KB beside the single-speed tables and two copies
    do not.  Handed over with copied arrays the problem does not fit (that pins the sizing); with the same arrays in both vehicles it
    is planned, and equals the reference."""
    options, mpa, iters = cc.twin_iters_from_a_moving_start(2, 3)
    cap = cc.joint_soup_capacity(mpa, 3)
    other = 2 * 2 + 2  # two boundaries of [NaN, NaN] each, and the two columns layout_joint adds
    one_copy, two_copies = (cap - other) // 15, (cap - other) // 30
    R = (one_copy + two_copies) // 2
    assert two_copies < R <= one_copy and R > 300
    rects = cc.far_rectangles(R)
    h = Handle(options)
    h.upload_mpa(mpa)
    for it in iters:
        it.obstacles = [r.copy() for r in rects]
    with pytest.raises(BackendError, match="do not fit into LDS") as e:
        h.plan_joint([iters])
    assert e.value.status == ERR_CAPACITY
    for it in iters:
        it.obstacles = list(rects)
    got = h.plan_joint([iters])
    assert h.stats()["lds_bytes"] > 64 * 1024
    assert_records_equal(got, jr.plan_joint(options, mpa, [iters], max_nodes=h.arena_nodes()[0]), "shared soup")
    # ... and through the optimizer interface, which the twin drives
    gpu = GraphSearchHip(options)
    infos = gpu.run_optimizer_joint(iters, mpa)
    assert [i.n_expanded for i in infos] == got["n_expanded"].tolist()
    gpu.handle.close()
    h.close()


def lines(y0, y1, shift):
    return (np.array([[-30.0 + shift, 60.0], [y0, y0]]), np.array([[-30.0, 60.0 + shift], [y1, y1]]))


def mixed_problem(blockers=True):
    """Three vehicles at Hp 3 from a moving start: vehicles 0 and 2 hold the same obstacle arrays, vehicle 1 its own, and each has a
    boundary of its own.  Each set holds a small rectangle in the way of ONE vehicle (set A: vehicle 0, set B: vehicle 1), so a
    vehicle that read the other set's soup would plan another path."""
    options, mpa, iters = cc.twin_iters_from_a_moving_start(3, 3, 0.2)

    def ahead(it, d):
        x, y, yaw = it.x0[:3]
        return cc.rectangle(x + d * np.cos(yaw), y + d * np.sin(yaw), 0.05, 0.05)

    a = cc.far_rectangles(7) + ([ahead(iters[0], 0.45)] if blockers else [])
    b = cc.far_rectangles(3) + ([ahead(iters[1], 0.45)] if blockers else [])
    iters[0].obstacles, iters[1].obstacles, iters[2].obstacles = list(a), list(b), list(a)
    for v, it in enumerate(iters):
        it.predicted_lanelet_boundary = lines(-20.0 - v, 40.0 + v, 0.5 * v)
    return options, mpa, iters


def test_mixed_sharing_in_one_problem():
    options, mpa, iters = mixed_problem()
    want = jr.plan_joint(options, mpa, [iters])
    assert (want["status"] == abi.OK).all()
    _, _, free = mixed_problem(blockers=False)
    unblocked = jr.plan_joint(options, mpa, [free])
    for v in (0, 1):
        assert not np.array_equal(want["y_predicted"][v], unblocked["y_predicted"][v]), "vehicle %d's blocker is not in its way" % v
    h = Handle(options)
    h.upload_mpa(mpa)
    got = h.plan_joint([iters])
    assert_records_equal(got, want, "shared arrays")
    lit = [h.packed_offsets(v)[0] for v in range(3)]
    ll = [h.packed_offsets(v)[2] for v in range(3)]
    assert lit[0] == lit[2] != lit[1] and len({l[0] for l in ll}) == 3
    for it in iters:
        it.obstacles = [o.copy() for o in it.obstacles]
    assert_records_equal(h.plan_joint([iters]), want, "copied arrays")
    lit = [h.packed_offsets(v)[0] for v in range(3)]
    assert len({tuple(l) for l in lit}) == 3
    h.close()


def test_packer_shares_obstacles_and_boundaries_apart():
    """Two vehicles with the same obstacle arrays and different boundaries: equal lit_off, different ll_off (before: separate copies of
    the obstacles, because the boundary arrays were part of the one key); the same boundary arrays under other obstacles: equal ll_off.
    The single-vehicle searches of the same vehicles read the shared pool and return what they return for copies."""
    options, mpa, iters = cc.twin_iters_from_a_moving_start(2, 3)
    rects = cc.far_rectangles(5)
    for v, it in enumerate(iters):
        it.obstacles = list(rects)
        it.predicted_lanelet_boundary = lines(-20.0 - v, 40.0 + v, 0.0)
    h = Handle(options)
    h.upload_mpa(mpa)
    shared = h.plan_batch(iters)
    (lit0, hdv0, ll0), (lit1, hdv1, ll1) = h.packed_offsets(0), h.packed_offsets(1)
    assert lit0 == lit1 and hdv0 == hdv1 and ll0[0] != ll1[0] and ll0[1] == ll1[1] == 6
    assert lit0[3] - lit0[0] == 3 * 5 * 5
    iters[1].obstacles = [r.copy() for r in rects]
    copied = h.plan_batch(iters)
    assert h.packed_offsets(0)[0] != h.packed_offsets(1)[0]
    assert_records_equal(shared, copied, "plan_batch on the shared pool")
    h.close()


def test_rejections_with_a_handle():
    """A handle whose checker is not the separating-axis one: PDMPC_ERR_INVALID; five vehicles in a controller or a member:
    PDMPC_ERR_CAPACITY; before anything advances, for a controller and a sweep."""
    h = handle_for(4)
    five, two = cc.native_on_circle(5, 4, handle=h), cc.native_on_circle(2, 4, handle=h)
    sweep = NativeSweep([two, five], h)
    for call in (five.centralized_step, lambda: five.centralized_run(2), sweep.centralized_step, lambda: sweep.centralized_run(2)):
        with pytest.raises(BackendError, match="PDMPC_JOINT_MAX") as e:
            call()
        assert e.value.status == ERR_CAPACITY
    assert five.state()["k"] == 0 and two.state()["k"] == 0
    sweep.close()
    two.centralized_step()  # (the refusals left the handle and the member as they were)
    assert two.state()["k"] == 1
    for c in (five, two):
        c.close()
    h.close()
    options = cc.circle_options(2, 4)
    hx = Handle(options, checker=abi.CHECK_INTERX)
    hx.upload_mpa(centralized_mpa(options))
    nat = cc.native_on_circle(2, 4, handle=hx)
    sweep = NativeSweep([nat], hx)
    for call in (nat.centralized_build, nat.centralized_step, lambda: nat.centralized_run(2), sweep.centralized_build, sweep.centralized_step, lambda: sweep.centralized_run(2)):
        with pytest.raises(BackendError, match="separating-axis") as e:
            call()
        assert e.value.status == ERR_INVALID
    assert nat.state()["k"] == 0
    sweep.close()
    nat.close()
    hx.close()
