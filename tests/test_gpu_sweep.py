"""Several closed loops in lock-step on the MI355X (pdmpc_sweep_step, csrc/reachable_kernel.hip and csrc/bounded_kernel.hip: the grouped
couplers): members stepped by a sweep end every step byte for byte where members stepped alone end it, a sweep's
records are the oracle's for its concatenated problem, every block of a grouped coupler call is the ungrouped call on that group
alone — also where the groups lie on top of each other —, and what does not fit is refused and leaves the handle working."""
import copy
import math
import os

import numpy as np
import pytest

from pdmpc.backend import BackendError, Handle
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeSweep

from test_gpu_parity import assert_records_equal
from test_sweep import ERR_CAPACITY, ERR_INVALID, HP, ONE_MEMBER_KINDS, _bits, _closed_loop_poses, assert_same_state, assert_sweep_problem, distance_members, reachable_members, road

pytestmark = pytest.mark.gpu


def shared_handle(max_vehicles, max_nodes=1 << 17):
    """One handle for all members: its automaton is the road network's (a circle member next to road members drives with it too)."""
    options = Config(scenario_type=ScenarioType.commonroad, Hp=HP, max_vehicles=max_vehicles, max_nodes=max_nodes)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    return h, mpa, options


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
@pytest.mark.parametrize("members", [distance_members, reachable_members], ids=["distance", "reachable_sets"])
def test_members_of_a_sweep_end_every_step_where_they_end_it_alone(members, optimizer):
    members = members(max_vehicles=64, max_nodes=1 << 17)
    h, mpa, _ = shared_handle(64)
    solo = [m.make(h, mpa, optimizer=optimizer) for m in members]
    swept = [m.make(h, mpa, optimizer=optimizer) for m in members]
    sweep = NativeSweep(swept, h)
    coupled = 0
    try:
        for k in range(1, 9):
            alone = [c.step() for c in solo]
            together = sweep.step()
            for i, (a, b) in enumerate(zip(alone, together)):
                ctx = "step %d member %d" % (k, i)
                assert_records_equal(b, a, ctx)
                assert a.tobytes() == b.tobytes(), ctx
                assert_same_state(solo[i].state(), swept[i].state(), ctx)
                assert solo[i].seeds() == swept[i].seeds(), ctx
            problems = [c.problem() for c in solo]
            assert_sweep_problem(sweep.problem(), problems, "step %d" % k)
            coupled += sum(len(q) for p in problems for q in p["preds"])
        assert coupled > 0
        t = sweep.last_timing()
        assert t["build"] > 0 and t["wait_and_read_back"] > 0
        # a member taken out of the sweep goes on alone like its twin
        sweep.close()
        for i, (a, b) in enumerate(zip(solo, swept)):
            ra, rb = a.step(), b.step()
            assert ra.tobytes() == rb.tobytes(), i
            assert_same_state(a.state(), b.state(), "alone after the sweep, member %d" % i)
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
        h.close()


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
@pytest.mark.parametrize("kind", ["bounded_every_step_host_coupling", "fca"])
def test_a_sweep_of_one_member_ends_every_step_where_the_member_ends_it_alone(kind, optimizer):
    """A solo step is a sweep of one member: the same grouped device calls with one group, the controller in the scratch it owns and the
    sweep in its own.  8 vehicles whose sets are bounded every step, and 8 with FCA priorities; the records carry the pops that weigh
    the next step's searches."""
    make, calls = ONE_MEMBER_KINDS[kind]
    member = make(max_vehicles=8, max_nodes=1 << 17)
    h, mpa, _ = shared_handle(8)
    solo, swept = member.make(h, mpa, optimizer=optimizer), member.make(h, mpa, optimizer=optimizer)
    sweep = NativeSweep([swept], h)
    try:
        for k in range(1, 4):
            a = solo.step()
            (b,) = sweep.step()
            assert sweep.prep_calls() == calls, k
            assert_records_equal(b, a, "step %d" % k)
            assert a.tobytes() == b.tobytes() and a["n_popped"].tolist() == b["n_popped"].tolist(), k
            assert_same_state(solo.state(), swept.state(), "step %d" % k)
            assert solo.seeds() == swept.seeds() and solo.priorities() == swept.priorities(), k
            assert_sweep_problem(sweep.problem(), [solo.problem()], "step %d" % k)
    finally:
        sweep.close()
        solo.close()
        swept.close()
        h.close()


def test_records_of_a_sweep_step_are_the_oracles_for_the_concatenated_problem():
    from oracle import oracle

    members = [road(20, 1, "distance", max_vehicles=32, max_nodes=1 << 17), road(12, 2, "distance", priority_strategy="coloring", max_num_CLs=2, max_vehicles=32, max_nodes=1 << 17)]
    h, mpa, options = shared_handle(32)
    swept = [m.make(h, mpa) for m in members]
    sweep = NativeSweep(swept, h)
    unbounded = copy.copy(options)
    unbounded.max_nodes = 1 << 30
    try:
        for k in range(1, 5):
            gpu = np.concatenate(sweep.step())
            sp = sweep.problem()
            # the oracle plans level by level: the sweep's slots sorted by their member's computation level
            level = [lv for c in swept for lv in c.problem()["levels"]]
            order = sorted(range(sweep.n), key=lambda s: level[s])
            place = {s: q for q, s in enumerate(order)}
            prob = {
                "iters": [sp["iters"][s] for s in order],
                "fallback": [sp["fallback"][s] for s in order],
                "preds": [[place[p] for p in sp["preds"][s]] for s in order],
                "level_sizes": [sum(1 for lv in level if lv == l) for l in range(1, max(level) + 1)],
            }
            ref, _ = oracle.plan_step(unbounded, mpa, prob, n_threads=min(os.cpu_count() or 1, 16))
            assert_records_equal(gpu[order], ref, "sweep step %d" % k)
    finally:
        sweep.close()
        for c in swept:
            c.close()
        h.close()


def test_sweep_create_refuses_members_that_outgrow_the_handle():
    members = [road(20, 1, "distance", max_vehicles=24), road(12, 2, "distance", max_vehicles=24)]
    h, mpa, _ = shared_handle(24, max_nodes=1 << 12)
    other, _, _ = shared_handle(24, max_nodes=1 << 12)
    cs = [m.make(h, mpa) for m in members]
    try:
        with pytest.raises(BackendError) as e:
            NativeSweep(cs, h)
        assert e.value.status == ERR_CAPACITY
        with pytest.raises(BackendError) as e:
            NativeSweep(cs[:1], other)
        assert e.value.status == ERR_INVALID
        assert all(c.state()["k"] == 0 for c in cs)
        NativeSweep(cs[:1], h).close()
    finally:
        for c in cs:
            c.close()
        h.close()
        other.close()


# ---- the grouped couplers against the ungrouped calls


def _same_blocks(blocks, alone, ctx):
    assert len(blocks) == len(alone), ctx
    for g, ((adj, area), (adj1, area1)) in enumerate(zip(blocks, alone)):
        assert adj.shape == adj1.shape and np.array_equal(adj, adj1), (ctx, g)
        assert np.array_equal(_bits(area), _bits(area1)), (ctx, g)
    return sum(int(b[0].sum()) for b in blocks)


def _hulls_alone(h, sizes, x, y, yaw, trim):
    out, at = [], 0
    for n in sizes:
        out.append(h.reachable_set_coupling(x[at : at + n], y[at : at + n], yaw[at : at + n], trim[at : at + n]))
        at += n
    return out


def _dense(rng, n, n_trims):
    side = max(1.0, math.sqrt(n) * 0.6)  # about as dense as a tile of the road network
    return rng.uniform(0, side, n), rng.uniform(0, side, n), rng.uniform(-math.pi, math.pi, n), rng.integers(1, n_trims + 1, n)


@pytest.fixture(scope="module")
def big():
    options = Config(scenario_type=ScenarioType.commonroad, Hp=HP, mpa_type=MpaType.single_speed, max_vehicles=512, max_nodes=1 << 12)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_reachable_sets(mpa.local_reachable_sets_conv)
    yield h, mpa
    h.close()


def test_grouped_hulls_on_recorded_closed_loop_poses(big):
    h, _ = big
    from test_bounded_reachable_sets import _states
    from pdmpc.road_network import commonroad_scenario

    _, c2 = _closed_loop_poses()  # C2-like: 20 vehicles (and a loop of 12)
    o = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=HP, max_num_CLs=2, mpa_type=MpaType.single_speed, max_nodes=1 << 20)
    _, c3 = _states(o, commonroad_scenario(o, seed=2, tiles=2), 2, priority_strategy="coloring")  # C3-like: 40 vehicles on two tiles
    groups = c2 + c3
    sizes = [len(g["x"]) for g in groups]
    x, y, yaw, trim = (np.concatenate([np.asarray(g[k]) for g in groups]) for k in ("x", "y", "yaw", "trim"))
    blocks = h.reachable_set_coupling_grouped(sizes, x, y, yaw, trim)
    assert h.reachable_set_coupling_kernel_ms() > 0.0
    assert _same_blocks(blocks, _hulls_alone(h, sizes, x, y, yaw, trim), "closed-loop poses") > 0


def test_grouped_hulls_at_every_group_size(big):
    h, mpa = big
    rng = np.random.default_rng(23)
    # 1, 2, 63, 64, 65 vehicles, an empty group, and 100 vehicles from vehicle 195 on: the columns of a row pass a 64-column boundary
    # both counted from the group's first vehicle and counted from vehicle 0
    sizes = [1, 2, 63, 64, 0, 65, 100]
    x, y, yaw, trim = _dense(rng, sum(sizes), mpa.n_trims)
    blocks = h.reachable_set_coupling_grouped(sizes, x, y, yaw, trim)
    assert blocks[4][0].shape == (0, 0) and blocks[0][0].shape == (1, 1) and not blocks[0][0].any() and not blocks[0][1].any()
    assert _same_blocks(blocks, _hulls_alone(h, sizes, x, y, yaw, trim), "every size") > 0
    # every vehicle alone: every block is one zero
    n = 70
    blocks = h.reachable_set_coupling_grouped([1] * n, x[:n], y[:n], yaw[:n], trim[:n])
    assert len(blocks) == n and all(b[0].shape == (1, 1) and not b[0].any() and not b[1].any() for b in blocks)
    assert h.reachable_set_coupling_grouped([], x[:0], y[:0], yaw[:0], trim[:0]) == []


def test_grouped_hulls_with_a_group_of_448_on_one_spot_at_max_vehicles(big):
    h, mpa = big
    rng = np.random.default_rng(29)
    sizes = [4] * 8 + [448] + [4] * 8
    assert sum(sizes) == 512
    x, y, yaw, trim = _dense(rng, 512, mpa.n_trims)
    x[32:480], y[32:480] = 3.0, 4.0  # every box of the big group overlaps every other: every lane of a ballot is a candidate
    blocks = h.reachable_set_coupling_grouped(sizes, x, y, yaw, trim)
    alone = _hulls_alone(h, sizes, x, y, yaw, trim)
    assert _same_blocks(blocks, alone, "448 on one spot") > 0
    big_area = blocks[8][1]
    assert (big_area[np.triu_indices(448, 1)] > 0).all(), "a pair of the big group did not reach the overlap computation"


def test_groups_at_the_same_coordinates_do_not_see_each_other(big):
    """Two groups with the same vehicles at the same coordinates: every pair of two groups would overlap if it were tested.  The blocks
    are the solo results -- this fails if the restriction to the group is dropped anywhere."""
    h, mpa = big
    rng = np.random.default_rng(31)
    for n in (5, 70):
        x, y, yaw, trim = _dense(rng, n, mpa.n_trims)
        two = [np.concatenate([a, a]) for a in (x, y, yaw, trim)]
        solo = h.reachable_set_coupling(x, y, yaw, trim)
        blocks = h.reachable_set_coupling_grouped([n, n], *two)
        assert _same_blocks(blocks, [solo, solo], "hulls, %d" % n) > 0
        together = h.reachable_set_coupling(*two)  # (what dropping the restriction would compute: the copies are coupled)
        assert together[0][:n, n:].diagonal().all()


def _bounded_alone(h, sizes, x, y, yaw, trim, lan, all_steps):
    out, at = [], 0
    for n in sizes:
        if n == 0:
            out.append((np.zeros((0, 0), np.uint8), np.zeros((0, 0))))
            continue
        h.bound_reachable_sets(x[at : at + n], y[at : at + n], yaw[at : at + n], trim[at : at + n], lan[at : at + n], all_steps)
        out.append(h.bounded_set_coupling())
        at += n
    return out


def test_grouped_bounded_sets_on_closed_loop_poses_and_on_top_of_each_other(big):
    h, _ = big
    _, states = _closed_loop_poses()
    groups = [states[0], states[3], states[0], states[1]]  # (the third group lies on the first)
    sizes = [len(g["x"]) for g in groups]
    x, y, yaw, trim = (np.concatenate([np.asarray(g[k]) for g in groups]) for k in ("x", "y", "yaw", "trim"))
    lan = [p for g in groups for p in g["lanelets"]]
    coupled = 0
    for all_steps in (0, 1):
        h.bound_reachable_sets(x, y, yaw, trim, lan, all_steps)
        blocks = h.bounded_set_coupling_grouped(sizes)
        t_bound, t_couple = h.bounded_reachable_kernel_ms()
        assert t_couple > 0.0
        coupled += _same_blocks(blocks, _bounded_alone(h, sizes, x, y, yaw, trim, lan, all_steps), "bounded, all_steps %d" % all_steps)
        assert np.array_equal(blocks[0][0], blocks[2][0]) and np.array_equal(_bits(blocks[0][1]), _bits(blocks[2][1]))
    assert coupled > 0


def test_grouped_bounded_sets_at_the_sizes_of_the_limit_tests():
    import exact_geometry as X
    from test_gpu_reachable_limits import _arrays, _bounding_batch, _one_spot_batch, _table

    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=2, max_vehicles=512, max_nodes=1 << 12))
    try:
        h.upload_reachable_sets(_arrays(_table()))
        # the batch of the declared sizes (sets of up to 1024 vertices) as two groups, and with every vehicle alone
        cases = _bounding_batch()
        n = len(cases)
        trim = np.array([c[0] for c in cases])
        lan = [None if c[1] is None else X.arr(c[1]) for c in cases]
        z = np.zeros(n)
        for sizes in ([5, n - 5], [1] * n):
            h.bound_reachable_sets(z, z, z, trim, lan, 0)
            blocks = h.bounded_set_coupling_grouped(sizes)
            _same_blocks(blocks, _bounded_alone(h, sizes, z, z, z, trim, lan, 0), "declared sizes %s" % sizes[:2])
        # 128 vehicles on one spot: every pair inside a group passes the box test (more pairs than the pair pass has workgroups)
        x, y, trim, raws = _one_spot_batch()
        n = len(x)
        lan = [None if q is None else X.arr(q) for q in raws]
        z = np.zeros(n)
        sizes = [1, 2, 0, 60, 65]
        h.bound_reachable_sets(x, y, z, trim, lan, 0)
        blocks = h.bounded_set_coupling_grouped(sizes)
        assert _same_blocks(blocks, _bounded_alone(h, sizes, x, y, z, trim, lan, 0), "one spot") > 0
        assert (blocks[4][1][np.triu_indices(65, 1)] > 0).all()
        # groups that do not cover the bounded vehicles are refused, and the handle goes on
        h.bound_reachable_sets(x, y, z, trim, lan, 0)
        with pytest.raises(BackendError, match="status -1"):
            h.bounded_set_coupling_grouped([n - 1])
        whole = h.bounded_set_coupling_grouped([n])
        _same_blocks(whole, [h.bounded_set_coupling()], "one group")
    finally:
        h.close()


def test_one_vehicle_too_many_is_refused_and_the_handle_goes_on():
    options = Config(scenario_type=ScenarioType.commonroad, Hp=HP, mpa_type=MpaType.single_speed, max_vehicles=8, max_nodes=1 << 12)
    mpa = get_mpa(options)
    h = Handle(options)
    try:
        rng = np.random.default_rng(37)
        x, y, yaw, trim = _dense(rng, 9, mpa.n_trims)
        with pytest.raises(BackendError, match="status -1"):
            h.reachable_set_coupling_grouped([4, 4], x[:8], y[:8], yaw[:8], trim[:8])  # before the upload
        with pytest.raises(BackendError, match="status -1"):
            h.bounded_set_coupling_grouped([4, 4])  # before a bounding call
        h.upload_reachable_sets(mpa.local_reachable_sets_conv)
        with pytest.raises(BackendError, match="status %d" % ERR_CAPACITY):
            h.reachable_set_coupling_grouped([4, 5], x, y, yaw, trim)
        h.bound_reachable_sets(x[:8], y[:8], yaw[:8], trim[:8], [None] * 8, 0)
        with pytest.raises(BackendError, match="status %d" % ERR_CAPACITY):
            h.bounded_set_coupling_grouped([4, 5])
        sizes = [4, 4]
        blocks = h.reachable_set_coupling_grouped(sizes, x[:8], y[:8], yaw[:8], trim[:8])
        _same_blocks(blocks, _hulls_alone(h, sizes, x[:8], y[:8], yaw[:8], trim[:8]), "after the refusals")
        h.bound_reachable_sets(x[:8], y[:8], yaw[:8], trim[:8], [None] * 8, 0)
        blocks = h.bounded_set_coupling_grouped(sizes)
        _same_blocks(blocks, _bounded_alone(h, sizes, x[:8], y[:8], yaw[:8], trim[:8], [None] * 8, 0), "bounded, after the refusals")
    finally:
        h.close()
