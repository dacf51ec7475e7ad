"""The optimal-priority step of a sweep on the device (pdmpc_sweep_optimal_step): members stepped by a sweep end every
lock-step byte for byte where their own pdmpc_controller_optimal_step leaves them -- one enumeration and one launch whatever the number
of members --, the kept records are the oracle's for the concatenated batch, plain, explorative and optimal-priority steps alternate,
and a member with more prioritizations than max_instances is refused and leaves the handle working."""
import copy

import pytest

from pdmpc.backend import BackendError, Handle
from pdmpc.config import Config, ScenarioType
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController, NativeSweep

from test_choice import assert_same_choice
from test_gpu_parity import assert_records_equal
from test_native_controller import assert_same_problem
from test_optimal_grouped import plan_concatenated
from test_sweep import ERR_CAPACITY, ERR_INVALID, assert_same_state

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def circle_members(amounts, max_vehicles, max_nodes=1 << 15):
    """circle members of the given sizes at Hp 5 with full coupling (K = n!) on one handle -> (handle, mpa, options, make)"""
    from pdmpc.scenario import circle_scenario

    made = []
    for a in amounts:
        o = Config(scenario_type=ScenarioType.circle, amount=a, Hp=5, max_vehicles=max_vehicles, max_nodes=max_nodes)
        made.append((o, circle_scenario(o)))
    options = made[0][0]
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    return h, mpa, options, lambda **kw: [NativeController(o, sc, mpa, h, coupling="full", **kw) for o, sc in made]


def road_members(max_vehicles, max_nodes=1 << 14):
    """road-network members of 5 and 6 vehicles (seeds 1 and 2) at Hp 6, distance coupling: K differs per member and per step"""
    from pdmpc.road_network import commonroad_scenario

    made = []
    for amount, seed in ((5, 1), (6, 2)):
        o = Config(scenario_type=ScenarioType.commonroad, amount=amount, Hp=6, max_vehicles=max_vehicles, max_nodes=max_nodes)
        made.append((o, commonroad_scenario(o, seed=seed)))
    options = made[0][0]
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    return h, mpa, options, lambda **kw: [NativeController(o, sc, mpa, h, coupling="distance", **kw) for o, sc in made]


def assert_same_member(a, b, ctx):
    """twin a after its own optimal_step, member b after the sweep's"""
    assert a.records().tobytes() == b.records().tobytes(), ctx
    assert_same_state(a.state(), b.state(), ctx)
    assert_same_choice(a.optimal_result(), b.optimal_result(), ctx)
    assert a.seeds() == b.seeds(), ctx
    assert_same_problem(a.problem(), b.problem(), ctx)  # (instance 0 of the step, as the build leaves it)


def sweep_against_solo(h, make, optimizer, max_instances, n_steps):
    solo, swept = make(optimizer=optimizer), make(optimizer=optimizer)
    sweep = NativeSweep(swept, h)
    seen = []  # per lock-step: (K per member, vehicles that chose another instance than 0)
    try:
        for k in range(1, n_steps + 1):
            for c in solo:
                c.optimal_step(max_instances)
            together = sweep.optimal_step(max_instances)
            assert sweep.optimal_calls() == [1, 1], k
            for i, (a, b) in enumerate(zip(solo, swept)):
                assert together[i].tobytes() == b.records().tobytes(), (k, i)
                assert_same_member(a, b, "step %d member %d" % (k, i))
            seen.append(([b.optimal_result()[1].shape[1] for b in swept], sum(int((b.optimal_result()[0] != 0).sum()) for b in swept)))
        # a member taken out of the sweep goes on alone like its twin
        sweep.close()
        for i, (a, b) in enumerate(zip(solo, swept)):
            a.optimal_step(max_instances)
            b.optimal_step(max_instances)
            assert_same_member(a, b, "alone after the sweep, member %d" % i)
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
    return seen


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
def test_circle_members_end_every_lock_step_where_their_own_optimal_steps_end(optimizer):
    h, _, _, make = circle_members((2, 3, 4), 128)
    try:
        seen = sweep_against_solo(h, make, optimizer, 30, 4)
        assert [ks for ks, _ in seen] == [[2, 6, 24]] * 4
    finally:
        h.close()


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
def test_road_members_whose_batches_differ_per_member_and_per_step(optimizer):
    h, _, _, make = road_members(6 * 200)
    try:
        seen = sweep_against_solo(h, make, optimizer, 200, 3)
        assert seen[0][0] == [24, 84]
        if optimizer == "graph_search":
            assert [ks for ks, _ in seen] == [[24, 84], [24, 90], [12, 48]]
            assert seen[0][1] > 0  # (step 1: the second member chooses instance 4)
    finally:
        h.close()


def test_a_sweep_of_one_member_is_the_member_alone():
    h, _, _, make = circle_members((3,), 32)
    try:
        assert [ks for ks, _ in sweep_against_solo(h, make, "graph_search", 6, 3)] == [[6]] * 3
    finally:
        h.close()


def test_kept_records_of_a_lock_step_are_the_oracles_for_the_concatenated_batch():
    h, mpa, options, make = circle_members((2, 3, 4), 128)
    swept = make()
    sweep = NativeSweep(swept, h)
    unbounded = copy.copy(options)
    unbounded.max_nodes = 1 << 30
    try:
        for k in range(1, 3):
            kept = sweep.optimal_step(30)
            sp = sweep.optimal_problem()  # (of the step just planned)
            assert len(sp["iters"]) == 2 * 2 + 6 * 3 + 24 * 4
            ref = plan_concatenated(unbounded, mpa, sp)
            first = 0
            for i, c in enumerate(swept):
                K = c.optimal_result()[1].shape[1]
                n_slots = c.n * K
                mine = ref[first : first + n_slots]
                chosen, cost = c.optimal_result()
                assert_same_choice((chosen, cost), c.optimal_choose(mine), "step %d member %d" % (k, i))  # (the host choice on the oracle's records)
                inst, veh = sp["instance"][first : first + n_slots], sp["vehicle"][first : first + n_slots]
                assert sp["member"][first : first + n_slots] == [i] * n_slots
                slot = {(p, v): s for s, (p, v) in enumerate(zip(inst, veh))}
                assert_records_equal(kept[i], mine[[slot[(int(chosen[v]), v)] for v in c.problem()["order"]]], "step %d member %d" % (k, i))
                first += n_slots
    finally:
        sweep.close()
        for c in swept:
            c.close()
        h.close()


def test_plain_explorative_and_optimal_steps_alternate():
    h, _, _, make = circle_members((3, 4), 128)
    solo, swept = make(), make()
    sweep = NativeSweep(swept, h)
    try:
        for k, kind in enumerate(["optimal", "plain", "explore", "optimal", "explore", "plain", "optimal"]):
            if kind == "optimal":
                for c in solo:
                    c.optimal_step(24)
                together = sweep.optimal_step(24)
            elif kind == "explore":
                for c in solo:
                    c.explore_step(3)
                together = sweep.explore_step(3)
            else:
                for c in solo:
                    c.step()
                together = sweep.step()
            for i, (a, b) in enumerate(zip(solo, swept)):
                ctx = "step %d (%s) member %d" % (k + 1, kind, i)
                assert a.records().tobytes() == together[i].tobytes() == b.records().tobytes(), ctx
                assert_same_state(a.state(), b.state(), ctx)
                assert a.seeds() == b.seeds(), ctx
                if kind == "optimal":
                    assert_same_choice(a.optimal_result(), b.optimal_result(), ctx)
                if kind == "explore":
                    assert_same_choice(a.explore_result(), b.explore_result(), ctx)
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
        h.close()


def test_max_instances_below_a_members_K_is_refused_and_the_handle_goes_on():
    h, _, _, make = circle_members((2, 3), 32)
    cs = make()
    sweep = NativeSweep(cs, h)
    fresh = None
    try:
        with pytest.raises(BackendError) as e:
            sweep.optimal_step(0)
        assert e.value.status == ERR_INVALID and all(c.state()["k"] == 0 for c in cs)
        with pytest.raises(BackendError) as e:
            sweep.optimal_step(5)  # the second member has 6 unique prioritizations
        assert e.value.status == ERR_CAPACITY
        assert sweep.optimal_calls() == [1, 0]
        for call in (lambda: sweep.optimal_step(6), lambda: sweep.step(), lambda: sweep.optimal_build(6)):
            with pytest.raises(BackendError) as e:
                call()
            assert e.value.status == ERR_INVALID  # the sweep refuses every step afterwards
        sweep.close()
        others = make()
        fresh = NativeSweep(others, h)
        try:
            fresh.optimal_step(6)
            assert fresh.optimal_calls() == [1, 1] and all(c.state()["k"] == 1 for c in others)
        finally:
            fresh.close()
            for c in others:
                c.close()
    finally:
        sweep.close()
        for c in cs:
            c.close()
        h.close()


def test_more_plans_than_the_handle_holds_are_refused_by_the_build():
    h, _, _, make = circle_members((3, 4), 100)  # 6 * 3 + 24 * 4 = 114 plans
    cs = make()
    sweep = NativeSweep(cs, h)
    try:
        with pytest.raises(BackendError) as e:
            sweep.optimal_step(24)
        assert e.value.status == ERR_CAPACITY
        with pytest.raises(BackendError) as e:
            sweep.optimal_step(24)
        assert e.value.status == ERR_INVALID
        solo = make()
        try:
            solo[1].optimal_step(24)  # 96 plans fit: the handle goes on
            assert solo[1].state()["k"] == 1
        finally:
            for c in solo:
                c.close()
    finally:
        sweep.close()
        for c in cs:
            c.close()
        h.close()
