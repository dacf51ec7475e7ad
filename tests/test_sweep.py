"""Several closed loops in lock-step (pdmpc_sweep_*, pdmpc_*_coupling_grouped_host) without a GPU: a sweep of
handle-less controllers builds the members' problems concatenated and leaves every member bit for bit where its own steps leave it
(planner = the oracle), the grouped host twins return the ungrouped twins' blocks, and pdmpc_sweep_create refuses what it must."""
import copy

import numpy as np
import pytest

from pdmpc.backend import BackendError, bound_reachable_sets_call, polygon_set_coupling_call, polygon_set_coupling_grouped_call, reachable_set_coupling_call, reachable_set_coupling_grouped_call
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController, NativeSweep

from test_native_controller import assert_same_problem

ERR_INVALID, ERR_CAPACITY = -1, -4
HP = 5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Member:
    """What one member of a sweep is made from; make() creates its controller (twice: for the solo set and for the swept one)."""

    def __init__(self, options, scenario, coupling, force_exhaustion=None, **kw):
        self.options, self.scenario, self.coupling, self.force, self.kw = options, scenario, coupling, force_exhaustion or (lambda k: None), kw
        self.mpa = get_mpa(options)

    def make(self, handle=None, mpa=None, **more):
        """(mpa: the automaton of the handle the members share, where it is not the member's own)"""
        return NativeController(self.options, self.scenario, mpa or self.mpa, handle, coupling=self.coupling, **dict(self.kw, **more))


def road(amount, seed, coupling, max_vehicles=0, max_nodes=1 << 20, **kw):
    from pdmpc.road_network import commonroad_scenario

    ctl = {k: kw.pop(k) for k in ("priority_strategy", "weight_strategy") if k in kw}
    options = Config(scenario_type=ScenarioType.commonroad, amount=amount, Hp=HP, max_nodes=max_nodes, max_vehicles=max_vehicles, **kw)
    return Member(options, commonroad_scenario(options, seed=seed), coupling, **ctl)


def circle(coupling, force_exhaustion=None, max_vehicles=0, max_nodes=1 << 20, **kw):
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=HP, max_nodes=max_nodes, max_vehicles=max_vehicles, **kw)
    return Member(options, circle_scenario(options), coupling, force_exhaustion)


def distance_members(**kw):
    """The three members the sweep is specified on: C2-like, colouring cut to two levels, the circle with forced exhaustion."""
    return [
        road(20, 1, "distance", **kw),
        road(12, 2, "distance", priority_strategy="coloring", max_num_CLs=2, **kw),
        circle("full", force_exhaustion=lambda k: {1: 2, 4: 1}.get(k), **kw),
    ]


def reachable_members(**kw):
    """Reachable-set coupling with and without lanelet bounding and with parallel predecessors as reachable sets: one member for each
    grouped call of a step (bounded step-Hp sets, bounded sets of every step, plain hulls), the circle (bounding switched on, nothing to
    bound), and a distance-coupled member whose sets are bounded for its parallel predecessors only."""
    return [
        road(20, 1, "reachable_set", bound_reachable_sets=True, **kw),
        road(12, 2, "reachable_set", priority_strategy="coloring", max_num_CLs=2, is_deal_prediction_inconsistency=True, bound_reachable_sets=True, **kw),
        road(10, 3, "reachable_set", **kw),
        circle("reachable_set", is_deal_prediction_inconsistency=True, bound_reachable_sets=True, **kw),
        road(8, 4, "distance", priority_strategy="coloring", max_num_CLs=2, is_deal_prediction_inconsistency=True, bound_reachable_sets=True, **kw),
    ]


def concatenated(problems):
    """The members' problems as the sweep lays them out: member after member, predecessor slots shifted by the member's first slot."""
    out = {"iters": [], "preds": [], "fallback": [], "member": [], "member_slot": []}
    for m, p in enumerate(problems):
        first = len(out["iters"])
        out["iters"] += p["iters"]
        out["fallback"] += p["fallback"]
        out["preds"] += [[first + q for q in pr] for pr in p["preds"]]
        out["member"] += [m] * len(p["iters"])
        out["member_slot"] += list(range(len(p["iters"])))
    return out


def assert_sweep_problem(sp, problems, ctx):
    want = concatenated(problems)
    assert sp["member"] == want["member"] and sp["member_slot"] == want["member_slot"], ctx
    same = {"order": [], "levels": [], "level_sizes": []}  # (per member only: not part of the concatenated problem)
    assert_same_problem(dict(want, **same), dict(sp, **same), ctx)


def assert_same_state(a, b, ctx):
    for key in ("x", "y", "yaw", "speed", "steering"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (ctx, key)
    assert a["needs_fallback"].tolist() == b["needs_fallback"].tolist() and a["k"] == b["k"], ctx


def sweep_against_solo(members, n_steps, prep_calls=None):
    """(prep_calls: what pdmpc_sweep_last_prep_calls reports after every build)"""
    from oracle import oracle

    solo = [m.make() for m in members]
    swept = [m.make() for m in members]
    sweep = NativeSweep(swept)
    try:
        for k in range(1, n_steps + 1):
            problems, records = [], []
            for m, c in zip(members, solo):
                c.build_step()
                p = c.problem()
                recs, _ = oracle.plan_step(m.options, m.mpa, p)
                if m.force(k) is not None:
                    recs[p["order"].index(m.force(k))]["status"] = 1  # this vehicle's search "ran empty"
                c.apply(recs)
                problems.append(p)
                records.append(recs)
            sweep.build()
            assert prep_calls is None or sweep.prep_calls() == prep_calls, (k, sweep.prep_calls())
            sp = sweep.problem()
            assert_sweep_problem(sp, problems, "step %d" % k)
            for c, p in zip(swept, problems):  # ... and every member's own problem is the one its own build leaves
                assert_same_problem(c.problem(), p, "step %d, a member's own problem" % k)
            sweep.apply(np.concatenate(records)[[sp["member_slot"][s] + sum(len(r) for r in records[: sp["member"][s]]) for s in range(sweep.n)]])
            for i, (a, b) in enumerate(zip(solo, swept)):
                assert_same_state(a.state(), b.state(), "step %d member %d" % (k, i))
                assert a.seeds() == b.seeds(), (k, i)
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
    return records


def test_sweep_builds_and_applies_what_the_members_would_alone():
    sweep_against_solo(distance_members(), 8)


def test_sweep_with_reachable_set_coupling_on_the_grouped_host_twins():
    sweep_against_solo(reachable_members(), 8)


def fca_member(**kw):
    """8 vehicles with FCA priorities (tests/test_fca_grouped.py: fca_members()[0])"""
    return road(8, 4, "distance", priority_strategy="fca", **kw)


# One member of every preparation kind, each the smallest of its kind among the members above, and the step-preparation calls a sweep of
# that member alone makes without a handle: [lanelet bounding, bounded coupling, hull coupling, collision assessment]
ONE_MEMBER_KINDS = {
    "bounded_every_step_host_coupling": (
        lambda **kw: road(8, 4, "distance", priority_strategy="coloring", max_num_CLs=2, is_deal_prediction_inconsistency=True, bound_reachable_sets=True, **kw),
        [1, 0, 0, 0],
    ),
    "plain_hulls": (lambda **kw: road(10, 3, "reachable_set", **kw), [0, 0, 1, 0]),
    "bounded_and_coupled_on_the_bounded_sets": (
        lambda **kw: road(12, 2, "reachable_set", priority_strategy="coloring", max_num_CLs=2, is_deal_prediction_inconsistency=True, bound_reachable_sets=True, **kw),
        [1, 1, 0, 0],
    ),
    "bounding_on_nothing_to_bound": (lambda **kw: circle("reachable_set", is_deal_prediction_inconsistency=True, bound_reachable_sets=True, **kw), [0, 0, 1, 0]),
    "fca": (fca_member, [0, 0, 0, 1]),
}


@pytest.mark.parametrize("kind", sorted(ONE_MEMBER_KINDS))
def test_a_sweep_of_one_member_is_the_member_alone(kind):
    """A solo step is a sweep of one member: both go through the same step preparation, the sweep in its own scratch,
    the controller in the one it owns; the problems, states and seeds are the same bits and the calls the ones of the member's kind."""
    make, calls = ONE_MEMBER_KINDS[kind]
    sweep_against_solo([make()], 3, prep_calls=calls)


def test_controllers_move_between_stepping_alone_and_a_sweep_like_never_swept_twins():
    """Alone, then in a sweep of two, then alone again, three steps each, next to twins that only ever step alone: what a controller's
    own step-preparation scratch holds does not reach the sweep's and the reverse.  The two members use all of the scratch (lanelet
    bounding, the coupler on the bounded sets, the collision assessment) and differ in size."""
    from oracle import oracle

    members = [ONE_MEMBER_KINDS["bounded_and_coupled_on_the_bounded_sets"][0](), fca_member()]
    twins = [m.make() for m in members]
    moved = [m.make() for m in members]

    def alone(m, c):
        c.build_step()
        p = c.problem()
        c.apply(oracle.plan_step(m.options, m.mpa, p)[0])
        return p

    def all_alone(phase):
        for k in range(3):
            for i, (m, a, b) in enumerate(zip(members, twins, moved)):
                ctx = "%s, step %d member %d" % (phase, k + 1, i)
                assert_same_problem(alone(m, a), alone(m, b), ctx)
                assert_same_state(a.state(), b.state(), ctx)
                assert a.priorities() == b.priorities() and a.seeds() == b.seeds(), ctx

    sweep = None
    try:
        all_alone("alone before the sweep")
        sweep = NativeSweep(moved)
        for k in range(3):
            problems = [alone(m, c) for m, c in zip(members, twins)]
            sweep.build()
            assert sweep.prep_calls() == [1, 1, 0, 1], k
            assert_sweep_problem(sweep.problem(), problems, "in the sweep, step %d" % (k + 1))
            sweep.apply(np.concatenate([oracle.plan_step(m.options, m.mpa, p)[0] for m, p in zip(members, problems)]))
            for i, (a, b) in enumerate(zip(twins, moved)):
                assert_same_state(a.state(), b.state(), "in the sweep, step %d member %d" % (k + 1, i))
                assert a.priorities() == b.priorities() and a.seeds() == b.seeds(), (k, i)
        sweep.close()
        all_alone("alone after the sweep")
    finally:
        if sweep is not None:
            sweep.close()
        for c in twins + moved:
            c.close()


def _closed_loop_poses():
    """Recorded closed-loop poses: three steps each of a C2-like and of a smaller loop."""
    from test_bounded_reachable_sets import _states
    from pdmpc.road_network import commonroad_scenario

    out = []
    for amount, seed in ((20, 1), (12, 2)):
        o = Config(scenario_type=ScenarioType.commonroad, amount=amount, Hp=HP, mpa_type=MpaType.single_speed, max_nodes=1 << 20)
        mpa, states = _states(o, commonroad_scenario(o, seed=seed), 3)
        out += states
    return mpa, out


def test_grouped_host_twins_return_the_ungrouped_blocks():
    mpa, states = _closed_loop_poses()
    L = mpa.local_reachable_sets_conv
    groups = [states[0], states[3], states[1], states[4]]
    sizes = [len(g["x"]) for g in groups]
    cat = lambda key: np.concatenate([np.asarray(g[key]) for g in groups])  # noqa: E731
    coupled = 0
    # with an empty group and a group of one vehicle in between
    sizes_x = sizes[:1] + [0] + sizes[1:] + [1]
    one = {k: np.asarray(states[2][k])[:1] for k in ("x", "y", "yaw", "trim")}
    x, y, yaw, trim = (np.concatenate([cat(k), one[k]]) for k in ("x", "y", "yaw", "trim"))
    blocks = reachable_set_coupling_grouped_call(L, sizes_x, x, y, yaw, trim)
    assert [b[0].shape[0] for b in blocks] == sizes_x
    alone = [reachable_set_coupling_call(L, g["x"], g["y"], g["yaw"], g["trim"]) for g in groups]
    alone = alone[:1] + [(np.zeros((0, 0), np.uint8), np.zeros((0, 0)))] + alone[1:] + [(np.zeros((1, 1), np.uint8), np.zeros((1, 1)))]
    for (adj, area), (adj1, area1) in zip(blocks, alone):
        assert np.array_equal(adj, adj1) and np.array_equal(_bits(area), _bits(area1))
        coupled += int(adj.sum())
    # the bounded step-Hp sets of the same states
    polys = [s[-1] for g in groups for s in g["sets"]]
    bounded = []
    for g in groups:
        sets, _ = bound_reachable_sets_call(L, g["x"], g["y"], g["yaw"], g["trim"], g["lanelets"], 0)
        bounded += [q[0] for q in sets]
    for sets in (polys, bounded):
        blocks = polygon_set_coupling_grouped_call(sets, sizes)
        at = 0
        for (adj, area), n in zip(blocks, sizes):
            adj1, area1 = polygon_set_coupling_call(sets[at : at + n])
            assert np.array_equal(adj, adj1) and np.array_equal(_bits(area), _bits(area1))
            coupled += int(adj.sum())
            at += n
    assert coupled > 0
    with pytest.raises(BackendError, match="status -1"):
        reachable_set_coupling_grouped_call(L, [sizes[0], -1, sizes[1] + 1] + sizes[2:] + [1], x, y, yaw, trim)  # offsets that decrease


def test_every_refusal_of_sweep_create():
    a, b = road(6, 1, "distance"), road(5, 2, "distance")
    other_hp = copy.copy(b)
    other_hp.options = copy.copy(b.options)
    other_hp.options.Hp = HP + 1
    other_hp.mpa = get_mpa(other_hp.options)
    ca, cb, ch, cs = a.make(), b.make(), other_hp.make(), b.make(optimizer="sampled")

    def status(members, handle=None):
        with pytest.raises(BackendError) as e:
            NativeSweep(members, handle)
        return e.value.status

    class OtherHandle:  # (any address that is not the members' handle: create compares, it does not dereference before that)
        h = 1

    try:
        assert status([ca, ch]) == ERR_INVALID      # another Hp
        assert status([ca, cs]) == ERR_INVALID      # another optimizer
        assert status([ca, cb, ca]) == ERR_INVALID  # a member twice
        assert status([ca, cb], OtherHandle()) == ERR_INVALID  # members that are not on the sweep's handle
        assert status([]) == ERR_INVALID
        for c in (ca, cb, ch, cs):
            assert c.state()["k"] == 0  # nothing advanced
    finally:
        for c in (ca, cb, ch, cs):
            c.close()


def test_a_member_steps_alone_after_a_sweep_like_its_never_swept_twin():
    from oracle import oracle

    members = [road(8, 1, "distance"), road(6, 2, "distance", priority_strategy="coloring", max_num_CLs=2)]
    solo = [m.make() for m in members]
    swept = [m.make() for m in members]

    def alone(m, c):
        c.build_step()
        p = c.problem()
        recs, _ = oracle.plan_step(m.options, m.mpa, p)
        c.apply(recs)
        return p

    try:
        sweep = NativeSweep(swept)
        for k in range(3):
            problems = [alone(m, c) for m, c in zip(members, solo)]
            sweep.build()
            sp = sweep.problem()
            assert_sweep_problem(sp, problems, "step %d" % (k + 1))
            recs = [oracle.plan_step(m.options, m.mpa, p)[0] for m, p in zip(members, problems)]
            sweep.apply(np.concatenate(recs))
        sweep.close()
        for k in range(3):
            for m, a, b in zip(members, solo, swept):
                assert_same_problem(alone(m, a), alone(m, b), "alone after the sweep, step %d" % (k + 1))
                assert_same_state(a.state(), b.state(), "alone after the sweep, step %d" % (k + 1))
    finally:
        for c in solo + swept:
            c.close()
