"""The joint search of centralized control on the GPU (pdmpc_plan_joint, joint_kernel.hip) against the CPU reference
(tests/joint_reference.py): records byte-identical.

Sizes: the Python reference expands about 30 000 joint nodes per second.  Two vehicles on the circle run at Hp 5 (at Hp 6 one step
of the closed loop reaches 134 000 nodes); three vehicles start from standstill with 12^3 children at the root and reach 1.3 million
nodes at Hp 5, so the three-vehicle problems run at Hp 4 and from a moving start.
"""

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.backend import BackendError, Handle
from pdmpc.centralized import CentralizedController, centralized_mpa, centralized_options
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.iteration_data import VehicleIter, info_from_record
from pdmpc.optimizer import GraphSearchHip
from pdmpc.scenario import circle_scenario

import joint_reference as jr
import problems
from test_joint_reference import assert_records_equal, crossing_problem

pytestmark = pytest.mark.gpu


def circle_options(N, Hp, **kw):
    return centralized_options(Config(scenario_type=ScenarioType.circle, amount=N, Hp=Hp, mpa_type=MpaType.single_speed, T_end=4, max_vehicles=16, **kw))


def circle_iters(N, Hp, steps):
    """The iteration data CentralizedController builds on the circle scenario after `steps` steps of the reference's closed loop."""
    options = circle_options(N, Hp)
    mpa = centralized_mpa(options)

    def plan(iters):
        return [info_from_record(r, Hp) for r in jr.plan_joint(options, mpa, [iters])]

    ctl = CentralizedController(options, circle_scenario(options), mpa, plan)
    for _ in range(steps):
        ctl.step()
    return options, mpa, ctl.build_iters()


def shifted(it, dx, dy):
    """A copy of a VehicleIter moved by (dx, dy): poses, references, obstacles and boundaries."""
    d = np.array([[dx], [dy]])
    left, right = it.predicted_lanelet_boundary
    return VehicleIter(
        x0=it.x0 + np.array([dx, dy, 0.0, 0.0]),
        trim_index=it.trim_index,
        reference_trajectory_points=it.reference_trajectory_points + np.array([dx, dy]),
        v_ref=it.v_ref.copy(),
        predicted_lanelet_boundary=(None if left is None else left + d, None if right is None else right + d),
        obstacles=[o + d for o in it.obstacles],
        dynamic_obstacle_area=[[o + d for o in row] for row in it.dynamic_obstacle_area],
        amount=it.amount,
    )


def test_single_vehicle_problems_equal_plan_batch_and_the_oracle():
    from oracle import oracle

    for seed, Hp in ((0, 5), (1, 6), (2, 6)):
        options, mpa, iters = problems.problem_set("sat", seed, 12, Hp=Hp, max_vehicles=16)
        h = Handle(options)
        h.upload_mpa(mpa)
        got = h.plan_joint([[it] for it in iters])
        assert h.stats()["kernel"] == 4
        batch = h.plan_batch(iters)
        _, want, _ = oracle.plan_batch(options, mpa, iters)
        ref = jr.plan_joint(options, mpa, [[it] for it in iters], max_nodes=h.arena_nodes()[0])
        assert_records_equal(got, ref, "seed %d: kernel vs reference" % seed)
        assert_records_equal(batch, want, "seed %d: plan_batch vs oracle" % seed)
        assert_records_equal(got, want, "seed %d: kernel vs oracle" % seed)
        h.close()


def test_two_to_four_vehicles_against_the_reference():
    """N = 2 at Hp 5 at several steps of the closed loop (the head-on start is mirror-symmetric about the vehicles' common axis, so
    the search meets equal keys), N = 3 at Hp 4 from a moving start, two mirror-image problems (problems.symmetric_problem) as
    one joint problem, and N = 4 at Hp 2."""
    cases = []
    for steps in (0, 8, 10):
        options, mpa, iters = circle_iters(2, 5, steps)
        cases.append((options, mpa, [iters]))
    options, mpa, iters = circle_iters(3, 4, 2)
    cases.append((options, mpa, [iters]))
    opt = circle_options(2, 5)
    mpa2 = centralized_mpa(opt)
    sym = problems.symmetric_problem(opt, mpa2)
    cases.append((opt, mpa2, [[sym, shifted(sym, 0.0, 3.0)]]))
    # four vehicles: the crossing plus two parked vehicles at Hp 2 (2 754 nodes; at Hp 3 the same problem has 1.7 million)
    opt4 = circle_options(4, 2)
    mpa4 = centralized_mpa(opt4)
    cases.append((opt4, mpa4, [crossing_problem(opt4, mpa4) + [parked(3.0 + 2.0 * v, 3.0, opt4.Hp) for v in range(2)]]))
    for options, mpa, probs in cases:
        opt = GraphSearchHip(options)
        infos = opt.run_optimizer_joint(probs[0], mpa)
        got = opt.handle.plan_joint(probs)
        want = jr.plan_joint(options, mpa, probs, max_nodes=opt.handle.arena_nodes()[0])
        assert_records_equal(got, want, "N %d Hp %d" % (len(probs[0]), options.Hp))
        assert [i.n_expanded for i in infos] == list(want["n_expanded"])
        opt.handle.close()


def test_joint_tie_order_matters_and_is_reproduced(monkeypatch):
    """The symmetric pair meets equal keys: at most of its pops the smallest key of the open list is not unique
    (problems.tied_pops), and breaking those ties by node id instead of the reference heap's layout pops the nodes in another
    order.  The kernel reproduces the reference heap's records."""
    opt = circle_options(2, 5)
    mpa = centralized_mpa(opt)
    sym = problems.symmetric_problem(opt, mpa)
    prob = [sym, shifted(sym, 0.0, 3.0)]
    _, info = jr.search(opt, jr.JointMpa(mpa), prob, 1 << 30)

    class Trace:
        pops = np.array(info["pops"])
        tree = {"g": info["tree"]["g"], "h": info["tree"]["h"], "parent": info["tree"]["parent"]}

    assert problems.tied_pops(Trace) > 100, "no equal keys at the top of the open list"
    with monkeypatch.context() as m:
        m.setattr(jr, "_comp", lambda a, b: (a[1], a[0]) > (b[1], b[0]))  # ties: the smaller id first
        _, by_id = jr.search(opt, jr.JointMpa(mpa), prob, 1 << 30)
    assert by_id["pops"] != info["pops"], "the tie order does not change the pop sequence"
    h = Handle(opt)
    h.upload_mpa(mpa)
    assert_records_equal(h.plan_joint([prob]), jr.plan_joint(opt, mpa, [prob]))
    h.close()


def test_two_vehicles_with_lanelet_boundaries():
    """A commonroad first step built by CentralizedController with the boundary provider: boundaries in every vehicle's check."""
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = centralized_options(Config(scenario_type=ScenarioType.commonroad, amount=2, Hp=5, mpa_type=MpaType.single_speed, max_vehicles=8))
    mpa = centralized_mpa(options)
    sc = commonroad_scenario(options, seed=1)
    ctl = CentralizedController(options, sc, mpa, None, boundary_provider=boundary_provider(sc))
    iters = ctl.build_iters()
    assert all(it.predicted_lanelet_boundary[0] is not None for it in iters)
    h = Handle(options)
    assert h.cfg.checker == abi.CHECK_SAT
    h.upload_mpa(mpa)
    got = h.plan_joint([iters])
    assert_records_equal(got, jr.plan_joint(options, mpa, [iters], max_nodes=h.arena_nodes()[0]))
    h.close()


def parked(x, y, Hp):
    """A vehicle at standstill whose reference stays where it is."""
    return VehicleIter(x0=np.array([x, y, 0.0, 0.0]), trim_index=1, reference_trajectory_points=np.tile([x, y], (Hp, 1)), v_ref=np.zeros(Hp))


def test_mixed_problem_sizes_in_one_launch_equal_each_problem_alone():
    """22 problems of 1 to 4 vehicles at Hp 3: one- and two-vehicle problems from problems.problem_set (the vehicles of a problem
    5 m apart), three and four vehicles as the crossing plus parked vehicles (the four-vehicle ones reach 1.7 million nodes: the arena
    grows several times within the call)."""
    options, mpa, pool = problems.problem_set("sat", 11, 60, Hp=3, max_vehicles=64)
    options = centralized_options(options)
    mpa = centralized_mpa(options)
    cross = crossing_problem(options, mpa)
    sizes = [1, 2, 3, 4, 2, 1, 3, 2, 1, 4, 2, 3, 1, 2, 2, 1, 3, 1, 2, 1, 2, 3]
    probs, at = [], 0
    for p, n in enumerate(sizes):
        if n <= 2:
            probs.append([shifted(pool[(at + v) % len(pool)], 0.0, 5.0 * v) for v in range(n)])
        else:
            probs.append([shifted(c, 0.0, 0.1 * p) for c in cross] + [parked(3.0 + 2.0 * v, 3.0 + 0.1 * p, options.Hp) for v in range(n - 2)])
        at += n
    h = Handle(options)
    h.upload_mpa(mpa)
    together = h.plan_joint(probs)
    at = 0
    for p, prob in enumerate(probs):
        alone = h.plan_joint([prob])
        assert_records_equal(together[at : at + len(prob)], alone, "problem %d (%d vehicles)" % (p, len(prob)))
        at += len(prob)
    st = h.stats()
    assert st["kernel"] == 4 and st["n_vehicles"] == len(probs[-1]) and st["n_launches"] >= 1
    # a problem's pops and nodes are counted once, not once per vehicle; the single-vehicle byte formula does not apply
    assert st["nodes_popped"] == int(alone["n_popped"][0]) and st["nodes_generated"] == int(alone["n_expanded"][0]) - 1
    assert st["algorithmic_bytes"] == 0 and st["obstacle_columns"] == 0
    # and the small ones against the reference
    at = 0
    for p, prob in enumerate(probs):
        if len(prob) <= 3:
            assert_records_equal(together[at : at + len(prob)], jr.plan_joint(options, mpa, [prob], max_nodes=h.arena_nodes()[0]), "problem %d" % p)
        at += len(prob)
    h.close()


def boxed_problem(options, mpa):
    """Vehicle 1 stands inside an obstacle: every edge out of the root collides, the open list runs empty."""
    Hp = options.Hp
    box = np.array([[-0.3, 0.3, 0.3, -0.3], [-0.2, -0.2, 0.2, 0.2]])
    stuck = VehicleIter(
        x0=np.array([0.0, 0.0, 0.0, 0.0]),
        trim_index=1,
        reference_trajectory_points=np.column_stack([0.1 * np.arange(1, Hp + 1), np.zeros(Hp)]),
        v_ref=np.full(Hp, 0.5),
        obstacles=[box],
        amount=2,
    )
    free = VehicleIter(
        x0=np.array([0.0, 5.0, 0.0, 0.0]),
        trim_index=1,
        reference_trajectory_points=stuck.reference_trajectory_points + np.array([0.0, 5.0]),
        v_ref=stuck.v_ref.copy(),
        amount=2,
    )
    return [stuck, free]


def test_boxed_in_problem_is_exhausted_with_the_reference_tree_size():
    options = circle_options(2, 5)
    mpa = centralized_mpa(options)
    prob = boxed_problem(options, mpa)
    h = Handle(options)
    h.upload_mpa(mpa)
    got = h.plan_joint([prob])
    want = jr.plan_joint(options, mpa, [prob], max_nodes=h.arena_nodes()[0])
    assert (want["status"] == abi.EXHAUSTED).all() and want["n_expanded"][0] > 1
    assert_records_equal(got, want)
    h.close()


def test_small_arena_grows_and_the_limit_gives_overflow():
    options, mpa, iters = circle_iters(2, 5, 8)
    ref = jr.plan_joint(options, mpa, [iters])
    assert ref["n_expanded"][0] > 2048
    small = dataclass_replace(options, max_nodes=512)
    h = Handle(small)
    h.upload_mpa(mpa)
    assert_records_equal(h.plan_joint([iters]), ref, "after growth")
    assert h.arena_nodes()[0] > 512
    h.close()
    h = Handle(small)
    h.upload_mpa(mpa)
    h.set_arena_limit(512)
    h.allow_overflow = True
    rec = h.plan_joint([iters])
    assert (rec["status"] == abi.ARENA_OVERFLOW).all()
    assert_records_equal(rec, jr.plan_joint(options, mpa, [iters], max_nodes=512), "overflow record")
    h.allow_overflow = False
    with pytest.raises(BackendError):
        h.plan_joint([iters])
    h.close()


def dataclass_replace(options, **kw):
    import dataclasses

    return dataclasses.replace(options, **kw)


def test_rejections():
    import ctypes as C

    options = circle_options(2, 5)
    mpa = centralized_mpa(options)
    it = crossing_problem(options, mpa)
    hx = Handle(options, checker=abi.CHECK_INTERX)
    hx.upload_mpa(mpa)
    with pytest.raises(BackendError, match="separating-axis"):
        hx.plan_joint([it])
    hx.close()
    h = Handle(options)
    h.upload_mpa(mpa)
    with pytest.raises(BackendError, match="PDMPC_JOINT_MAX"):
        h.plan_joint([it, []])
    with pytest.raises(BackendError, match="PDMPC_JOINT_MAX"):
        h.plan_joint([it * 3])  # 6 vehicles
    arr, keep = abi.pack_vehicles(it, options.Hp)
    off = np.array([0, 2], dtype=np.int32)
    rc = h.L.pdmpc_plan_joint(h.h, 1, off.ctypes.data_as(abi.c_int32_p), arr, None)
    assert rc == -1  # PDMPC_ERR_INVALID
    del keep
    # ... and a valid call still works on the same handle
    assert_records_equal(h.plan_joint([it]), jr.plan_joint(options, mpa, [it], max_nodes=h.arena_nodes()[0]))
    h.close()


def test_closed_loop_matches_the_reference():
    """Config_systemtests_centralized.json on the circle: 2 vehicles, single_speed, T_end 4 s at dt 0.2 s = all 20 steps, at Hp 5
    (about 10 s of the reference).  The GPU controller and the reference controller drive identical trajectories."""
    options = circle_options(2, 5)
    mpa = centralized_mpa(options)
    gpu = GraphSearchHip(options)

    def plan_ref(iters):
        return [info_from_record(r, options.Hp) for r in jr.plan_joint(options, mpa, [iters])]

    a = CentralizedController(options, circle_scenario(options), mpa, lambda iters: gpu.run_optimizer_joint(iters, mpa))
    b = CentralizedController(options, circle_scenario(options), mpa, plan_ref)
    steps = options.k_end
    assert steps == 20
    for k in range(steps):
        ia, ib = a.step(), b.step()
        for v in range(2):
            assert np.array_equal(ia[v].y_predicted, ib[v].y_predicted), "step %d vehicle %d" % (k + 1, v)
            assert np.array_equal(ia[v].tree_path, ib[v].tree_path)
            assert ia[v].n_expanded == ib[v].n_expanded
        assert [(m.x, m.y, m.yaw, m.speed) for m in a.meas] == [(m.x, m.y, m.yaw, m.speed) for m in b.meas]
    gpu.handle.close()
