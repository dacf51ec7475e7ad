"""Reachable sets and the reachable-set coupler without a GPU.

The local table of the automaton (pdmpc.reachability, Python) and its C++ twin (pdmpc_local_reachable_sets) are bit-identical,
convex, in polyshape's vertex order, and equal to the hulls of the enumerated vertices; the overlap areas of the host twin agree with
scipy's half-space intersection and are bit-identical to Python's; the native controller (no handle, oracle as planner) builds the
same step problems as the Python controller with reachable-set coupling and with parallel predecessors as reachable sets."""
import itertools
import math

import numpy as np
import pytest

from pdmpc import reachability as R
from pdmpc.backend import local_reachable_sets_native, reachable_set_coupling_call
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.mpa import MotionPrimitiveAutomaton, get_mpa
from pdmpc.native_controller import NativeController

scipy_spatial = pytest.importorskip("scipy.spatial")
HULL_CASES = [(MpaType.single_speed, Hp) for Hp in (1, 5, 6, 8, 10)] + [(MpaType.triple_speed, 8)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def tables():
    out = {}
    for mt, Hp in HULL_CASES:
        for scenario in (ScenarioType.circle, ScenarioType.commonroad):  # convex / non-convex maneuver areas
            mpa = MotionPrimitiveAutomaton(Config(mpa_type=mt, Hp=Hp, scenario_type=scenario))
            out[(mt, Hp, scenario)] = (mpa, mpa.local_reachable_sets_conv, local_reachable_sets_native(mpa))
    return out


def test_python_and_native_tables_are_bit_identical(tables):
    for key, (mpa, py, nat) in tables.items():
        assert len(py) == len(nat) == mpa.n_trims
        for i in range(mpa.n_trims):
            assert len(py[i]) == len(nat[i]) == mpa.Hp
            for k in range(mpa.Hp):
                assert py[i][k].shape == nat[i][k].shape and np.array_equal(bits(py[i][k]), bits(nat[i][k])), (key, i, k)


def test_hulls_are_strictly_convex_clockwise_and_start_at_the_smallest_x(tables):
    for key, (mpa, py, _) in tables.items():
        for i, k in itertools.product(range(mpa.n_trims), range(mpa.Hp)):
            h = py[i][k]
            m = h.shape[1]
            assert m >= 3
            assert not (h[0, 0] == h[0, -1] and h[1, 0] == h[1, -1]), "first vertex repeated"
            start = min(range(m), key=lambda q: (h[0, q], h[1, q]))
            assert start == 0, (key, i, k)
            for q in range(m):
                a, b, c = h[:, q], h[:, (q + 1) % m], h[:, (q + 2) % m]
                # read backwards (counter-clockwise, as the monotone chain built it) every vertex is a strict left turn: clockwise,
                # no collinear vertex
                assert R._cross(c[0], c[1], b[0], b[1], a[0], a[1]) > 0, (key, i, k, q)


def _enumerated_points(mpa, i, t):
    """Every vertex the reference unions for trim i (0-based) at step t (1-based): the DP of MotionPrimitiveAutomaton.m:394-647
    without hulls in between (the second half places the unions' vertices, which have the same hull as the enumerated points)."""
    T = mpa.transition_matrix_single
    Hp = mpa.Hp
    h = (Hp + 1) // 2

    def areas(parents, k):
        pts, kids = [], []
        for trim, (x0, y0, yaw0) in parents:
            for j in np.nonzero(T[trim, :, k])[0]:
                m = mpa.maneuvers[trim][int(j)]
                ax, ay = R.translate_global(yaw0, x0, y0, m.area[0], m.area[1])
                pts.append(np.array([ax, ay]))
                c, s = math.cos(yaw0), math.sin(yaw0)
                kids.append((int(j), (c * m.dx - s * m.dy + x0, s * m.dx + c * m.dy + y0, yaw0 + m.dyaw)))
        return np.hstack(pts), kids

    def first(trim, upto, last_slice=None):
        parents = [(trim, (0.0, 0.0, 0.0))]
        for k in range(upto):
            sl = last_slice if (last_slice is not None and k == upto - 1) else k
            pts, kids = areas(parents, sl)
            parents = kids
        return pts, parents

    if t <= h:
        return first(i, t)[0]
    _, steps = first(i, t - h)
    out = []
    for j, (x0, y0, yaw0) in steps:
        pts = first(j, h, Hp - 1 if t == Hp else None)[0]
        out.append(np.array(R.translate_global(yaw0, x0, y0, pts[0], pts[1])))
    return np.hstack(out)


def _same_vertex_set(h, pts, tol=1e-12):
    hull = scipy_spatial.ConvexHull(pts.T)
    ref = pts[:, hull.vertices]
    if ref.shape[1] != h.shape[1]:
        return False
    return all(np.min(np.hypot(ref[0] - h[0, q], ref[1] - h[1, q])) < tol for q in range(h.shape[1]))


@pytest.mark.parametrize("mt,Hp", [(MpaType.single_speed, 1), (MpaType.single_speed, 5), (MpaType.single_speed, 6), (MpaType.triple_speed, 8)])
def test_hulls_equal_scipy_hulls_of_the_enumerated_vertices(tables, mt, Hp):
    mpa, py, _ = tables[(mt, Hp, ScenarioType.commonroad)]
    rng = np.random.default_rng(Hp)
    for i in rng.choice(mpa.n_trims, size=min(4, mpa.n_trims), replace=False):
        for k in range(Hp):
            assert _same_vertex_set(py[i][k], _enumerated_points(mpa, int(i), k + 1)), (mt, Hp, i, k)


@pytest.mark.parametrize("Hp", [3, 4])
def test_time_invariant_dp_equals_brute_force_over_all_sequences(Hp):
    """recursive_feasibility = False: every transition slice is the same, so the DP hull at step t is the hull of the areas of every
    t-step maneuver sequence."""
    mpa = MotionPrimitiveAutomaton(Config(mpa_type=MpaType.single_speed, Hp=Hp, recursive_feasibility=False, scenario_type=ScenarioType.circle))
    A = mpa.adjacency
    table = mpa.local_reachable_sets_conv
    for i in range(mpa.n_trims):
        poses = [(i, 0.0, 0.0, 0.0)]
        for t in range(1, Hp + 1):
            pts, nxt = [], []
            for trim, x0, y0, yaw0 in poses:
                for j in np.nonzero(A[trim])[0]:
                    m = mpa.maneuvers[trim][int(j)]
                    pts.append(np.array(R.translate_global(yaw0, x0, y0, m.area[0], m.area[1])))
                    c, s = math.cos(yaw0), math.sin(yaw0)
                    nxt.append((int(j), c * m.dx - s * m.dy + x0, s * m.dx + c * m.dy + y0, yaw0 + m.dyaw))
            poses = nxt
            assert _same_vertex_set(table[i][t - 1], np.hstack(pts), tol=1e-9), (i, t)


def _scipy_overlap(a, b):
    """Area of the intersection of two clockwise convex polygons (open) by scipy's half-space intersection."""
    from scipy.optimize import linprog

    def halfspaces(p):
        x, y = p
        rows = []
        for e in range(x.size):
            e1 = (e + 1) % x.size
            ux, uy = x[e1] - x[e], y[e1] - y[e]
            rows.append([-uy, ux, uy * x[e] - ux * y[e]])  # inside: cross(u, p - q) <= 0
        return np.array(rows)

    H = np.vstack([halfspaces(a), halfspaces(b)])
    norm = np.linalg.norm(H[:, :2], axis=1)
    res = linprog([0, 0, -1], A_ub=np.hstack([H[:, :2], norm[:, None]]), b_ub=-H[:, 2], bounds=[(None, None), (None, None), (0, None)])
    if res.status != 0 or res.x[2] < 1e-9:
        return 0.0
    pts = scipy_spatial.HalfspaceIntersection(H, res.x[:2]).intersections
    return scipy_spatial.ConvexHull(pts).volume


def _random_poses(rng, n, n_trims, spread):
    return rng.uniform(0, spread, n), rng.uniform(0, spread, n), rng.uniform(-math.pi, math.pi, n), rng.integers(1, n_trims + 1, n)


def test_overlap_areas_match_scipy(tables):
    mpa, L, _ = tables[(MpaType.single_speed, 8, ScenarioType.commonroad)]
    rng = np.random.default_rng(7)
    x, y, yaw, trim = _random_poses(rng, 120, mpa.n_trims, 3.0)
    for q in range(0, 120, 2):
        a = R.reachable_sets_at_pose(L, x[q], y[q], yaw[q], trim[q])[-1][:, :-1]
        b = R.reachable_sets_at_pose(L, x[q + 1], y[q + 1], yaw[q + 1], trim[q + 1])[-1][:, :-1]
        assert abs(R.overlap_area(a, b) - _scipy_overlap(a, b)) < 1e-9, q
    # identical poses: the hull's own area
    a = R.reachable_sets_at_pose(L, 0.4, -0.2, 0.7, 5)[-1]
    assert abs(R.overlap_area(a, a) - scipy_spatial.ConvexHull(a[:, :-1].T).volume) < 1e-9
    # far apart: not even the boxes overlap
    adj, area = R.reachable_set_coupling([a, a + np.array([[50.0], [0.0]])])
    assert adj.sum() == 0 and area.sum() == 0


def test_boxes_that_only_touch_are_not_coupled(tables):
    mpa, L, _ = tables[(MpaType.single_speed, 5, ScenarioType.circle)]
    a = R.reachable_sets_at_pose(L, 0.0, 0.0, 0.0, 3)[-1]
    width = float(a[0].max() - a[0].min())
    for dx in (width, 0.0):  # touching boxes: skipped by the box test; the same place: coupled
        b = R.reachable_sets_at_pose(L, dx, 0.0, 0.0, 3)[-1]
        if dx:
            assert b[0].min() == a[0].max()
        adj, area = R.reachable_set_coupling([a, b])
        nat_adj, nat_area = reachable_set_coupling_call(L, [0.0, dx], [0.0, 0.0], [0.0, 0.0], [3, 3])
        assert np.array_equal(adj, nat_adj) and np.array_equal(bits(area), bits(nat_area))
        assert adj[0, 1] == (0 if dx else 1)


@pytest.mark.parametrize("mt,Hp,spread", [(MpaType.single_speed, 6, 3.0), (MpaType.single_speed, 10, 6.0), (MpaType.triple_speed, 8, 4.0)])
def test_python_and_host_twin_couplings_are_bit_identical(tables, mt, Hp, spread):
    mpa, L, _ = tables[(mt, Hp, ScenarioType.commonroad)]
    rng = np.random.default_rng(Hp)
    n = 60
    x, y, yaw, trim = _random_poses(rng, n, mpa.n_trims, spread)
    x[1], y[1], yaw[1], trim[1] = x[0], y[0], yaw[0], trim[0]  # an identical pair
    sets = [R.reachable_sets_at_pose(L, x[i], y[i], yaw[i], int(trim[i]))[-1] for i in range(n)]
    adj, area = R.reachable_set_coupling(sets)
    nat_adj, nat_area = reachable_set_coupling_call(L, x, y, yaw, trim)
    assert np.array_equal(adj, nat_adj) and np.array_equal(bits(area), bits(nat_area))
    assert np.array_equal(adj, adj.T) and not adj.diagonal().any()
    assert adj[0, 1] == 1 and 0 < adj.sum() < n * (n - 1)


# ---- the controllers: native (no handle, oracle as planner) against Python
from test_native_controller import assert_same_problem, run_both  # noqa: E402


def _levels_with_parallel(py):
    return int(np.sum(np.asarray(py.last_directed) != np.asarray(py.last_directed_seq)))


@pytest.mark.parametrize("deal", [False, True])
def test_circle_reachable_set_coupling_twins(deal):
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_nodes=1 << 20, is_deal_prediction_inconsistency=deal)
    py = run_both(options, circle_scenario(options), 10, "reachable_set")
    assert py.last_adjacency.sum() > 0
    run_both(options, circle_scenario(options), 3, "full")


@pytest.mark.parametrize("deal", [False, True])
def test_c2_like_reachable_set_coupling_twins(deal):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=6, max_nodes=1 << 20, is_deal_prediction_inconsistency=deal)
    sc = commonroad_scenario(options, seed=1)
    py = run_both(options, sc, 10, "reachable_set", boundary_provider(sc))
    assert py.last_adjacency.sum() > 0


@pytest.mark.parametrize("deal", [False, True])
def test_c3_like_cut_to_two_levels_twins(deal):
    """Colouring cut to two computation levels: parallel couplings exist, and with is_deal_prediction_inconsistency their predecessors'
    reachable sets enter the searches (from the first step on)."""
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=5, max_num_CLs=2, max_nodes=1 << 20, is_deal_prediction_inconsistency=deal)
    sc = commonroad_scenario(options, seed=2, tiles=2)
    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="reachable_set", boundary_provider=boundary_provider(sc), priority_strategy="coloring")
    nat = NativeController(options, sc, mpa, None, coupling="reachable_set", priority_strategy="coloring")
    nat.build_step()
    prob = py.build_step_problem()
    assert_same_problem(prob, nat.problem(), "first step")
    assert _levels_with_parallel(py) > 0, "no parallel coupling: the test would not exercise the parallel predecessors"
    n_dyn = sum(len(it.dynamic_obstacle_area) for it in prob["iters"])
    assert (n_dyn > 0) == deal  # step 1: only reachable sets can be there (no previous plans yet)
    nat.close()
    py = run_both(options, sc, 10, "reachable_set", boundary_provider(sc), priority_strategy="coloring", weight_strategy="distance")
    assert int(py.last_levels.max()) <= 2


def test_step_without_the_table_is_refused():
    from pdmpc.backend import BackendError
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=3, Hp=5)
    nat = NativeController(options, circle_scenario(options), get_mpa(options), None, coupling="full")
    nat.L.pdmpc_controller_set_parallel_coupling(nat.c, 1)
    with pytest.raises(BackendError, match="set_reachability"):
        nat.build_step()
    nat.close()


def test_explorative_step_in_reachable_set_mode():
    from oracle import oracle
    from pdmpc.explorative import choose_solution, explore_step
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=14, Hp=5, max_num_CLs=3, max_nodes=1 << 30, is_deal_prediction_inconsistency=True)
    sc = commonroad_scenario(options, seed=5)
    mpa = get_mpa(options)
    K = 4
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="reachable_set", boundary_provider=boundary_provider(sc), priority_strategy="coloring")
    nat = NativeController(options, sc, mpa, None, coupling="reachable_set", priority_strategy="coloring")
    for k in range(2):
        nat.explore_build(K, seed=k + 1)
        q = nat.explore_problem()
        base_order = nat.problem()["order"]

        def plan_batch(batch):
            assert_same_problem(batch, q, "explorative step %d" % (k + 1))
            assert batch["instance"] == q["instance"] and batch["vehicle"] == q["vehicle"]
            recs, _ = oracle.plan_step(options, mpa, batch)
            chosen_nat, cost_nat = nat.explore_choose(recs)
            _, cost = choose_solution(batch, recs, options.Hp)
            assert np.array_equal(cost_nat, cost)
            slot = {(p, v): s for s, (p, v) in enumerate(zip(batch["instance"], batch["vehicle"]))}
            nat.apply(recs[[slot[(int(chosen_nat[v]), v)] for v in base_order]])
            plan_batch.chosen_nat = chosen_nat
            return recs

        _, _, chosen = explore_step(py, plan_batch, K)
        assert chosen == plan_batch.chosen_nat.tolist()
        st = nat.state()
        assert np.array_equal(st["x"], np.array([m.x for m in py.meas])) and np.array_equal(st["yaw"], np.array([m.yaw for m in py.meas])), k
    nat.close()


def test_optimal_priority_step_in_reachable_set_mode():
    from pdmpc.road_network import boundary_provider, commonroad_scenario
    from test_optimal_reference import optimal_twins

    options = Config(scenario_type=ScenarioType.commonroad, amount=6, Hp=5, max_num_CLs=2, max_nodes=1 << 30, is_deal_prediction_inconsistency=True)
    sc = commonroad_scenario(options, seed=1)
    optimal_twins(options, sc, "reachable_set", boundary_provider(sc), 2)


def test_reachable_kernel_uses_no_scratch_and_spills_no_vgprs():
    """The coupling kernel's two passes (make resources) use no scratch memory and spill no VGPRs."""
    import re
    import shutil
    import subprocess

    from test_build import CSRC, HIPCC

    if not __import__("os").path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resources"], capture_output=True, text=True, check=True).stdout
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    for kernel in ("pdmpc_reach_pose_kernel", "pdmpc_reach_pairs_kernel"):
        assert kernel in seen, seen.keys()
        assert seen[kernel] == {"scratch": 0, "vgpr_spill": 0}, (kernel, seen[kernel])
