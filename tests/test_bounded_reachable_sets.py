"""Lanelet bounding of the reachable sets and the coupler on simple polygons, without a GPU.

The Python twin (pdmpc.reachability.bound_reachable_set / polygon_overlap_area) and the C++ host twin
(pdmpc_bound_reachable_sets_host / pdmpc_polygon_set_coupling_host) are bit-identical; the bounded sets meet hand-built answers and
are valid (simple, clockwise, inside K and L, with the exact area of K ∩ L); the overlap area of two simple polygons agrees with the
exact answer (tests/exact_geometry.py: ear clipping and Sutherland–Hodgman in fractions.Fraction); the native controller (no handle, oracle as planner) builds the same
step problems as the Python controller with bounding on; and bounding drops couplings that exist only because the sets were not
bounded."""
import math

import numpy as np
import pytest

import exact_geometry as X
from pdmpc import reachability as R
from pdmpc.backend import bound_reachable_sets_call, polygon_set_coupling_call
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa

K_SQ = np.array([[0.0, 0.0, 2.0, 2.0], [0.0, 2.0, 2.0, 0.0]])  # clockwise square [0, 2]^2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _closed(p):
    p = np.asarray(p, dtype=np.float64)
    return np.concatenate([p, p[:, :1]], axis=1)


def _bound(K, L):
    return R.bound_reachable_set(K, R.normalize_lanelet_polygon(L))


def _signed_area(p):
    x, y = p[0], p[1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def _open(p):
    p = np.asarray(p, dtype=np.float64)
    if p.shape[1] > 1 and p[0, 0] == p[0, -1] and p[1, 0] == p[1, -1]:
        return p[:, :-1]
    return p


# ---- closed-loop states: every vehicle's unbounded sets, pose, trim and lanelet polygon of the first steps of a run


def _states(options, sc, n_steps, **kw):
    from oracle import oracle
    from pdmpc.road_network import boundary_provider

    options.is_deal_prediction_inconsistency = True  # (the controller then computes every step's sets)
    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="reachable_set", boundary_provider=boundary_provider(sc), **kw)
    out = []

    def plan_step(prob):
        recs, _ = oracle.plan_step(options, mpa, prob)
        return [info_from_record(recs[i], options.Hp) for i in range(len(recs))]

    for _ in range(n_steps):
        py.step(plan_step=plan_step)
        out.append(
            dict(
                x=py.x0[:, 0].copy(),
                y=py.x0[:, 1].copy(),
                yaw=py.x0[:, 2].copy(),
                trim=py.trims.copy(),
                sets=[list(s) for s in py.reachable_sets],
                lanelets=[R.lanelet_polygon(*b) for b in py.boundary],
            )
        )
    return mpa, out


@pytest.fixture(scope="module")
def closed_loop_states():
    from pdmpc.road_network import commonroad_scenario

    out = []
    o2 = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, mpa_type=MpaType.single_speed, max_nodes=1 << 20)
    out.append(("C2-like", _states(o2, commonroad_scenario(o2, seed=1), 5)))
    o3 = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=8, max_num_CLs=2, max_nodes=1 << 20)
    out.append(("C3-like", _states(o3, commonroad_scenario(o3, seed=2, tiles=2), 5, priority_strategy="coloring")))
    return out


def _python_bound_all(state):
    sets, flags = [], []
    for v in range(len(state["sets"])):
        s, f = R.bound_reachable_sets(state["sets"][v], state["lanelets"][v])
        sets.append(s)
        flags.append(f)
    return sets, np.array(flags, dtype=np.uint8)


def _assert_twins(mpa, x, y, yaw, trim, lanelets, sets_py, flags_py, all_steps=True):
    nat, fl = bound_reachable_sets_call(mpa.local_reachable_sets_conv, x, y, yaw, trim, lanelets, all_steps)
    for v in range(len(x)):
        ref = sets_py[v] if all_steps else sets_py[v][-1:]
        rf = flags_py[v] if all_steps else flags_py[v][-1:]
        assert len(nat[v]) == len(ref)
        for q in range(len(ref)):
            assert nat[v][q].shape == ref[q].shape and np.array_equal(bits(nat[v][q]), bits(ref[q])), (v, q)
            assert int(fl[v, q]) == int(rf[q]), (v, q)
    return nat, fl


# ---- 1. twins


def test_twins_on_closed_loop_states(closed_loop_states):
    seen_flags = set()
    for name, (mpa, states) in closed_loop_states:
        for st in states:
            sets, flags = _python_bound_all(st)
            _assert_twins(mpa, st["x"], st["y"], st["yaw"], st["trim"], st["lanelets"], sets, flags, True)
            _assert_twins(mpa, st["x"], st["y"], st["yaw"], st["trim"], st["lanelets"], sets, flags, False)
            seen_flags |= set(np.unique(flags).tolist())
    assert 0 in seen_flags


@pytest.mark.parametrize("Hp", [8, 10])
def test_twins_on_random_poses_on_lanelet_polygons(closed_loop_states, Hp):
    _, (_, states) = closed_loop_states[0]
    polys = states[0]["lanelets"]
    options = Config(scenario_type=ScenarioType.commonroad, Hp=Hp, mpa_type=MpaType.single_speed)
    mpa = get_mpa(options)
    L = mpa.local_reachable_sets_conv
    rng = np.random.default_rng(Hp)
    n = 48
    lan = [polys[i % len(polys)] for i in range(n)]
    x, y = np.zeros(n), np.zeros(n)
    for i in range(n):
        p = lan[i][:, rng.integers(lan[i].shape[1])]
        x[i], y[i] = p + rng.normal(0.0, 0.15, 2)
    yaw = rng.uniform(-math.pi, math.pi, n)
    trim = rng.integers(1, mpa.n_trims + 1, n)
    lan[0] = None  # not bounded
    lan[1] = lan[1] + 50.0  # far away: restored
    sets, flags = [], []
    for i in range(n):
        s, f = R.bound_reachable_sets(R.reachable_sets_at_pose(L, x[i], y[i], yaw[i], int(trim[i])), lan[i])
        sets.append(s)
        flags.append(f)
    flags = np.array(flags, dtype=np.uint8)
    assert (flags[1] == R.BOUND_RESTORED).all() and (flags[0] == 0).all()
    _assert_twins(mpa, x, y, yaw, trim, lan, sets, flags, True)
    _assert_twins(mpa, x, y, yaw, trim, lan, sets, flags, False)


# ---- 2. known answers


def test_strip_containing_k_returns_k():
    r, f = _bound(K_SQ, np.array([[-1.0, -1.0, 3.0, 3.0], [-1.0, 3.0, 3.0, -1.0]]))
    assert f == 0 and np.array_equal(r, _closed(K_SQ))


def test_small_l_inside_k_returns_l():
    L = np.array([[0.5, 0.5, 1.5, 1.5], [0.5, 1.5, 1.5, 0.5]])
    r, f = _bound(K_SQ, L[:, ::-1])  # given counter-clockwise: normalized
    assert f == 0 and np.array_equal(r, _closed(R.normalize_lanelet_polygon(L[:, ::-1])))
    assert _signed_area(r[:, :-1]) < 0


def test_disjoint_returns_k_restored():
    r, f = _bound(K_SQ, np.array([[5.0, 5.0, 6.0, 6.0], [5.0, 6.0, 6.0, 5.0]]))
    assert f == R.BOUND_RESTORED and np.array_equal(r, _closed(K_SQ))


def test_u_shaped_strip_gives_two_regions_and_keeps_the_larger():
    # two arms through K joined outside it; the lower arm is cut by a notch, so its region has more vertices
    U = np.array([[-1, -1, 0.8, 1.0, 1.2, 2.5, 2.5, -1, -1, 3, 3], [0.2, 0.6, 0.6, 0.4, 0.6, 0.6, 1.4, 1.4, 1.8, 1.8, 0.2]], float)
    U = R.normalize_lanelet_polygon(U)
    r, f = R.bound_reachable_set(K_SQ, U)
    assert f == R.BOUND_MULTIPLE
    assert r.shape[1] == 8  # 7 vertices + closing
    assert np.all(r[1] <= 0.6 + 1e-15)
    assert abs(-_signed_area(r[:, :-1]) - (2 * 0.4 - 0.5 * 0.4 * 0.2)) < 1e-12


def test_u_shaped_tie_keeps_the_region_starting_on_the_smaller_l_edge():
    U = R.normalize_lanelet_polygon(np.array([[-1, -1, 2.5, 2.5, -1, -1, 3, 3], [0.2, 0.6, 0.6, 1.4, 1.4, 1.8, 1.8, 0.2]], float))
    r, f = R.bound_reachable_set(K_SQ, U)
    assert f == R.BOUND_MULTIPLE and r.shape[1] == 5
    assert np.all(r[1] <= 0.6)  # the arm whose chain starts on L edge 0


def test_l_vertex_on_a_k_edge():
    # a triangle whose apex touches K's top edge from outside: a single touching point, K ∩ L has no interior
    r, f = _bound(K_SQ, np.array([[1.0, 0.5, 1.5], [2.0, 3.0, 3.0]]))
    assert f == R.BOUND_RESTORED and np.array_equal(r, _closed(K_SQ))
    # a triangle reaching into K with its apex on the bottom edge
    r, f = _bound(K_SQ, np.array([[1.0, 0.5, 1.5], [0.0, 3.0, 3.0]]))
    assert f == 0
    area = -_signed_area(r[:, :-1])
    assert abs(area - 2.0 / 3.0) < 1e-12  # the apex (1, 0) to y = 2, where the triangle is 2/3 wide
    assert any(px == 1.0 and py == 0.0 for px, py in zip(r[0], r[1]))


def test_l_edge_collinear_with_a_k_edge_in_both_directions():
    same = np.array([[0.0, 0.0, 1.0, 1.0], [-1.0, 3.0, 3.0, -1.0]])  # shares the line x = 0 on K's side
    r, f = _bound(K_SQ, same)
    assert f == 0 and abs(-_signed_area(r[:, :-1]) - 2.0) < 1e-15
    opposite = np.array([[-1.0, -1.0, 0.0, 0.0], [-1.0, 3.0, 3.0, -1.0]])  # touches K along x = 0 from outside
    r, f = _bound(K_SQ, opposite)
    assert f == R.BOUND_RESTORED and np.array_equal(r, _closed(K_SQ))


def test_single_touching_corner():
    r, f = _bound(K_SQ, np.array([[2.0, 2.0, 3.0, 3.0], [2.0, 3.0, 3.0, 2.0]]))
    assert f == R.BOUND_RESTORED and np.array_equal(r, _closed(K_SQ))


def test_degenerate_cases_twins():
    mpa = get_mpa(Config(scenario_type=ScenarioType.commonroad, Hp=8))
    L = mpa.local_reachable_sets_conv
    trim = 3
    K = R.reachable_sets_at_pose(L, 0.0, 0.0, 0.0, trim)
    cases = []
    for q in (0, 3, 7):  # polygons built on K's own vertices and edges: vertex on ∂K, edges along K edges (both directions)
        k = _open(K[q])
        m = k.shape[1]
        a, b = k[:, 0], k[:, 1]
        mid = 0.5 * (a + b)
        out = mid + 2.0 * np.array([-(b - a)[1], (b - a)[0]])
        cases.append(np.array([[a[0], b[0], out[0]], [a[1], b[1], out[1]]]))  # along edge 0, outward: touches only
        cases.append(np.array([[b[0], a[0], k[0, m // 2]], [b[1], a[1], k[1, m // 2]]]))  # along edge 0 reversed, through K
        cases.append(np.array([[mid[0], out[0] + 1.0, out[0] - 1.0], [mid[1], out[1], out[1]]]))  # vertex on the edge
    n = len(cases)
    sets, flags = [], []
    for c in cases:
        s, f = R.bound_reachable_sets(K, c)
        sets.append(s)
        flags.append(f)
    _assert_twins(mpa, np.zeros(n), np.zeros(n), np.zeros(n), np.full(n, trim), cases, sets, np.array(flags, dtype=np.uint8), True)


# ---- 3. validity


def _segments_cross(p, q, r, s):
    def o(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])

    return o(p, q, r) * o(p, q, s) < 0 and o(r, s, p) * o(r, s, q) < 0


def _is_simple(p):
    p = _open(p)
    m = p.shape[1]
    for i in range(m):
        for j in range(i + 2, m):
            if i == 0 and j == m - 1:
                continue
            if _segments_cross(p[:, i], p[:, (i + 1) % m], p[:, j], p[:, (j + 1) % m]):
                return False
    return True


def _inside_convex(p, K, tol):
    K = _open(K)
    kx, ky = K[0], K[1]
    ux, uy = np.roll(kx, -1) - kx, np.roll(ky, -1) - ky
    v = ux[None, :] * (p[1][:, None] - ky[None, :]) - uy[None, :] * (p[0][:, None] - kx[None, :])
    return bool(np.all(v <= tol * np.hypot(ux, uy)[None, :]))


def _dist_to_polygon_boundary(px, py, L):
    L = _open(L)
    ax, ay = L[0], L[1]
    bx, by = np.roll(ax, -1), np.roll(ay, -1)
    dx, dy = bx - ax, by - ay
    t = np.clip(((px - ax) * dx + (py - ay) * dy) / np.maximum(dx * dx + dy * dy, 1e-300), 0.0, 1.0)
    return float(np.min(np.hypot(ax + t * dx - px, ay + t * dy - py)))


def _inside_simple(px, py, L):
    L = _open(L)
    inside = False
    m = L.shape[1]
    for i in range(m):
        j = (i + 1) % m
        if (L[1, i] > py) != (L[1, j] > py):
            xi = L[0, i] + (py - L[1, i]) * (L[0, j] - L[0, i]) / (L[1, j] - L[1, i])
            if px < xi:
                inside = not inside
    return inside


def test_bounded_sets_of_closed_loop_states_are_valid(closed_loop_states):
    checked = multi = 0
    for name, (mpa, states) in closed_loop_states:
        for st in states[:2]:
            for v in range(len(st["sets"])):
                Ln = R.normalize_lanelet_polygon(st["lanelets"][v])
                for q in (0, len(st["sets"][v]) - 1):
                    K = st["sets"][v][q]
                    r, f = R.bound_reachable_set(K, Ln)
                    if f & R.BOUND_RESTORED:
                        continue
                    ro = _open(r)
                    assert _is_simple(r), (name, v, q)
                    assert _signed_area(ro) < 0, (name, v, q)
                    assert _inside_convex(ro, K, 1e-12), (name, v, q)
                    for px, py in zip(ro[0], ro[1]):
                        assert _inside_simple(px, py, Ln) or _dist_to_polygon_boundary(px, py, Ln) <= 1e-12, (name, v, q)
                    full = float(X.area_convex_simple(X.poly(K), X.poly(Ln)))  # exact (tests/exact_geometry.py)
                    area = -_signed_area(ro)
                    assert area <= full * (1 + 1e-12) + 1e-15, (name, v, q)
                    if f & R.BOUND_MULTIPLE:
                        multi += 1
                    else:
                        assert abs(area - full) <= 1e-9 * max(full, 1e-3), (name, v, q, area, full)
                    checked += 1
    assert checked > 100


# ---- 4. overlap area against the exact reference


def _reference_area(A, B):
    """the exact area of A ∩ B (tests/exact_geometry.py: ear clipping and Sutherland–Hodgman in fractions.Fraction)"""
    return float(X.area_simple_simple(X.poly(A), X.poly(B)))


def _star(rng, cx, cy, m, rmin=0.3, rmax=1.0):
    ang = np.sort(rng.uniform(0, 2 * math.pi, m))
    r = rng.uniform(rmin, rmax, m)
    return np.array([cx + r * np.cos(ang), cy + r * np.sin(ang)])[:, ::-1].copy()  # clockwise


def _check_area(A, B):
    got = R.polygon_overlap_area(A, B)
    ref = _reference_area(A, B)
    scale = max(abs(ref), 1e-3 * min(-_signed_area(_open(A)), -_signed_area(_open(B))))
    assert abs(got - ref) <= 1e-9 * scale, (got, ref)
    return got


def test_overlap_area_of_random_star_polygons():
    rng = np.random.default_rng(5)
    for _ in range(40):
        A = _star(rng, 0.0, 0.0, int(rng.integers(5, 25)))
        B = _star(rng, rng.uniform(-1, 1), rng.uniform(-1, 1), int(rng.integers(5, 25)))
        _check_area(A, B)
        _check_area(B, A)


def test_overlap_area_special_cases():
    rng = np.random.default_rng(6)
    A = _star(rng, 0.0, 0.0, 12)
    assert abs(R.polygon_overlap_area(A, A) + _signed_area(A)) <= 1e-12 * abs(_signed_area(A))  # identical
    small = _star(rng, 0.0, 0.0, 9, 0.05, 0.1)
    _check_area(A, small)  # nested
    _check_area(small, A)
    sq = np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 0.0]])
    tall = np.array([[0.0, 0.0, 0.5, 0.5], [0.0, 2.0, 2.0, 0.0]])  # shares the edge x = 0 in the same direction
    assert R.polygon_overlap_area(sq, tall) == 0.5 and R.polygon_overlap_area(tall, sq) == 0.5
    left = np.array([[-1.0, -1.0, 0.0, 0.0], [0.0, 1.0, 1.0, 0.0]])  # shares x = 0 in the opposite direction: touching
    assert R.polygon_overlap_area(sq, left) == 0.0 and R.polygon_overlap_area(left, sq) == 0.0
    corner = sq + 1.0  # one touching point
    assert R.polygon_overlap_area(sq, corner) == 0.0
    notch = np.array([[0.0, 0.0, 0.5, 1.0, 1.0], [0.0, 1.0, 0.5, 1.0, 0.0]])  # non-convex, shares edges with sq
    assert abs(R.polygon_overlap_area(sq, notch) - 0.75) < 1e-15 and abs(R.polygon_overlap_area(notch, sq) - 0.75) < 1e-15


def test_overlap_area_matches_the_convex_rule_on_convex_sets():
    mpa = get_mpa(Config(scenario_type=ScenarioType.commonroad, Hp=8))
    L = mpa.local_reachable_sets_conv
    rng = np.random.default_rng(7)
    hits = 0
    for _ in range(60):
        a = R.reachable_sets_at_pose(L, 0.0, 0.0, rng.uniform(-3, 3), int(rng.integers(1, mpa.n_trims + 1)))[-1]
        b = R.reachable_sets_at_pose(L, rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-3, 3), int(rng.integers(1, mpa.n_trims + 1)))[-1]
        ref = R.overlap_area(a, b)
        got = R.polygon_overlap_area(a, b)
        assert abs(got - ref) <= 1e-12 * max(abs(ref), 1e-12), (got, ref)
        hits += ref > 0
    assert hits > 10


def test_overlap_area_of_bounded_sets(closed_loop_states):
    _, (_, states) = closed_loop_states[0]
    st = states[0]
    sets, _ = _python_bound_all(st)
    last = [s[-1] for s in sets]
    adj, _ = R.polygon_set_coupling(last)
    pairs = list(zip(*np.nonzero(np.triu(adj))))[:4]
    assert pairs
    # bounded sets of two vehicles can run along the same map boundary points, where the triangle sum of the reference is itself
    # degenerate: compare on a copy moved by 1e-7 (general position), and check that the area moves continuously
    shift = np.array([[1e-7], [0.7e-7]])
    for i, j in pairs:
        got = _check_area(last[i], last[j] + shift)
        assert abs(R.polygon_overlap_area(last[i], last[j]) - got) <= 1e-6


# ---- 5. coupling twins


def test_coupling_twins(closed_loop_states):
    for name, (mpa, states) in closed_loop_states:
        for st in states[:3]:
            sets, _ = _python_bound_all(st)
            last = [s[-1] for s in sets]
            adj, area = R.polygon_set_coupling(last)
            nadj, narea = polygon_set_coupling_call(last)
            assert np.array_equal(adj, nadj) and np.array_equal(bits(area), bits(narea)), name


# ---- 6. controllers: native (no handle, oracle as planner) against Python, bounding on
from test_native_controller import assert_same_problem, run_both  # noqa: E402


def test_c2_like_bounded_controllers_are_twins():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=6, max_nodes=1 << 20, is_deal_prediction_inconsistency=True,
                     bound_reachable_sets=True)
    sc = commonroad_scenario(options, seed=1)
    py = run_both(options, sc, 10, "reachable_set", boundary_provider(sc))
    assert py.reachable_sets_bounded and py.last_adjacency.sum() > 0


def test_c3_like_bounded_controllers_cut_to_two_levels_are_twins():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=5, max_num_CLs=2, max_nodes=1 << 20, is_deal_prediction_inconsistency=True,
                     bound_reachable_sets=True)
    sc = commonroad_scenario(options, seed=2, tiles=2)
    py = run_both(options, sc, 10, "reachable_set", boundary_provider(sc), priority_strategy="coloring", weight_strategy="distance")
    assert int(py.last_levels.max()) <= 2


def test_circle_bounding_changes_nothing():
    from pdmpc.native_controller import NativeController
    from pdmpc.scenario import circle_scenario

    problems = []
    for bound in (False, True):
        options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_nodes=1 << 20, is_deal_prediction_inconsistency=True,
                         bound_reachable_sets=bound)
        run_both(options, circle_scenario(options), 3, "reachable_set")
        nat = NativeController(options, circle_scenario(options), get_mpa(options), None, coupling="reachable_set")
        nat.build_step()
        problems.append(nat.problem())
        nat.close()
    assert_same_problem(problems[0], problems[1], "circle, bounding off / on")


def test_explorative_step_with_bounding():
    from oracle import oracle
    from pdmpc.explorative import explore_step
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=14, Hp=5, max_num_CLs=3, max_nodes=1 << 30, is_deal_prediction_inconsistency=True,
                     bound_reachable_sets=True)
    sc = commonroad_scenario(options, seed=5)
    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="reachable_set", boundary_provider=boundary_provider(sc), priority_strategy="coloring")
    nat = NativeController(options, sc, mpa, None, coupling="reachable_set", priority_strategy="coloring")
    nat.explore_build(4, seed=1)
    q = nat.explore_problem()

    def plan_batch(batch):
        assert_same_problem(batch, q, "explorative step")
        recs, _ = oracle.plan_step(options, mpa, batch)
        return recs

    explore_step(py, plan_batch, 4)
    nat.close()


def test_optimal_priority_step_with_bounding():
    from pdmpc.road_network import boundary_provider, commonroad_scenario
    from test_optimal_reference import optimal_twins

    options = Config(scenario_type=ScenarioType.commonroad, amount=6, Hp=5, max_num_CLs=2, max_nodes=1 << 30, is_deal_prediction_inconsistency=True,
                     bound_reachable_sets=True)
    sc = commonroad_scenario(options, seed=1)
    optimal_twins(options, sc, "reachable_set", boundary_provider(sc), 1)


# ---- 7. bounding drops couplings


def test_bounding_drops_couplings_on_the_first_c2_step():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    counts = []
    for bound in (False, True):
        options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, mpa_type=MpaType.single_speed, bound_reachable_sets=bound)
        sc = commonroad_scenario(options, seed=1)
        py = PrioritizedSequentialController(options, sc, get_mpa(options), None, coupling="reachable_set", boundary_provider=boundary_provider(sc))
        py._traffic_info()
        counts.append(int(py._couple().sum()) // 2)
    assert counts[0] == 32
    assert counts[1] < counts[0], counts


# ---- 8. resources


def test_bounded_kernels_use_no_scratch_and_spill_no_vgprs():
    """The bounding kernel and the two passes of the bounded coupler (make resources) use no scratch memory and spill no VGPRs."""
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
    for kernel in ("pdmpc_bound_sets_kernel", "pdmpc_bounded_box_kernel", "pdmpc_bounded_pairs_kernel"):
        assert kernel in seen, seen.keys()
        assert seen[kernel] == {"scratch": 0, "vgpr_spill": 0}, (kernel, seen[kernel])
