"""Optimal-priority control without a GPU: Prioritizer.unique_priorities restated (pdmpc.optimal) and its native twin
(pdmpc_unique_priorities_host), the flattened batch of every unique prioritization built natively (pdmpc_controller_optimal_build
without a handle) against pdmpc.optimal.build_optimal_batch, and the per-vehicle choice of PrioritizedOptimalController.m:56-114."""
import itertools

import numpy as np
import pytest

from pdmpc.backend import CapacityError, unique_priorities_call
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController, directed_coupling_from_priorities
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController
from pdmpc.optimal import choose_from_costs, choose_solution, optimal_step, unique_priorities

from test_native_controller import assert_same_problem


def complete(n):
    return np.ones((n, n), dtype=np.int64) - np.eye(n, dtype=np.int64)


def random_graph(rng, n, max_edges):
    A = np.zeros((n, n), dtype=np.int64)
    pairs = [(r, c) for c in range(n) for r in range(c)]
    m = int(rng.integers(0, min(max_edges, len(pairs)) + 1))
    for q in rng.choice(len(pairs), size=m, replace=False):
        r, c = pairs[q]
        A[r, c] = A[c, r] = 1
    return A


def chromatic_at_minus_one(A):
    """|chi_G(-1)| by deletion-contraction: chi_G(k) = chi_{G-e}(k) - chi_{G/e}(k) (Stanley: the number of acyclic orientations)."""

    def chi(n, edges):  # edges: frozenset of (a, b), a < b, over vertices 0..n-1; value at k = -1
        if not edges:
            return (-1) ** n
        e = min(edges)
        a, b = e
        rest = edges - {e}
        merged = set()
        for x, y in rest:  # contract b into a, then renumber the vertices above b
            x, y = (a if x == b else x), (a if y == b else y)
            if x != y:
                x, y = (x - (x > b)), (y - (y > b))
                merged.add((min(x, y), max(x, y)))
        return chi(n, rest) - chi(n - 1, frozenset(merged))

    n = A.shape[0]
    edges = frozenset((r, c) for c in range(n) for r in range(c) if A[r, c])
    return abs(chi(n, edges))


def test_triangle_masks_and_priorities():
    """K_3: edges (1,2), (1,3), (2,3); masks 2 and 5 are the two 3-cycles."""
    prio, masks = unique_priorities(complete(3))
    assert masks.tolist() == [0, 1, 3, 4, 6, 7]
    assert prio.T.tolist() == [[1, 2, 3], [1, 3, 2], [2, 3, 1], [2, 1, 3], [3, 1, 2], [3, 2, 1]]
    assert prio.shape == (3, 6)  # n x K like MATLAB


@pytest.mark.parametrize("n", range(1, 7))
def test_complete_graph_gives_n_factorial(n):
    import math

    prio, masks = unique_priorities(complete(n))
    assert len(masks) == math.factorial(n)
    assert sorted(map(tuple, prio.T.tolist())) == sorted(itertools.permutations(range(1, n + 1)))


@pytest.mark.parametrize("n", [3, 4, 5, 7])
def test_cycle_and_forest_counts(n):
    C = np.zeros((n, n), dtype=np.int64)
    for v in range(n):
        C[v, (v + 1) % n] = C[(v + 1) % n, v] = 1
    assert len(unique_priorities(C)[1]) == 2 ** n - 2
    F = np.zeros((n + 3, n + 3), dtype=np.int64)  # a path over n vertices plus a star over the next three, one vertex alone
    for v in range(n - 1):
        F[v, v + 1] = F[v + 1, v] = 1
    F[n, n + 1] = F[n + 1, n] = F[n, n + 2] = F[n + 2, n] = 1
    assert len(unique_priorities(F)[1]) == 2 ** (n - 1 + 2)


def test_no_edges_gives_one_instance():
    prio, masks = unique_priorities(np.zeros((5, 5)))
    assert masks.tolist() == [0] and prio[:, 0].tolist() == [1, 2, 3, 4, 5]
    prio, masks = unique_priorities_call(np.zeros((5, 5)), 4)
    assert masks.tolist() == [0] and prio[:, 0].tolist() == [1, 2, 3, 4, 5]


def test_random_graph_counts_equal_the_chromatic_polynomial_at_minus_one():
    rng = np.random.default_rng(7)
    for _ in range(12):
        A = random_graph(rng, int(rng.integers(2, 8)), 11)
        assert len(unique_priorities(A)[1]) == chromatic_at_minus_one(A)


def test_masks_ascend_and_priorities_give_back_every_orientation():
    rng = np.random.default_rng(3)
    for A in [complete(5)] + [random_graph(rng, 6, 10) for _ in range(6)]:
        prio, masks = unique_priorities(A)
        assert (np.diff(masks) > 0).all()
        n = A.shape[0]
        edges = [(r, c) for c in range(n) for r in range(c) if A[r, c]]
        E = len(edges)
        for k, m in enumerate(masks):
            d = directed_coupling_from_priorities(A, prio[:, k])
            for e, (r, c) in enumerate(edges):
                flipped = (int(m) >> (E - 1 - e)) & 1
                assert (d[r, c], d[c, r]) == ((0, 1) if flipped else (1, 0)), (k, e)


def test_native_twin_equals_the_restatement():
    rng = np.random.default_rng(11)
    graphs = [complete(4), complete(6), np.zeros((3, 3))] + [random_graph(rng, int(rng.integers(2, 10)), 16) for _ in range(14)]
    for A in graphs:
        want_p, want_m = unique_priorities(A)
        got_p, got_m = unique_priorities_call(A, len(want_m))
        assert np.array_equal(got_m, want_m) and np.array_equal(got_p, want_p)


def test_capacity_errors_report_the_true_count():
    with pytest.raises(CapacityError) as e:
        unique_priorities_call(complete(5), 119)
    assert e.value.count == 120
    prio, _ = unique_priorities_call(complete(5), 120)
    assert prio.shape == (5, 120)
    A = np.zeros((40, 40), dtype=np.int64)  # 33 edges: a path over 34 vertices
    for v in range(33):
        A[v, v + 1] = A[v + 1, v] = 1
    with pytest.raises(CapacityError) as e:
        unique_priorities_call(A, 10)
    assert e.value.count == -1
    with pytest.raises(CapacityError) as e:
        unique_priorities_call(np.zeros((65, 65)), 10)
    assert e.value.count == -1
    with pytest.raises(CapacityError):
        unique_priorities_call(np.zeros((64, 64)), 0)  # K = 1 > max_out = 0
    assert unique_priorities_call(np.zeros((64, 64)), 1)[0][:, 0].tolist() == list(range(1, 65))


def test_choice_on_synthetic_tables():
    # a tie picks the first instance, for every vehicle
    chosen, cost = choose_from_costs(np.array([[1.0, 2.0], [3.0, 0.0], [0.5, 2.5]]))
    assert chosen == [0, 0] and cost.shape == (2, 3)
    # an exhausted search makes its instance infinitely expensive; if every instance has one, the first
    chosen, _ = choose_from_costs(np.array([[1.0, np.inf], [9.0, 9.0]]))
    assert chosen == [1, 1]
    chosen, cost = choose_from_costs(np.array([[np.inf, 1.0], [1.0, np.inf]]))
    assert chosen == [0, 0] and np.isinf(cost).all()
    # summation order: v's own cost first, then the others by ascending index -- in floating point the vehicles' sums may differ
    val = np.array([[1e16, 1.0, 1.0], [1e16, 1.0, 1.0]])
    _, cost = choose_from_costs(val)
    assert cost[0, 0] == (1e16 + 1.0) + 1.0 == 1e16 and cost[1, 0] == (1.0 + 1e16) + 1.0 == 1e16
    val = np.array([[1.0, 1.0, -1e16, 1e16]])
    _, cost = choose_from_costs(val)
    assert cost[:, 0].tolist() == [round(((1.0 + 1.0) - 1e16) + 1e16, 8), round(((1.0 + 1.0) - 1e16) + 1e16, 8),
                                   round(((-1e16 + 1.0) + 1.0) + 1e16, 8), round(((1e16 + 1.0) + 1.0) - 1e16, 8)]
    assert cost[0, 0] != cost[2, 0]


def test_vehicles_whose_summation_orders_round_differently_choose_differently():
    """Instance 1's three costs sum to a value next to a rounding boundary of round(., 8): vehicle 1 adds (x + y) + z, vehicle 3
    adds (z + x) + y, and the two sums round to neighbouring multiples of 1e-8.  Instance 0 costs the larger of them for everyone, so
    one vehicle prefers instance 1 and the other ties and keeps the first instance -- the choice is per vehicle, as in the reference."""
    rng = np.random.default_rng(5)
    for _ in range(100000):
        x, y = rng.uniform(0, 1, 2)
        z = (np.round(x + y + 0.7, 8) + 0.5e-8) - x - y
        low, high = sorted((np.round((x + y) + z, 8), np.round((z + x) + y, 8)))
        if low != high:
            break
    else:
        pytest.fail("no costs found that round differently")
    chosen, cost = choose_from_costs(np.array([[high, 0.0, 0.0], [x, y, z]]))
    assert cost[0].tolist() == [high, np.round((x + y) + z, 8)] and cost[2].tolist() == [high, np.round((z + x) + y, 8)]
    assert chosen[0] != chosen[2] and sorted({chosen[0], chosen[2]}) == [0, 1]


def optimal_twins(options, sc, coupling, boundary, n_steps, K_expected=None):
    """Native batch (no handle) == Python batch slot for slot, the native choice == the Python choice, closed loops equal."""
    from oracle import oracle

    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling=coupling, boundary_provider=boundary)
    nat = NativeController(options, sc, mpa, None, coupling=coupling)
    base = NativeController(options, sc, mpa, None, coupling=coupling)
    seen = {"other": 0, "cut": 0}
    for k in range(n_steps):
        K = nat.optimal_build(1000)
        if K_expected is not None:
            assert K == K_expected
        q = nat.optimal_problem()
        base.build_step()
        own = base.problem()

        def plan_batch(batch):
            assert batch["n_instances"] == K
            assert_same_problem(batch, q, "optimal step %d" % (k + 1))
            assert batch["instance"] == q["instance"] and batch["vehicle"] == q["vehicle"]
            # instance 0 is the constant-priority step problem
            zero = [s for s, p in enumerate(batch["instance"]) if p == 0]
            inst0 = {"order": [batch["vehicle"][s] for s in zero], "iters": [batch["iters"][s] for s in zero], "fallback": [batch["fallback"][s] for s in zero],
                     "preds": [[zero.index(t) for t in batch["preds"][s]] for s in zero], "levels": [batch["levels"][s] for s in zero]}
            inst0["level_sizes"] = [inst0["levels"].count(l) for l in range(1, max(inst0["levels"]) + 1)]
            if k == 0:  # (later steps: the traffic state follows the chosen plans, the constant-priority controller's does not)
                assert_same_problem(inst0, own, "instance 0 of step %d" % (k + 1))
            seen["cut"] += int(max(batch["levels"]) < options.amount)
            recs, _ = oracle.plan_step(options, mpa, batch)
            chosen_nat, cost_nat = nat.optimal_choose(recs)
            want, cost = choose_solution(batch, recs, options.Hp)
            assert np.array_equal(cost_nat, cost) and chosen_nat.tolist() == want
            slot = {(p, v): s for s, (p, v) in enumerate(zip(batch["instance"], batch["vehicle"]))}
            nat.apply(recs[[slot[(int(chosen_nat[v]), v)] for v in q_order]])
            return recs

        q_order = nat.problem()["order"]
        _, _, chosen = optimal_step(py, plan_batch, 1000)
        seen["other"] += sum(1 for c in chosen if c != 0)
        st = nat.state()
        assert np.array_equal(st["x"], np.array([m.x for m in py.meas])) and np.array_equal(st["y"], np.array([m.y for m in py.meas])), k
        assert np.array_equal(st["yaw"], np.array([m.yaw for m in py.meas])) and np.array_equal(st["speed"], np.array([m.speed for m in py.meas])), k
        assert st["needs_fallback"].tolist() == [bool(i.needs_fallback) for i in py.infos], k
    nat.close()
    base.close()
    return seen


@pytest.mark.parametrize("amount,max_levels", [(3, 99), (4, 99), (4, 2)])
def test_native_batch_equals_the_python_batch_on_the_circle(amount, max_levels):
    from pdmpc.scenario import circle_scenario

    import math

    options = Config(scenario_type=ScenarioType.circle, amount=amount, Hp=5, max_num_CLs=max_levels, max_nodes=1 << 30)
    seen = optimal_twins(options, circle_scenario(options), "full", None, 3, K_expected=math.factorial(amount))
    if max_levels < amount:
        assert seen["cut"] > 0


@pytest.mark.parametrize("max_levels", [99, 2])
def test_native_batch_equals_the_python_batch_on_a_road_network(max_levels):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=6, Hp=5, max_num_CLs=max_levels, max_nodes=1 << 30)
    sc = commonroad_scenario(options, seed=1)
    optimal_twins(options, sc, "distance", boundary_provider(sc), 3)
