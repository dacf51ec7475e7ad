"""Optimal-priority control on the device: the enumeration kernel (pdmpc_unique_priorities, csrc/priority_kernel.hip) against its
host twin, and the native optimal-priority step (every unique prioritization in ONE launch) against pdmpc.optimal planned by the
oracle."""
import copy
import os

import numpy as np
import pytest

from pdmpc.backend import CapacityError, Handle, unique_priorities_call
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.mpa import get_mpa

from test_gpu_parity import assert_records_equal
from test_optimal_reference import complete, random_graph

pytestmark = pytest.mark.gpu


def masks_of(prio, A):
    """The orientation of every priority column as a mask (edge e flipped <=> bit E - 1 - e)."""
    n = A.shape[0]
    edges = [(r, c) for c in range(n) for r in range(c) if A[r, c]]
    E = len(edges)
    m = np.zeros(prio.shape[1], dtype=np.int64)
    for e, (r, c) in enumerate(edges):
        m |= (prio[r] > prio[c]).astype(np.int64) << (E - 1 - e)
    return m


@pytest.mark.timeout(300)
def test_kernel_equals_the_host_twin():
    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 12)
    h = Handle(options)
    rng = np.random.default_rng(17)
    graphs = [np.zeros((1, 1)), np.zeros((6, 6)), complete(3), complete(5)]
    graphs += [random_graph(rng, int(rng.integers(2, 12)), 20) for _ in range(10)]
    A = np.zeros((9, 9), dtype=np.int64)  # 24 edges
    pairs = [(r, c) for c in range(9) for r in range(c)][:24]
    for r, c in pairs:
        A[r, c] = A[c, r] = 1
    graphs.append(A)
    for A in graphs:
        with pytest.raises(CapacityError) as e:
            h.unique_priorities(A, 0)
        want_p, want_m = unique_priorities_call(A, e.value.count)
        got_p, got_m = h.unique_priorities(A, len(want_m))
        assert np.array_equal(got_m, want_m) and np.array_equal(got_p, want_p), A
    # K_7 (E = 21) and K_8 (E = 28): n! orientations, each acyclic (its priorities give back its mask), distinct and ascending
    import math

    for n in (7, 8):
        prio, masks = h.unique_priorities(complete(n), 50000)
        assert len(masks) == math.factorial(n)
        assert (np.diff(masks) > 0).all()
        assert np.array_equal(masks_of(prio, complete(n)), masks)
        assert np.array_equal(np.sort(prio, axis=0), np.tile(np.arange(1, n + 1)[:, None], (1, len(masks))))
    with pytest.raises(CapacityError) as e:
        h.unique_priorities(complete(7), 5039)
    assert e.value.count == 5040
    h.close()


def optimal_closed_loop(options, sc, coupling, boundary, n_steps, K_expected=None):
    """pdmpc_controller_optimal_step next to pdmpc.optimal.optimal_step planned by the oracle: records of every batch, chosen
    instances and plant state equal; then optimal_run (lean read-back) drives the same closed loop."""
    from oracle import oracle
    from pdmpc.native_controller import NativeController
    from pdmpc.optimal import optimal_step
    from pdmpc.optimizer import GraphSearchHip

    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, sc, mpa, opt.handle, coupling=coupling)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling=coupling, boundary_provider=boundary)
    unbounded = copy.copy(options)
    unbounded.max_nodes = 1 << 30
    other = 0
    for k in range(n_steps):
        gpu, chosen_nat = nat.optimal_step(options.max_vehicles // options.amount)
        batch, ref, chosen = optimal_step(py, lambda b: oracle.plan_step(unbounded, mpa, b, n_threads=min(16, os.cpu_count() or 1))[0],
                                          options.max_vehicles // options.amount)
        if K_expected is not None:
            assert batch["n_instances"] == K_expected
        assert_records_equal(gpu, ref, "optimal step %d" % (k + 1))
        assert chosen_nat.tolist() == chosen, k
        other += sum(1 for c in chosen if c != 0)
        st = nat.state()
        for key, attr in (("x", "x"), ("y", "y"), ("yaw", "yaw"), ("speed", "speed")):
            assert np.array_equal(st[key], np.array([getattr(m, attr) for m in py.meas])), (k, key)
    nat2 = NativeController(options, sc, mpa, opt.handle, coupling=coupling)
    ms = nat2.optimal_run(options.max_vehicles // options.amount, n_steps)
    assert len(ms) == n_steps and (ms > 0).all()
    a, b = nat.state(), nat2.state()
    for key in ("x", "y", "yaw", "speed", "steering"):
        assert np.array_equal(a[key], b[key]), key
    nat2.close()
    nat.close()
    opt.handle.close()
    return other


@pytest.mark.timeout(300)
def test_optimal_step_circle_three_vehicles():
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=3, Hp=5, max_vehicles=3 * 6, max_nodes=1 << 15)
    optimal_closed_loop(options, circle_scenario(options), "full", None, 20, K_expected=6)  # (symmetric: every step ties, instance 0)


@pytest.mark.timeout(300)
def test_optimal_step_circle_four_vehicles():
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=4 * 24, max_nodes=1 << 15)
    optimal_closed_loop(options, circle_scenario(options), "full", None, 6, K_expected=24)


@pytest.mark.timeout(300)
def test_optimal_step_road_network_six_vehicles():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=6, Hp=6, max_vehicles=6 * 200, max_nodes=1 << 14)  # (K = 108 to 162 here)
    sc = commonroad_scenario(options, seed=1)
    assert optimal_closed_loop(options, sc, "distance", boundary_provider(sc), 4) > 0  # (step 1 chooses instance 1)


@pytest.mark.timeout(300)
def test_optimal_step_without_coupling_is_the_sequential_step():
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=4, max_nodes=1 << 15)
    sc = circle_scenario(options)
    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    a = NativeController(options, sc, mpa, opt.handle, coupling="none")
    b = NativeController(options, sc, mpa, opt.handle, coupling="none")
    for k in range(5):
        recs, chosen = a.optimal_step(1)
        ref = b.step()
        assert chosen.tolist() == [0] * 4
        assert_records_equal(recs, ref, "step %d" % (k + 1))
        sa, sb = a.state(), b.state()
        for key in ("x", "y", "yaw", "speed", "steering"):
            assert np.array_equal(sa[key], sb[key]), (k, key)
    a.close()
    b.close()
    opt.handle.close()
