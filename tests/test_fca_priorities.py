"""Random and FCA prioritization and random weights in the native step controller, without a GPU: the host twin of
the collision assessment (pdmpc_fca_collisions_host) against pdmpc.prioritizer.fca_priorities, and the native controller against the
Python controller step for step (tests/test_native_controller.py's harness, planned by the oracle)."""
import math

import numpy as np
import pytest

from pdmpc.backend import BackendError, fca_collisions_host, fca_pairs
from pdmpc.config import Config, ScenarioType
from pdmpc.mpa import VEHICLE_LENGTH, VEHICLE_WIDTH, get_mpa
from pdmpc.prioritizer import fca_priorities

from test_native_controller import run_both

L_, W_, OFF = VEHICLE_LENGTH, VEHICLE_WIDTH, 0.01


def _traffic(rng, n, Hp, side):
    """n straight reference trajectories of Hp points, dense enough that footprints meet."""
    refs = []
    for _ in range(n):
        x0, y0 = rng.uniform(0, side, 2)
        a = rng.uniform(-math.pi, math.pi)
        t = np.arange(Hp) * rng.uniform(0.02, 0.08)
        bend = rng.uniform(-0.3, 0.3) * t * t
        refs.append(np.stack([x0 + math.cos(a) * t - math.sin(a) * bend, y0 + math.sin(a) * t + math.cos(a) * bend], axis=1))
    return refs


def _box(rng, side, size):
    x, y = rng.uniform(0, side, 2)
    return np.array([[x, x + size, x + size, x], [y, y, y + size, y + size]])


def _coupling(kind, rng, n, refs):
    if kind == "full":
        return np.ones((n, n), dtype=np.int64) - np.eye(n, dtype=np.int64)
    if kind == "none":
        return np.zeros((n, n), dtype=np.int64)
    p = np.array([r[0] for r in refs])
    d = np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1])
    A = (d <= 0.8).astype(np.int64)
    np.fill_diagonal(A, 0)
    return A


@pytest.mark.parametrize("coupling", ["full", "distance", "none"])
@pytest.mark.parametrize("n", [1, 2, 3, 20, 128])
def test_host_twin_equals_python_twin(n, coupling):
    rng = np.random.default_rng(1000 * n + len(coupling))
    Hp = 7
    side = max(0.5, math.sqrt(n) * 0.35)
    refs = _traffic(rng, n, Hp, side)
    A = _coupling(coupling, rng, n, refs)
    obstacles = [_box(rng, side, 0.15) for _ in range(3)]
    dynamic = [[_box(rng, side, 0.1) for _ in range(Hp)] for _ in range(2)]
    for obst, dyn in (((), ()), (obstacles, ()), ((), dynamic), (obstacles, dynamic)):
        want_prio, want = fca_priorities(A, refs, L_, W_, OFF, obst, dyn)
        got, prio = fca_collisions_host(refs, fca_pairs(A), L_, W_, OFF, obst, dyn)
        assert np.array_equal(got, np.asarray(want, dtype=np.int64)), (n, coupling, len(obst), len(dyn))
        assert prio.tolist() == list(want_prio)
    if n >= 20 and coupling != "none":
        assert got.sum() > 0, "no collision at all: the case tests nothing"


def test_ties_keep_index_order_and_the_last_vehicle_skips_obstacles():
    Hp = 4
    far = [np.stack([np.arange(Hp) * 0.05 + 10 * v, np.zeros(Hp)], axis=1) for v in range(5)]
    coll, prio = fca_collisions_host(far, fca_pairs(np.ones((5, 5)) - np.eye(5)), L_, W_, OFF)
    assert coll.tolist() == [0] * 5 and prio.tolist() == [1, 2, 3, 4, 5]
    # an obstacle under the last vehicle only: the reference's outer loop never reaches it
    under_last = [np.array([[39.9, 40.2, 40.2, 39.9], [-0.1, -0.1, 0.1, 0.1]])]
    coll, prio = fca_collisions_host(far, np.zeros((0, 2)), L_, W_, OFF, under_last)
    assert coll.tolist() == [0] * 5
    coll, prio = fca_collisions_host(far[::-1], np.zeros((0, 2)), L_, W_, OFF, under_last)
    assert coll.tolist() == [Hp, 0, 0, 0, 0] and prio.tolist() == [1, 2, 3, 4, 5]
    # the sort index, not the rank: counts (0, 2, 1) -> index vector (2, 3, 1), as the reference passes it on
    refs = [far[4], np.stack([np.arange(Hp) * 0.05, np.zeros(Hp)], axis=1), np.stack([np.arange(Hp) * 0.05 + 0.1, np.zeros(Hp)], axis=1)]
    coll, prio = fca_collisions_host(refs, [[1, 2]], L_, W_, OFF, [_box(np.random.default_rng(0), 0, 0.01) + [[0.2], [0.0]]])
    want_prio, want = fca_priorities(np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0]]), refs, L_, W_, OFF, [_box(np.random.default_rng(0), 0, 0.01) + [[0.2], [0.0]]])
    assert coll.tolist() == [int(c) for c in want] and prio.tolist() == want_prio
    assert coll[1] > coll[2] > 0 == coll[0] and prio.tolist() == [2, 3, 1]


def test_bad_arguments_are_rejected():
    Hp = 3
    refs = [np.stack([np.arange(Hp) * 0.05 + v, np.zeros(Hp)], axis=1) for v in range(3)]
    with pytest.raises(BackendError):  # Hp 1: calculate_yaw needs two points
        fca_collisions_host([r[:1] for r in refs], np.zeros((0, 2)), L_, W_, OFF)
    for bad in ([[1, 0]], [[0, 0]], [[0, 3]], [[-1, 2]], [[0, 2], [0, 1]], [[0, 1], [0, 1]]):
        with pytest.raises(BackendError):
            fca_collisions_host(refs, bad, L_, W_, OFF)
    with pytest.raises(BackendError):  # dynamic rows must hold Hp polygons each
        fca_collisions_host(refs, [[0, 1]], L_, W_, OFF, (), [[_box(np.random.default_rng(0), 1, 0.1)] * (Hp - 1)])
    coll, prio = fca_collisions_host(refs, [[0, 1], [0, 2], [1, 2]], L_, W_, OFF)
    assert prio.tolist() == [1, 2, 3]


def _c2():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=6, max_nodes=1 << 20)
    sc = commonroad_scenario(options, seed=1)
    return options, sc, boundary_provider(sc)


@pytest.mark.parametrize("strategy", ["random", "fca"])
def test_native_twin_c2_like(strategy):
    options, sc, boundary = _c2()
    py = run_both(options, sc, 6, "distance", boundary, priority_strategy=strategy)
    assert py.last_adjacency.sum() > 0


@pytest.mark.parametrize("strategy", ["random", "fca"])
def test_native_twin_c3_like(strategy):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=5, max_nodes=1 << 20)
    sc = commonroad_scenario(options, seed=2, tiles=2)
    run_both(options, sc, 4, "distance", boundary_provider(sc), priority_strategy=strategy)


@pytest.mark.parametrize("strategy", ["random", "fca"])
def test_native_twin_circle(strategy):
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_nodes=1 << 20)
    run_both(options, circle_scenario(options), 5, "full", priority_strategy=strategy)


@pytest.mark.parametrize("max_levels", [2, 3])
def test_native_twin_random_weights_cut(max_levels):
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=40, Hp=5, max_num_CLs=max_levels, max_nodes=1 << 20)
    sc = commonroad_scenario(options, seed=2, tiles=2)
    py = run_both(options, sc, 4, "distance", boundary_provider(sc), weight_strategy="random")
    assert int(py.last_levels.max()) <= max_levels
    assert (np.asarray(py.last_directed) != np.asarray(py.last_directed_seq)).any(), "nothing was cut: the weights decide nothing"


def test_fca_priorities_differ_from_constant_ones():
    """FCA reorders the vehicles of the C2-like first step (otherwise the twin tests above would not tell FCA from constant)."""
    from pdmpc.controller import PrioritizedSequentialController

    options, sc, boundary = _c2()
    mpa = get_mpa(options)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary, priority_strategy="fca")
    ctl.k = 1
    ctl._traffic_info()
    A = ctl._couple()
    prio, coll = fca_priorities(A, ctl.ref_points, sc.vehicles[0].Length, sc.vehicles[0].Width, options.offset, sc.obstacles)
    assert coll.sum() > 0 and prio != list(range(1, options.amount + 1))


@pytest.mark.parametrize("strategy", ["fca", "random"])
def test_native_controller_constructs_and_steps(strategy):
    from oracle import oracle
    from pdmpc.native_controller import NativeController
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_nodes=1 << 20)
    mpa = get_mpa(options)
    nat = NativeController(options, circle_scenario(options), mpa, None, coupling="full", priority_strategy=strategy, weight_strategy="random")
    try:
        for _ in range(2):
            nat.build_step()
            prob = nat.problem()
            recs, _ = oracle.plan_step(options, mpa, prob)
            nat.apply(recs)
        assert len(prob["order"]) == options.amount
    finally:
        nat.close()


def test_fca_kernels_use_no_scratch_memory_and_spill_nothing():
    """`make resources` lists both passes of fca_kernel.hip without scratch memory or spills (hipcc cross-compiles: no GPU needed)."""
    import os
    import re
    import shutil
    import subprocess

    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "p-dmpc_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "resources"], capture_output=True, text=True, check=True).stdout
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    for kernel in ("pdmpc_fca_footprint_kernel", "pdmpc_fca_items_kernel"):
        assert kernel in seen, sorted(seen)
        assert seen[kernel] == {"scratch": 0, "vgpr_spill": 0, "sgpr_spill": 0}, (kernel, seen[kernel])
