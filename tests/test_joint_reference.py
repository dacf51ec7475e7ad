"""The CPU restatement of the joint search (tests/joint_reference.py) and the centralized controller on top of it (no GPU).

The reference is pinned to the oracle: with one vehicle per problem its records are byte-identical to oracle.plan_batch's, and its
heap pops in the order of the oracle's std::priority_queue.  The GPU tests (tests/test_gpu_joint.py) compare the kernel with it.
"""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.centralized import CentralizedController, CentralizedExhaustedError, centralized_mpa, centralized_options
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.iteration_data import VehicleIter, info_from_record
from pdmpc.scenario import circle_scenario

import joint_reference as jr
import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")


def assert_records_equal(a, b, ctx=""):
    assert a.dtype == b.dtype
    for name in a.dtype.names:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        same = (x.view(np.uint64) == y.view(np.uint64)) if x.dtype.kind == "f" else (x == y)
        assert np.all(same), "%s field %s differs at %s" % (ctx, name, np.argwhere(~same)[:5])


def _oracle():
    from oracle import oracle

    return oracle


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_heap_pops_like_the_reference_priority_queue(seed):
    """libstdc++'s push_heap / pop_heap restated: the same pops as the oracle's std::priority_queue on scripts full of equal keys."""
    rng = np.random.default_rng(seed)
    n = 4000
    ops = (rng.random(n) < 0.4).astype(np.int32)
    ids = np.arange(1, n + 1, dtype=np.int32)
    keys = rng.integers(0, 6, n).astype(np.float64) * 0.25  # six distinct keys: nearly every pop meets ties
    got = jr.pq_script(ops, ids, keys)
    want = _oracle().pq_script(ops, ids, keys)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("seed,Hp", [(0, 5), (1, 6), (2, 6), (5, 4)])
def test_single_vehicle_problems_reproduce_the_oracle(seed, Hp):
    """N = 1 is today's separating-axis search: records byte-identical to oracle.plan_batch."""
    options, mpa, iters = problems.problem_set("sat", seed, 8, Hp=Hp)
    _, want, _ = _oracle().plan_batch(options, mpa, iters)
    got = jr.plan_joint(options, mpa, [[it] for it in iters], max_nodes=jr.arena_nodes(options))
    assert_records_equal(got, want, "seed %d Hp %d" % (seed, Hp))


def _cartprod_matlab(*sets):
    """cartprod.m with ind2subVect.m, literally (1-based MATLAB indices)."""
    sizes = [len(s) for s in sets]
    rows = []
    for i in range(1, int(np.prod(sizes)) + 1):
        k = [1] + list(np.cumprod(sizes[:-1]))
        ndx = i - 1
        ix = [0] * len(sizes)
        for q in range(len(sizes) - 1, -1, -1):
            ix[q] = ndx // k[q] + 1
            ndx = ndx % k[q]
        rows.append([sorted(sets[q])[ix[q] - 1] for q in range(len(sets))])
    return np.array(rows, dtype=np.int64).reshape(-1, len(sets))


def test_child_order_is_the_reference_cartprod_order():
    """expand_node.m:15-41: successor ids = sum(cartprod(per-vehicle lists scaled by the trim counts)), then trim_tuple(id, :)
    with trim_tuple = cartprod(1:n, ..., 1:n) (MotionPrimitiveAutomaton.m:141)."""
    options = centralized_options(Config(scenario_type=ScenarioType.circle, amount=3, Hp=4, mpa_type=MpaType.single_speed))
    mpa = centralized_mpa(options)
    jm = jr.JointMpa(mpa)
    n = jm.n
    for trims, k_exp in (((1, 1, 1), 1), ((2, 5, 1), 2), ((3, 3), 3), ((7,), 1)):
        per = [jm.successors(t, k_exp) for t in trims]
        N = len(trims)
        scaled = [np.array(per[0])] + [(np.array(per[v]) - 1) * n**v for v in range(1, N)]
        ids = _cartprod_matlab(*scaled).sum(axis=1)
        trim_tuple = _cartprod_matlab(*[list(range(1, n + 1))] * N)
        want = [tuple(int(t) for t in trim_tuple[i - 1]) for i in ids]
        assert jr.child_tuples(per) == want


def _straight_trim(mpa):
    return [i + 1 for i, t in enumerate(mpa.trims) if t.steering == 0 and t.speed > 0][-1]


def crossing_problem(options, mpa):
    """Two vehicles on perpendicular straight references that reach the crossing point at the same step."""
    Hp = options.Hp
    trim = _straight_trim(mpa)
    v = mpa.trims[trim - 1].speed
    step = v * options.dt_seconds
    d = 3 * step
    out = []
    for yaw in (0.0, math.pi / 2):
        c, s = math.cos(yaw), math.sin(yaw)
        x0, y0 = -d * c, -d * s
        ref = np.array([[x0 + c * step * (k + 1), y0 + s * step * (k + 1)] for k in range(Hp)])
        out.append(
            VehicleIter(
                x0=np.array([x0, y0, yaw, v]),
                trim_index=trim,
                reference_trajectory_points=ref,
                v_ref=np.full(Hp, v),
                amount=2,
            )
        )
    return out


def test_crossing_vehicles_keep_clear_of_each_other():
    """Each vehicle's own optimum drives through the crossing at the same step as the other's: the joint plan differs from the two
    independent plans, and at no step do its two areas intersect."""
    oracle = _oracle()
    options = centralized_options(Config(scenario_type=ScenarioType.circle, amount=2, Hp=5, mpa_type=MpaType.single_speed))
    mpa = centralized_mpa(options)
    iters = crossing_problem(options, mpa)
    alone = [info_from_record(r, options.Hp) for r in jr.plan_joint(options, mpa, [[it] for it in iters])]
    assert any(oracle.intersect_sat(alone[0].shapes[k], alone[1].shapes[k]) for k in range(options.Hp)), "the independent plans must collide"
    joint = jr.plan_joint(options, mpa, [iters])
    assert (joint["status"] == abi.OK).all()
    infos = [info_from_record(r, options.Hp) for r in joint]
    assert any(not np.array_equal(infos[v].predicted_trims, alone[v].predicted_trims) for v in range(2))
    for k in range(options.Hp):
        assert not oracle.intersect_sat(infos[0].shapes[k], infos[1].shapes[k]), "step %d" % (k + 1)
    # the joint cost is at least the sum of the independent ones (the joint tree holds every pair of independent paths)
    assert joint["path_nodes"][0][options.Hp][4] >= alone[0].tree.g[-1] + alone[1].tree.g[-1]


def test_centralized_controller_runs_on_the_reference():
    """The systemtest configuration (Config_systemtests_centralized.json: 2 vehicles, single_speed) on the circle scenario, a few
    steps planned by the CPU reference: no exception, both vehicles move, no two areas of a plan intersect."""
    oracle = _oracle()
    options = Config(scenario_type=ScenarioType.circle, amount=2, Hp=5, mpa_type=MpaType.single_speed, T_end=4)
    mpa = centralized_mpa(options)

    def plan(iters):
        return [info_from_record(r, options.Hp) for r in jr.plan_joint(centralized_options(options), mpa, [iters])]

    ctl = CentralizedController(options, circle_scenario(options), mpa, plan)
    assert not ctl.options.is_prioritized and not ctl.options.are_any_obstacles_non_convex
    start = [(m.x, m.y) for m in ctl.meas]
    for _ in range(4):
        infos = ctl.step()
        for k in range(options.Hp):
            assert not oracle.intersect_sat(infos[0].shapes[k], infos[1].shapes[k])
    for (x0, y0), m in zip(start, ctl.meas):
        assert math.hypot(m.x - x0, m.y - y0) > 0.1


def test_centralized_controller_raises_on_exhaustion():
    options = Config(scenario_type=ScenarioType.circle, amount=2, Hp=5, mpa_type=MpaType.single_speed)
    mpa = centralized_mpa(options)

    def plan(iters):
        rec = np.zeros(len(iters), dtype=abi.VEHICLE_OUT_DTYPE)
        rec["status"] = abi.EXHAUSTED
        return [info_from_record(r, options.Hp) for r in rec]

    ctl = CentralizedController(options, circle_scenario(options), mpa, plan)
    with pytest.raises(CentralizedExhaustedError):
        ctl.step()


@pytest.mark.timeout(900)
def test_joint_kernel_uses_no_scratch_memory_and_spills_no_vgprs():
    """The joint kernel (one wavefront per problem) in `make resources`: no scratch, no VGPR spills."""
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and shutil.which("hipcc") is None:
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
    assert "pdmpc_joint_kernel" in seen, sorted(seen)
    assert seen["pdmpc_joint_kernel"] == {"scratch": 0, "vgpr_spill": 0}, seen["pdmpc_joint_kernel"]
