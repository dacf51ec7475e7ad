"""The sampled optimizer with a configurable expansion budget (pdmpc_set_sampled_budget, csrc/sampled_budget_kernel.hip; DESIGN.md
§3.18) on the GPU: records byte for byte against the restatement with the budget as a parameter (sampled_budget_reference.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

import problems
import sampled_budget_reference as sbr
from pdmpc import abi
from pdmpc.backend import BackendError, Handle
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.mpa import get_mpa
from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu

NEW_KERNEL, NEW_KERNEL_HBM, OLD_KERNEL = "pdmpc_sampled_budget_kernel", "pdmpc_sampled_budget_kernel_hbm", "pdmpc_sampled_kernel"


def handle_for(options, mpa, budget=None, max_vehicles=16):
    opt = copy.copy(options)
    opt.max_vehicles = max_vehicles
    h = Handle(opt)
    h.upload_mpa(mpa)
    if budget is not None:
        h.set_sampled_budget(budget)
    return h


@pytest.fixture(scope="module")
def batch():
    """8 vehicles of problems.problem_set per checker with their seeds, and the reference records per budget (computed once)."""
    out = {}
    for mode in ("interx", "sat"):
        options, mpa, iters = problems.problem_set(mode, 21, 8, Hp=6, n_hdv=1 if mode == "interx" else 0)
        out[mode] = {"options": options, "mpa": mpa, "sm": sbr.SampledMpa(mpa), "iters": iters, "seeds": [2 + i for i in range(8)], "ref": {}}
    return out


def reference(b, budget):
    if budget not in b["ref"]:
        b["ref"][budget] = sbr.plan_batch_sampled(b["options"], b["sm"], b["iters"], b["seeds"], budget=budget)
    return b["ref"][budget]


@pytest.mark.parametrize("budget", [1, 7, 249, 251, 1000])
@pytest.mark.parametrize("mode", ["interx", "sat"])
def test_budgets_around_the_default_and_beyond(batch, mode, budget):
    b = batch[mode]
    h = handle_for(b["options"], b["mpa"], budget)
    assert h.sampled_budget() == budget
    got = h.plan_batch_sampled(b["iters"], b["seeds"])
    assert h.last_sampled_kernel() == NEW_KERNEL
    st = h.stats()
    assert st["kernel"] == 3 and st["n_launches"] == 1
    h.close()
    want = reference(b, budget)
    assert_records_equal(got, want, "%s budget %d" % (mode, budget))
    assert np.all(want["n_expanded"] <= budget + b["options"].Hp - 1)
    if budget >= 249:
        assert (want["status"] == 0).any()


@pytest.mark.parametrize("mode", ["interx", "sat"])
def test_default_budget_through_the_setter_is_the_default_call(batch, mode):
    b = batch[mode]
    h = handle_for(b["options"], b["mpa"])
    assert h.sampled_budget() == 250 and h.last_sampled_kernel() == ""
    plain = h.plan_batch_sampled(b["iters"], b["seeds"])
    assert h.last_sampled_kernel() == OLD_KERNEL
    h.set_sampled_budget(64)
    other = h.plan_batch_sampled(b["iters"], b["seeds"])
    assert h.last_sampled_kernel() == NEW_KERNEL
    h.set_sampled_budget(250)
    again = h.plan_batch_sampled(b["iters"], b["seeds"])
    assert h.last_sampled_kernel() == OLD_KERNEL
    assert again.tobytes() == plain.tobytes() and other.tobytes() != plain.tobytes()
    assert_records_equal(plain, reference(b, 250), "%s default budget" % mode)
    # the range of the setter, with a live handle: a refused value leaves the budget as it was
    for bad in (0, -5, 16385):
        with pytest.raises(BackendError):
            h.set_sampled_budget(bad)
    assert h.sampled_budget() == 250
    assert h.L.pdmpc_get_sampled_budget(h.h, None) == -1
    for ok in (1, 16384):
        h.set_sampled_budget(ok)
        assert h.sampled_budget() == ok
    h.close()


@pytest.mark.parametrize("mode", ["interx", "sat"])
def test_the_edge_between_the_tree_in_lds_and_in_hbm(batch, mode):
    """The largest budget whose tree the plan of THIS bank keeps in LDS, and the next one: read from the window."""
    b = batch[mode]
    h = handle_for(b["options"], b["mpa"], 7)
    h.plan_batch_sampled(b["iters"], b["seeds"])  # (packs the bank the window then plans for)
    lo, hi = 7, 16384
    assert h.sampled_plan_bank(lo)[1]["tree_in_lds"] == 1 and h.sampled_plan_bank(hi)[1]["tree_in_lds"] == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if h.sampled_plan_bank(mid)[1]["tree_in_lds"]:
            lo = mid
        else:
            hi = mid
    for budget, in_lds in ((lo, 1), (hi, 0)):
        plan, extra = h.sampled_plan_bank(budget)
        assert extra["tree_in_lds"] == in_lds and plan["kernel"] == (NEW_KERNEL if in_lds else NEW_KERNEL_HBM)
        h.set_sampled_budget(budget)
        got = h.plan_batch_sampled(b["iters"], b["seeds"])
        assert h.last_sampled_kernel() == plan["kernel"]
        assert h.stats()["lds_bytes"] == plan["total"]
        assert_records_equal(got, reference(b, budget), "%s budget %d (tree %s)" % (mode, budget, "in LDS" if in_lds else "in HBM"))
    h.close()


@pytest.fixture(scope="module")
def free_road():
    options = problems.make_options("interx", Hp=8)
    mpa = get_mpa(options)
    rng = np.random.default_rng(4)
    iters = [problems.road_problem(rng, options, mpa, n_dyn=0, n_static=0, with_boundary=False) for _ in range(2)]
    return options, mpa, sbr.SampledMpa(mpa), iters, [5, 6]


@pytest.mark.parametrize("budget", [4096, 16384])
def test_the_budget_ends_the_search_on_a_free_road(free_road, budget):
    """Nothing cuts the tree, so the budget ends the search and the tree fills (in HBM at the limit): node ids up to budget + Hp - 1."""
    options, mpa, sm, iters, seeds = free_road
    want = sbr.plan_batch_sampled(options, sm, iters, seeds, budget=budget)
    assert np.all(want["n_expanded"] >= budget) and np.all(want["status"] == 0)
    h = handle_for(options, mpa, budget, max_vehicles=4)
    got = h.plan_batch_sampled(iters, seeds)
    plan, extra = h.sampled_plan_bank(budget)
    assert h.last_sampled_kernel() == plan["kernel"]
    if budget == 16384:  # (590 KB: no layout holds it; 4 096 nodes of a free road's small soup still fit the 160 KB layout)
        assert plan["kernel"] == NEW_KERNEL_HBM and extra["tree_hbm_bytes"] >= (1 + budget + options.Hp) * 36
    # a second launch of the resident bank finds the trees of the first in HBM: nothing is cleared, nothing of them is read
    h.launch()
    again = h.fetch(len(iters))
    h.close()
    assert_records_equal(got, want, "free road, budget %d" % budget)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("mode", ["interx", "sat"])
def test_the_default_kernel_at_the_longest_horizon(mode):
    """pdmpc_sampled_kernel at Hp = PDMPC_HP_MAX = 16 and its own budget of 250, on a free road: its stream drawn ahead is at its longest
    (4 000 doubles: 13 twists, with the tree's region as the generator's state) and its tree at its tallest (a descent adds up to 16
    rows; up to 265 of the 288).  Two vehicles, the second 0.3 m beside the first and coupled to it, so the first's areas cut some of
    its edges: records and tree sizes byte for byte."""
    options = problems.make_options(mode, Hp=16)
    mpa = get_mpa(options)
    rng = np.random.default_rng(9)
    iters = [problems.road_problem(rng, options, mpa, n_dyn=0, n_static=0, with_boundary=False, convex=(mode == "sat")) for _ in range(2)]
    beside = copy.copy(iters[1])
    beside.x0 = np.array(beside.x0, dtype=np.float64) + np.array([0.0, 0.3, 0.0, 0.0])
    beside.reference_trajectory_points = np.array(beside.reference_trajectory_points, dtype=np.float64) + np.array([0.0, 0.3])
    iters[1] = beside
    prob = {"iters": iters, "preds": [[], [0]], "fallback": [None, None], "level_sizes": [1, 1]}
    seeds, sm, sizes = [11, 12], sbr.SampledMpa(mpa), []
    want = sbr.plan_step_sampled(options, mpa, prob, seeds, lambda its, sd: sbr.plan_batch_sampled(options, sm, its, sd, budget=250, tree_sizes=sizes))
    assert np.all(want["n_expanded"] >= 250) and np.all(want["status"] == 0) and sizes[0] == 1 + int(want["n_expanded"][0])
    assert want[1].tobytes() != sbr.plan_batch_sampled(options, sm, [beside], seeds[1:], budget=250)[0].tobytes(), "the hand-over changes nothing"
    h = handle_for(options, mpa, max_vehicles=4)
    got = plan_step_gpu(h, prob, seeds)
    assert h.last_sampled_kernel() == OLD_KERNEL
    st = h.stats()
    assert st["kernel"] == 3 and st["n_launches"] == 1 and st["safe_replans"] == 0
    got_sizes = []
    for v in range(2):
        n = C.c_int32(-1)
        assert h.L.pdmpc_debug_tree(h.h, v, 0, None, None, None, None, None, None, None, None, C.byref(n)) == 0
        got_sizes.append(n.value)
    h.close()
    assert_records_equal(got, want, "%s, Hp 16, default budget" % mode)
    assert got_sizes == sizes


def boxed_in_problem():
    """tests/test_gpu_sampled_step.py's: slot 0 is boxed in by an obstacle, its fallback areas lie across slot 1's way."""
    from pdmpc.reference_trajectory import get_occupied_areas
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=6, Hp=6, max_vehicles=8)
    mpa = get_mpa(options)
    sc = circle_scenario(options)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="full")
    ctl.k = 3
    prob = ctl.build_step_problem()
    it0 = copy.copy(prob["iters"][0])
    x, y = float(it0.x0[0]), float(it0.x0[1])
    box = np.array([[x - 0.8, x + 0.8, x + 0.8, x - 0.8, x - 0.8], [y - 0.8, y - 0.8, y + 0.8, y + 0.8, y - 0.8]])
    it0.obstacles = list(it0.obstacles) + [box]
    prob["iters"][0] = it0
    veh = sc.vehicles[0]
    x1, y1, yaw1 = (float(v) for v in prob["iters"][1].x0[:3])
    _, rect = get_occupied_areas(x1 + veh.Length * np.cos(yaw1), y1 + veh.Length * np.sin(yaw1), yaw1, veh.Length, 2 * veh.Width, options.offset)
    prob["fallback"][0] = [np.asarray(rect, dtype=np.float64) for _ in range(options.Hp)]
    return options, mpa, prob, [int(ctl.k) + int(v) + 1 for v in prob["order"]], rect


def step_reference(options, mpa, prob, seeds, budget):
    sm = sbr.SampledMpa(mpa)
    return sbr.plan_step_sampled(options, mpa, prob, seeds, lambda iters, sd: sbr.plan_batch_sampled(options, sm, iters, sd, budget=budget))


def plan_step_gpu(h, prob, seeds):
    return h.plan_step_sampled(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]], seeds)


@pytest.mark.parametrize("budget", [1, 40, 2500])
def test_a_boxed_in_vehicle_is_exhausted_at_every_budget(budget):
    options, mpa, prob, seeds, rect = boxed_in_problem()
    h = handle_for(options, mpa, budget, max_vehicles=8)
    got = plan_step_gpu(h, prob, seeds)
    st = h.stats()
    assert st["kernel"] == 3 and st["n_launches"] == 1 and st["safe_replans"] == 0
    h.close()
    assert_records_equal(got, step_reference(options, mpa, prob, seeds, budget), "boxed in, budget %d" % budget)
    assert int(got[0]["status"]) == 1
    assert list(got[0]["shape_cols"][: options.Hp]) == [rect.shape[1]] * options.Hp  # its successors got its fallback areas


def test_realistic_automaton():
    options, mpa, iters = problems.problem_set("interx", 8, 4, Hp=5, mpa_type=MpaType.realistic)
    seeds = [4, 5, 6, 7]
    h = handle_for(options, mpa, 600)
    got = h.plan_batch_sampled(iters, seeds)
    assert h.last_sampled_kernel().startswith(NEW_KERNEL)
    h.close()
    assert_records_equal(got, sbr.plan_batch_sampled(options, mpa, iters, seeds, budget=600), "realistic automaton")


@pytest.mark.parametrize("n", [1, 311, 312, 313, 624, 10000])
def test_chunked_generator_matches_mt19937ar(n):
    from oracle import oracle

    options = Config(scenario_type=ScenarioType.circle, amount=2, Hp=6, max_vehicles=4)
    h = Handle(options)
    seeds = [0, 1, 4294967295]
    got = h.debug_random_stream(seeds, n)
    assert h.L.pdmpc_debug_random_stream(h.h, 1, None, 4, None) == -1 and h.L.pdmpc_debug_random_stream(h.h, -1, None, 4, None) == -1
    assert h.L.pdmpc_debug_random_stream(h.h, 0, None, 4, None) == 0
    h.close()
    for i, s in enumerate(seeds):
        want = oracle.mt19937_doubles(s if s else 5489, n)  # (Seed = 0 is MATLAB's default seed 5489, mt19937ar.hpp)
        assert np.array_equal(got[i].view(np.uint64), want.view(np.uint64)), (s, n)


def circle_step():
    """The 8-vehicle circle (full coupling, separating-axis checks) at its 10th step, when the vehicles meet in the middle and searches
    run empty (exhaustions, fallback areas): the closed loop is advanced with the restatement at budget 32."""
    from pdmpc.iteration_data import info_from_record
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=8, Hp=6, max_vehicles=8)
    mpa = get_mpa(options)
    ctl = PrioritizedSequentialController(options, circle_scenario(options), mpa, None, coupling="full")
    seen = {}

    def plan_step(prob):
        seeds = [int(ctl.k) + int(v) + 1 for v in prob["order"]]
        seen["prob"], seen["seeds"] = prob, seeds
        recs = step_reference(options, mpa, prob, seeds, 32)
        return [info_from_record(recs[i], options.Hp) for i in range(len(recs))]

    for _ in range(10):
        ctl.step(plan_step=plan_step)
    return options, mpa, seen["prob"], seen["seeds"]


def road_step():
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32)
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=1)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    ctl.k = 1
    prob = ctl.build_step_problem()
    return options, mpa, prob, [int(ctl.k) + int(v) + 1 for v in prob["order"]]


@pytest.mark.parametrize("budget", [32, 600])
@pytest.mark.parametrize("which", ["circle", "road"])
def test_a_whole_step_and_its_resident_path(which, budget):
    """pdmpc_plan_step_sampled at a budget: one launch, the predecessors' areas (or fallback areas) handed over on the device; then the
    resident path: pack once with the seeds, launch twice, pdmpc_fetch_records_at."""
    options, mpa, prob, seeds = circle_step() if which == "circle" else road_step()
    want = step_reference(options, mpa, prob, seeds, budget)
    if which == "circle":
        assert (want["status"] != 0).any() and (want["status"] == 0).any(), "no search ran empty: the fallback hand-over was not exercised"
    assert len(prob["level_sizes"]) > 1
    h = handle_for(options, mpa, budget, max_vehicles=options.max_vehicles)
    got = plan_step_gpu(h, prob, seeds)
    st = h.stats()
    assert st["kernel"] == 3 and st["n_launches"] == 1 and st["safe_replans"] == 0
    assert h.last_sampled_kernel() == NEW_KERNEL
    assert_records_equal(got, want, "%s step, budget %d" % (which, budget))
    # resident: the bank keeps the budget it was packed with, whatever the handle's is afterwards
    n = len(prob["iters"])
    h.set_step_seeds(seeds)
    h.pack_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])
    h.set_sampled_budget(250)
    idx = np.arange(n, dtype=np.int32)
    for _ in range(2):
        h.launch()
        out = abi.out_array(n)
        assert h.L.pdmpc_fetch_records_at(h.h, n, abi.i32p(idx), abi.out_ptr(out)) == 0
        assert h.last_sampled_kernel() == NEW_KERNEL
        assert_records_equal(out[:n], want, "%s resident step, budget %d" % (which, budget))
    h.close()


def test_handle_applies_the_configured_budget():
    """Config.n_expansions_max reaches the handle, and MonteCarloTreeSearchHip plans with it."""
    from pdmpc.optimizer import MonteCarloTreeSearchHip

    options, mpa, prob, seeds = circle_step()
    opt64 = copy.copy(options)
    opt64.n_expansions_max = 64
    o = MonteCarloTreeSearchHip(opt64)
    assert o.handle.sampled_budget() == 64
    got = o.plan_step_records(prob, mpa)
    assert o.handle.last_sampled_kernel() == NEW_KERNEL
    o.handle.close()
    assert_records_equal(got, step_reference(options, mpa, prob, seeds, 64), "configured budget")
    plain = MonteCarloTreeSearchHip(options)
    assert plain.handle.sampled_budget() == 250
    plain.handle.close()
