"""The sampled optimizer's host side (csrc/sampled_launch.hpp) next to the graph search's on one handle: banks
of both kinds and of every sampled kernel resident side by side, launched in turn on the scratch they share, and the sliced launch
loop of the budget and the ensemble launchers."""
import copy

import numpy as np
import pytest

import problems
from pdmpc.backend import Handle
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.mpa import get_mpa
from pdmpc.scenario import circle_scenario

pytestmark = pytest.mark.gpu

SEARCH, SAMPLED = 2, 3  # stats()["kernel"]


def circle_chain():
    """The circle scenario, 4 vehicles, full coupling, Hp 5: a chain of three predecessors, so the wait and the hand-over run."""
    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8)
    mpa = get_mpa(options)
    ctl = PrioritizedSequentialController(options, circle_scenario(options), mpa, None, coupling="full")
    ctl.k = 2
    prob = ctl.build_step_problem()
    assert [len(p) for p in prob["preds"]] == [0, 1, 2, 3]
    return options, mpa, prob, [int(ctl.k) + int(v) + 1 for v in prob["order"]]


def new_handle(options, mpa):
    h = Handle(options)
    h.upload_mpa(mpa)
    return h


def pack_bank(h, prob, seeds, budget, members):
    """The step into the current bank: the graph search's (budget None), or the sampled optimizer's at (budget, members)."""
    if budget is not None:
        h.set_sampled_budget(budget)
        h.set_sampled_ensemble(members)
        h.set_step_seeds(seeds)
    h.pack_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])


def smallest_budget_in_hbm(h):
    """... of the current (sampled) bank's plan, read from the window."""
    lo, hi = 251, 16384
    assert h.sampled_plan_bank(lo)[1]["tree_in_lds"] == 1 and h.sampled_plan_bank(hi)[1]["tree_in_lds"] == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if h.sampled_plan_bank(mid)[1]["tree_in_lds"]:
            lo = mid
        else:
            hi = mid
    return hi


def test_five_resident_banks_on_one_handle():
    options, mpa, prob, seeds = circle_chain()
    n = len(seeds)
    h = new_handle(options, mpa)
    try:
        h.select_bank(1)
        pack_bank(h, prob, seeds, 250, 1)
        hbm = smallest_budget_in_hbm(h)
        banks = [(None, 1), (250, 1), (251, 1), (hbm, 1), (250, 2)]  # (budget, members)
        want, kernel = [], []
        for budget, members in banks:
            alone = new_handle(options, mpa)
            try:
                pack_bank(alone, prob, seeds, budget, members)
                alone.launch()
                want.append(np.ascontiguousarray(alone.fetch(n)).tobytes())
                kernel.append(None if budget is None else alone.sampled_plan_bank(budget)[0]["kernel"])
            finally:
                alone.close()
        assert kernel == [None, "pdmpc_sampled_kernel", "pdmpc_sampled_budget_kernel", "pdmpc_sampled_budget_kernel_hbm", "pdmpc_sampled_ensemble_kernel"]
        assert len(set(want)) == 5, "two banks plan the same records: launching the wrong one would go unseen"
        for b, (budget, members) in enumerate(banks):
            h.select_bank(b)
            pack_bank(h, prob, seeds, budget, members)
        last = ""
        for b in (0, 1, 2, 3, 4, 4, 3, 2, 1, 0):
            h.select_bank(b)
            h.launch()
            got = np.ascontiguousarray(h.fetch(n)).tobytes()
            assert got == want[b], "bank %d" % b
            if kernel[b] is not None:
                last = kernel[b]
            assert h.last_sampled_kernel() == last, "bank %d" % b
            st = h.stats()
            assert st["kernel"] == (SEARCH if kernel[b] is None else SAMPLED) and st["safe_replans"] == 0, "bank %d" % b
    finally:
        h.close()


@pytest.mark.parametrize("budget,members,kernel", [(251, 1, "pdmpc_sampled_budget_kernel"), (250, 2, "pdmpc_sampled_ensemble_kernel")])
def test_resident_slices_of_the_budget_and_the_ensemble_launchers(budget, members, kernel):
    """An uncoupled batch of 2 x CU count + 3 vehicles with safe launches on: more slots than any resident slice holds, so the launch
    goes out in slices (three of them for the ensemble, whose slices count slots with all their members)."""
    import torch

    options, mpa, base = problems.problem_set("interx", 33, 8, Hp=5)
    n = 2 * torch.cuda.get_device_properties(options.device).multi_processor_count + 3
    iters = [base[i % len(base)] for i in range(n)]
    seeds = [7 + i for i in range(n)]
    opt = copy.copy(options)
    opt.max_vehicles = n
    opt.max_nodes = 1 << 10
    h = new_handle(opt, mpa)
    try:
        h.set_sampled_budget(budget)
        h.set_sampled_ensemble(members)
        whole = np.ascontiguousarray(h.plan_batch_sampled(iters, seeds)).tobytes()
        assert h.last_sampled_kernel() == kernel and h.sampled_plan_bank(budget)[0]["slice"] == n
        h.set_safe_launch(True)
        sliced = np.ascontiguousarray(h.plan_batch_sampled(iters, seeds)).tobytes()
        assert h.last_sampled_kernel() == kernel and 0 < h.sampled_plan_bank(budget)[0]["slice"] < n
        st = h.stats()
        assert st["kernel"] == SAMPLED and st["n_launches"] == 1 and st["safe_replans"] == 0
        assert sliced == whole
        assert len({whole[i * len(whole) // n : (i + 1) * len(whole) // n] for i in range(8)}) > 1, "every slot plans the same record"
    finally:
        h.close()
