"""The step problems of the seed-ensemble tests (tests/test_sampled_ensemble_host.py, tests/test_gpu_sampled_ensemble.py): the smallest
steps at which the ensemble's protocol can go wrong, and their expected records by the twin (sampled_ensemble_reference.py), computed
once per (case, E, budget).  TEST INFRASTRUCTURE ONLY."""
import copy

import numpy as np

import sampled_ensemble_reference as ser
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.mpa import get_mpa

CIRCLE_STEP, ROAD_STEP, ROAD_SEED = 2, 2, 1  # (chosen so that a slot with successors has a winner other than member 0: see has_handed_over_winner)


def circle_case(time_step=CIRCLE_STEP):
    """Case A: the circle scenario, 4 vehicles fully coupled -- a chain of 4 levels --, Hp 4, separating-axis checks."""
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=4, max_vehicles=8)
    mpa = get_mpa(options)
    ctl = PrioritizedSequentialController(options, circle_scenario(options), mpa, None, coupling="full")
    ctl.k = time_step
    prob = ctl.build_step_problem()
    return options, mpa, prob, [int(ctl.k) + int(v) + 1 for v in prob["order"]]


def road_case(time_step=ROAD_STEP, seed=ROAD_SEED):
    """Case B: a road-network step of 5 vehicles fully coupled (5 levels), Hp 5, InterX checks."""
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=5, Hp=5, max_vehicles=8)
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=seed)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="full", boundary_provider=boundary_provider(sc))
    ctl.k = time_step
    prob = ctl.build_step_problem()
    return options, mpa, prob, [int(ctl.k) + int(v) + 1 for v in prob["order"]]


CASES = {"circle": circle_case, "road": road_case}
_case_cache, _twin_cache = {}, {}


def case(name):
    if name not in _case_cache:
        _case_cache[name] = CASES[name]()
    return _case_cache[name]


def twin(name, n_members, budget):
    """(records, winners, costs) of a case by the twin; shared among the tests and never changed."""
    key = (name, n_members, budget)
    if key not in _twin_cache:
        options, mpa, prob, seeds = case(name)
        _twin_cache[key] = ser.plan_step_ensemble(options, mpa, prob, seeds, n_members, budget)
    return _twin_cache[key]


def has_successors(prob):
    """slot -> whether any slot plans against it."""
    pred_of_any = set(p for ps in prob["preds"] for p in ps)
    return [s in pred_of_any for s in range(len(prob["iters"]))]


def has_handed_over_winner(prob, records, winners):
    """The tests' condition: a slot WITH successors was solved by a member other than 0, so its areas -- a member's other than the
    reference stream's -- are what a successor planned against."""
    succ = has_successors(prob)
    return any(succ[s] and int(winners[s]) != 0 and int(records[s]["status"]) == 0 for s in range(len(winners)))


def fallback_args(prob):
    return [f if f is not None else [] for f in prob["fallback"]]


def boxed_in(iter_v, half=0.8):
    """A copy of a vehicle's problem with a square obstacle around its start pose: every first edge collides."""
    it = copy.copy(iter_v)
    x, y = float(it.x0[0]), float(it.x0[1])
    box = np.array([[x - half, x + half, x + half, x - half, x - half], [y - half, y - half, y + half, y + half, y - half]])
    it.obstacles = list(it.obstacles) + [box]
    return it
