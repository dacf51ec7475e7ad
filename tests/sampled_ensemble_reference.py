"""Expected records of a whole time step planned with the sampled optimizer as a seed ensemble (pdmpc_set_sampled_ensemble;
DESIGN.md §3.18).  TEST INFRASTRUCTURE ONLY.

The level-by-level step of tests/sampled_step_reference.py with, per slot, E runs of the planner and the winner rule of
include/pdmpc.h:

    member e of a slot with seed s plans with mt19937ar((s + e * 1000003) mod 2^32) against the same obstacles, the areas its
    predecessors published (the WINNERS' areas, or fallback areas) among them;
    among the members with status OK the smallest final cost path_nodes[Hp][4] wins, compared as doubles with <, members in
    ascending order: the lowest index wins a tie;
    no member OK: the slot's record is member 0's (exhausted, carrying the slot's fallback areas).

The planner is oracle.plan_batch_sampled at budget 250 and tests/sampled_budget_reference.py's at any other budget."""
import copy

import numpy as np

import sampled_budget_reference as sbr
from oracle import oracle
from pdmpc import abi

STRIDE = 1000003  # PDMPC_SAMPLED_ENSEMBLE_STRIDE
MEMBERS_MAX = 16  # PDMPC_SAMPLED_ENSEMBLE_MAX
MAX_THREADS = 16


def member_seed(seed, e):
    """PDMPC_SAMPLED_MEMBER_SEED(seed, e)."""
    return (int(seed) + int(e) * STRIDE) % (1 << 32)


def planner_for(options, mpa, budget):
    """planner(iters, seeds) -> records, by the restatement that belongs to the budget."""
    if budget == sbr.DEFAULT_BUDGET:
        return lambda iters, seeds: oracle.plan_batch_sampled(options, mpa, iters, seeds, n_threads=max(1, min(MAX_THREADS, len(iters))))[1]
    sm = sbr.SampledMpa(mpa)
    return lambda iters, seeds: sbr.plan_batch_sampled(options, sm, iters, seeds, budget=budget)


def pick(member_records, Hp):
    """The winner rule on one slot's E records -> (winner, costs (E,), any member OK)."""
    costs = np.array([float(r["path_nodes"][Hp][4]) if int(r["status"]) == abi.OK else np.inf for r in member_records])
    winner, have = 0, False
    for e, r in enumerate(member_records):
        if int(r["status"]) == abi.OK and (not have or costs[e] < costs[winner]):
            winner, have = e, True
    return winner, costs, have


def plan_step_ensemble(options, mpa, problem, seeds, n_members, budget=sbr.DEFAULT_BUDGET):
    """-> (records (n,), winners (n,) int32, costs (E, n): +inf where a member is not OK)."""
    Hp, E = options.Hp, int(n_members)
    planner = planner_for(options, mpa, budget)
    n = len(problem["iters"])
    recs = np.zeros(n, dtype=abi.VEHICLE_OUT_DTYPE)
    winners = np.zeros(n, dtype=np.int32)
    costs = np.full((E, n), np.inf)
    first = 0
    for size in problem["level_sizes"]:
        slots = list(range(first, first + size))
        iters = []
        for s in slots:
            it = copy.copy(problem["iters"][s])
            dyn = list(it.dynamic_obstacle_area)
            for p in problem["preds"][s]:
                assert p < first, "slots are not in level order"
                if int(recs[p]["status"]) == 0:
                    dyn.append([np.array(recs[p]["shapes"][k][:, : int(recs[p]["shape_cols"][k])]) for k in range(Hp)])
                else:
                    fb = problem["fallback"][p]
                    if fb is not None and len(fb):
                        dyn.append([np.asarray(a, dtype=np.float64) for a in fb])
            it.dynamic_obstacle_area = dyn
            iters.append(it)
        # all members of the level in one call: member e of the q-th slot is record e * size + q
        out = planner(iters * E, [member_seed(seeds[s], e) for e in range(E) for s in slots])
        for q, s in enumerate(slots):
            members = [out[e * size + q] for e in range(E)]
            winners[s], costs[:, s], have = pick(members, Hp)
            recs[s] = members[winners[s]]
            if not have:
                fb = problem["fallback"][s]
                if fb is not None and len(fb):
                    for k in range(Hp):
                        a = np.asarray(fb[k], dtype=np.float64)
                        recs[s]["shape_cols"][k] = a.shape[1]
                        recs[s]["shapes"][k][:, : a.shape[1]] = a
        first += size
    return recs, winners, costs
