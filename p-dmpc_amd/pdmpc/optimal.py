"""Optimal-priority control: every unique prioritization of the coupling graph in one batch.

Restates the host side of the reference's optimal-priority controller
(hlc/controller/prioritized/PrioritizedOptimalController.m, PrioritizedOptimalSequentialController.m):

    unique_priorities        Prioritizer.m:97-140    the acyclic orientations of the coupling graph's edges, one priority
                                                     vector per orientation
    one plan per orientation :25-53, controller      prepare_permutation: constant priorities = the orientation's priorities,
                                                     then prioritize() and group()
    compute_solution_cost    :56-71                  per vehicle and orientation the cost-to-come of the final node
    receive_solution_cost    :82-100                 a vehicle adds the costs of ALL other vehicles to its own (ascending index)
    choose_solution          :102-114                round(., 8), the first minimum, per vehicle

The reference plans the orientations one after the other.  Here all K instances are flattened into ONE batch exactly as the
explorative step flattens its permutations (pdmpc.explorative.flatten_instances): slots ordered by (level, instance, slot).
The native twin is pdmpc_controller_optimal_* (csrc/step_controller.cpp, csrc/step_batch.hpp); the enumeration runs on the device there
(pdmpc_unique_priorities, csrc/priority_kernel.hip).
"""
import heapq

import numpy as np

from .explorative import flatten_instances


class TooManyPrioritizations(RuntimeError):
    pass


def _stable_toposort(d):
    """toposort(digraph(d), 'Order', 'stable'): the lexicographically smallest topological order (0-based), None for a cycle."""
    n = d.shape[0]
    indeg = d.sum(axis=0).astype(np.int64)
    ready = [v for v in range(n) if indeg[v] == 0]
    heapq.heapify(ready)
    order = []
    while ready:
        v = heapq.heappop(ready)
        order.append(v)
        for w in np.flatnonzero(d[v]):
            indeg[w] -= 1
            if indeg[w] == 0:
                heapq.heappush(ready, int(w))
    return order if len(order) == n else None


def unique_priorities(adjacency):
    """Prioritizer.unique_priorities (Prioritizer.m:97-140) -> (result n x K as in MATLAB, masks [K]).  Column k holds the priorities
    of the k-th acyclic orientation in ascending order of its mask m = i_permutation - 1; m flips edge e (0-based) of
    find(triu(adjacency, 1)) exactly when bit E - 1 - e is set (dec2bin(m, E)).  MATLAB's default toposort order is not documented;
    this takes the lexicographically smallest one ('Order', 'stable'), which fixes the priorities.  The plans depend on the
    orientation only: directed_coupling_from_priorities gives back the orientation for any of its topological orders."""
    A = np.asarray(adjacency)
    n = A.shape[0]
    edge_row, edge_col = [], []
    for c in range(n):  # find(triu(adjacency, 1)): column-major
        for r in range(c):
            if A[r, c] != 0:
                edge_row.append(r)
                edge_col.append(c)
    n_edges = len(edge_row)
    result, masks = [], []
    for i_permutation in range(1, 2 ** n_edges + 1):
        m = i_permutation - 1
        flips = [(m >> (n_edges - 1 - e)) & 1 == 1 for e in range(n_edges)]  # dec2bin(i_permutation - 1, n_edges) == '1'
        directed = np.zeros((n, n), dtype=np.int64)
        for e in range(n_edges):
            if flips[e]:
                directed[edge_col[e], edge_row[e]] = 1
            else:
                directed[edge_row[e], edge_col[e]] = 1
        order = _stable_toposort(directed)
        if order is None:  # isdag
            continue
        priority = np.zeros(n, dtype=np.int64)
        priority[order] = np.arange(1, n + 1)  # priority(topological_order) = 1:n_vehicles
        result.append(priority)
        masks.append(m)
    return np.array(result, dtype=np.int64).reshape(-1, n).T, np.array(masks, dtype=np.int64)


def build_optimal_batch(ctl, max_instances):
    """One flattened step problem holding every unique prioritization of the controller's current traffic state (the twin of
    pdmpc_controller_optimal_build).  Instance p plans with constant priorities = column p of unique_priorities, grouped as the
    controller groups.  Raises TooManyPrioritizations for more than max_instances of them."""
    ctl.build_step_problem()  # refreshes the traffic state and the adjacency
    priorities, masks = unique_priorities(ctl.last_adjacency)
    K = priorities.shape[1]
    if K > max_instances:
        raise TooManyPrioritizations("%d unique prioritizations, max_instances is %d" % (K, max_instances))
    parts = [ctl.build_step_problem(priorities=list(priorities[:, p]), refresh=False) for p in range(K)]
    out = flatten_instances(parts)
    out["n_instances"] = K
    out["masks"] = masks
    out["priorities"] = priorities
    out["adjacency"] = np.array(ctl.last_adjacency)
    return out


def choose_solution(batch, records, Hp):
    """PrioritizedOptimalController.m:56-114 for every vehicle v: per instance the sum of the final nodes' cost-to-come of ALL
    vehicles, v's own first and then the others in ascending index (receive_solution_cost), round(., 8), the first minimum.  An
    exhausted search makes its instance infinitely expensive (the explorative step's rule).
    Returns (chosen instance per vehicle, cost table n x K)."""
    K = batch["n_instances"]
    n = len(batch["vehicle"]) // K
    val = np.zeros((K, n))
    for slot, (p, v) in enumerate(zip(batch["instance"], batch["vehicle"])):
        rec = records[slot]
        val[p, v] = float(rec["path_nodes"][Hp][4]) if int(rec["status"]) == 0 else np.inf
    return choose_from_costs(val)


def choose_from_costs(val):
    """The choice on a table val[p, v] = solution cost of vehicle v in instance p -> (chosen per vehicle, cost table n x K)."""
    K, n = val.shape
    cost = np.zeros((n, K))
    for v in range(n):
        s = val[:, v].copy()  # compute_solution_cost: the vehicle's own costs
        for j in range(n):
            if j != v:
                s = s + val[:, j]  # receive_solution_cost: solution_cost + latest_msg_j.solution_cost
        cost[v] = np.round(s, 8)
    return [int(np.argmin(cost[v])) for v in range(n)], cost


def optimal_step(ctl, plan_batch, max_instances):
    """One optimal-priority time step of the Python controller (twin of pdmpc_controller_optimal_step): every unique prioritization
    as one batch, `plan_batch(batch)` -> records in slot order, the choice per vehicle, and every vehicle goes on with the plan and
    the couplings of its choice (obj.info / obj.iter = ..._array_tmp{chosen_solution}, :100-101).
    Returns (batch, records, chosen instance per vehicle)."""
    from .iteration_data import info_from_record

    Hp = ctl.options.Hp
    kept = {}

    def plan_step(prob):
        batch = build_optimal_batch(ctl, max_instances)
        records = plan_batch(batch)
        chosen, _ = choose_solution(batch, records, Hp)
        slot = {(p, v): s for s, (p, v) in enumerate(zip(batch["instance"], batch["vehicle"]))}
        seq = np.zeros_like(batch["directed_seq"][0])
        for v in range(ctl.n):
            seq[v, :] = batch["directed_seq"][chosen[v]][v, :]
        ctl.last_directed_seq = seq
        kept.update(batch=batch, records=records, chosen=chosen)
        return [info_from_record(records[slot[(chosen[v], v)]], Hp) for v in prob["order"]]

    ctl.step(plan_step=plan_step)
    return kept["batch"], kept["records"], kept["chosen"]
