"""Expected records of a whole time step planned with the sampled optimizer: the oracle's restatement of MonteCarloTreeSearch.m
(oracle.plan_batch_sampled) level by level, with the hand-over of oracle.plan_step (PrioritizedController.m:476-491):

    a predecessor whose status is OK contributes its solved areas (record shapes) as a dynamic obstacle,
    an exhausted predecessor contributes its fallback areas (the problem's `fallback` of its slot), if it has any,
    an exhausted slot's record carries its fallback areas (what the device publishes for its successors).

`problem` is a step problem in slot order (controller.build_step_problem, or a flattened explorative / optimal batch) whose slots are
in level order; seeds[s] = time_step + vehicle_index of slot s (MonteCarloTreeSearch.m:31-32)."""
import copy

import numpy as np

from oracle import oracle, packing

MAX_THREADS = 16


def step_seeds(problem, time_step):
    """time_step + vehicle_index (1-based) of every slot."""
    return [int(time_step) + int(v) + 1 for v in problem["order"]]


def plan_step_sampled(options, mpa, problem, seeds, n_threads=MAX_THREADS):
    Hp = options.Hp
    n = len(problem["iters"])
    recs = packing.out_array(n)
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
        _, out = oracle.plan_batch_sampled(options, mpa, iters, [seeds[s] for s in slots], n_threads=min(n_threads, size))
        for q, s in enumerate(slots):
            recs[s] = out[q]
            if int(out[q]["status"]) != 0:
                fb = problem["fallback"][s]
                if fb is not None and len(fb):
                    for k in range(Hp):
                        a = np.asarray(fb[k], dtype=np.float64)
                        recs[s]["shape_cols"][k] = a.shape[1]
                        recs[s]["shapes"][k][:, : a.shape[1]] = a
        first += size
    return recs
