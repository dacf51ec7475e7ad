"""Seed ensembles of the sampled optimizer (pdmpc_set_sampled_ensemble): what E members per vehicle cost and buy.

Workload: recorded closed-loop steps of the C2-like road network (20 vehicles, Hp 8, distance coupling, seed 1; the loop that records
them plans with one member), planned with the sampled optimizer at budget 250 by pdmpc_plan_step_sampled.

  timing   the step's device time -- the kernel time between HIP events on the launch stream, pdmpc_stats.kernel_ms -- for
           E in 1, 2, 4, 8, 16: per recorded step the median of LAUNCHES launches after a warm-up, E = 1 and E alternated launch by
           launch in the same run; the table gives the mean of the steps' medians.  "E = 1 against itself" runs the same alternation
           with E = 1 on both sides: the spread a difference has to exceed.
  quality  the mean final cost (path_nodes[Hp][4]) over the vehicles every planner solved, relative to E = 1 and relative to the graph
           search's optimal cost of the same step problems (pdmpc_plan_step: each vehicle's optimum against ITS predecessors' optimal
           plans, so a ratio below 1 is possible for a vehicle whose predecessors chose differently).

    python tools/sampled_ensemble_timing.py [--quick]          (profiles/sampled_ensemble_timing.txt is its output)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np

from pdmpc.backend import Handle
from pdmpc.config import Config, ScenarioType
from pdmpc.mpa import get_mpa
from pdmpc.road_network import commonroad_scenario
from sampled_step_timing import record_steps

QUICK = "--quick" in sys.argv
LAUNCHES = 4 if QUICK else 20
WARM = 1 if QUICK else 3
SIZES = [1, 2, 4, 8, 16]


def main():
    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32, max_nodes=1 << 15)
    Hp = options.Hp
    sc = commonroad_scenario(options, seed=1)
    mpa = get_mpa(options)
    steps = record_steps(options, mpa, sc, 3 if QUICK else 8)
    levels = [len(p["level_sizes"]) for p, _ in steps]
    h = Handle(options)
    h.upload_mpa(mpa)

    def launch(prob, seeds, E):
        h.set_sampled_ensemble(E)
        recs = h.plan_step_sampled(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]], seeds)
        st = h.stats()
        assert st["safe_replans"] == 0
        return recs, st

    info, recs_of = {}, {}
    base_ms, ens_ms = {E: [] for E in SIZES}, {E: [] for E in SIZES}
    for E in SIZES:  # (E == 1: E = 1 against itself)
        for i, (prob, seeds) in enumerate(steps):
            a, b = [], []
            for k in range(WARM + LAUNCHES):
                _, st1 = launch(prob, seeds, 1)
                recs, stE = launch(prob, seeds, E)
                if k >= WARM:
                    a.append(st1["kernel_ms"])
                    b.append(stE["kernel_ms"])
            base_ms[E].append(float(np.median(a)))
            ens_ms[E].append(float(np.median(b)))
            recs_of[(E, i)] = recs.copy()
            info[E] = (h.last_sampled_kernel(), stE["lds_bytes"])
    h.close()

    g = Handle(options)
    g.upload_mpa(mpa)
    optimal = [g.plan_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]]).copy() for prob, _ in steps]
    g.close()

    print("C2-like: 20 vehicles, Hp 8, %d recorded steps of %d-%d computation levels, budget 250; per step the median of %d launches after %d warm-up launches," % (len(steps), min(levels), max(levels), LAUNCHES, WARM))
    print("E = 1 and E alternated launch by launch; kernel time between HIP events, mean over the steps (min .. max of the steps' medians)")
    for E in SIZES:
        ratio = np.array(ens_ms[E]) / np.array(base_ms[E])
        print("  E %2d  %-30s LDS %6d B  grid %4d  step %8.3f ms (%.3f .. %.3f)   E = 1 next to it %8.3f ms   ratio of medians per step: mean %.3f (%.3f .. %.3f)%s"
              % (E, info[E][0], info[E][1], 20 * E, float(np.mean(ens_ms[E])), min(ens_ms[E]), max(ens_ms[E]), float(np.mean(base_ms[E])), float(ratio.mean()), ratio.min(), ratio.max(),
                 "   <- E = 1 against itself" if E == 1 else ""))
    solved = [np.all([recs_of[(E, i)]["status"] == 0 for E in SIZES] + [optimal[i]["status"] == 0], axis=0) for i in range(len(steps))]
    n_solved = int(sum(int(m.sum()) for m in solved))

    def mean_cost(get):
        return float(sum(float(get(i)["path_nodes"][:, Hp, 4][solved[i]].sum()) for i in range(len(steps))) / max(n_solved, 1))

    opt = mean_cost(lambda i: optimal[i])
    one = mean_cost(lambda i: recs_of[(1, i)])
    print("quality: mean final cost over the %d of %d vehicle plans that every planner solved; graph search (optimal) %.6f" % (n_solved, 20 * len(steps), opt))
    for E in SIZES:
        c = mean_cost(lambda i: recs_of[(E, i)])
        unsolved = int(sum(int((recs_of[(E, i)]["status"] != 0).sum()) for i in range(len(steps))))
        print("  E %2d  mean cost %.6f   relative to E = 1 %.4f   relative to the graph search %.4f   exhausted plans %d" % (E, c, c / one, c / opt, unsolved))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
