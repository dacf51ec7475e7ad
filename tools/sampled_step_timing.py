"""The sampled optimizer's whole time step: steps per second of three ways of planning the same recorded steps.

  (i)   level loop: one pdmpc_plan_batch_sampled per computation level, the predecessors' areas handed over on the host
        (what Python's level loop and MonteCarloTreeSearchHip.m per vehicle do, one launch and one round trip per level)
  (ii)  pdmpc_plan_step_sampled: the whole step in one launch, the hand-over on the device
  (iii) the native controller's closed loop with PDMPC_OPTIMIZER_SAMPLED (build + pack + launch + read-back + apply, host-inclusive;
        its own traffic, not the recorded steps)

C2-like: 20 vehicles, Hp 8, distance coupling, road network seed 1.  C4-like: 512 vehicles, Hp 10, colouring priorities, 26 tiles.
Each way is run RUNS times, alternating (i) and (ii); the median and the spread (min .. max) are printed.  Every (ii) step is checked
against (i) byte for byte first.  --quick: one short run per way (for a profiler run).

--budget B[,B...]: instead, the launch (kernel) time of the C2-like recorded steps at each expansion budget (pdmpc_set_sampled_budget):
medians of RUNS alternating runs over the budgets, the kernel and its LDS, and the time of one launch of the step's vehicles as
independent searches (no predecessors: the time of the slowest single search).  profiles/sampled_budget_timing.txt is its output.

    python tools/sampled_step_timing.py [--quick] [--budget 64,250,251,1000,4096,16384]
"""
import copy
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd"), os.path.join(ROOT, "tests")]

import numpy as np

from pdmpc import abi
from pdmpc.backend import Handle
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController
from pdmpc.optimizer import MonteCarloTreeSearchHip
from pdmpc.road_network import boundary_provider, commonroad_scenario

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 5


def level_loop(h, prob, seeds, Hp):
    """(i): every computation level one pdmpc_plan_batch_sampled; a predecessor's solved areas (or its fallback if it was exhausted)
    become dynamic obstacles on the host; an exhausted slot's record carries its fallback areas."""
    n = len(prob["iters"])
    recs = abi.out_array(n)
    first = 0
    for size in prob["level_sizes"]:
        slots = range(first, first + size)
        iters = []
        for s in slots:
            it = copy.copy(prob["iters"][s])
            dyn = list(it.dynamic_obstacle_area)
            for p in prob["preds"][s]:
                if int(recs[p]["status"]) == 0:
                    dyn.append([recs[p]["shapes"][k][:, : int(recs[p]["shape_cols"][k])] for k in range(Hp)])
                elif prob["fallback"][p] is not None and len(prob["fallback"][p]):
                    dyn.append(list(prob["fallback"][p]))
            it.dynamic_obstacle_area = dyn
            iters.append(it)
        out = h.plan_batch_sampled(iters, [seeds[s] for s in slots])
        for q, s in enumerate(slots):
            recs[s] = out[q]
            fb = prob["fallback"][s]
            if int(out[q]["status"]) != 0 and fb is not None and len(fb):
                for k in range(Hp):
                    a = np.asarray(fb[k], dtype=np.float64)
                    recs[s]["shape_cols"][k] = a.shape[1]
                    recs[s]["shapes"][k][:, : a.shape[1]] = a
        first += size
    return recs


def record_steps(options, mpa, sc, n_steps, **kw):
    """The step problems of a closed loop driven by the sampled optimizer's whole-step path."""
    opt = MonteCarloTreeSearchHip(options)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc), **kw)
    steps = []

    def plan_step(prob):
        steps.append((prob, MonteCarloTreeSearchHip.step_seeds(prob)))
        return opt.run_optimizer_step(prob, mpa)

    for _ in range(n_steps):
        ctl.step(plan_step=plan_step)
    opt.handle.close()
    return steps


def spread(xs):
    return "%.1f steps/s (median of %d runs, %.1f .. %.1f)" % (float(np.median(xs)), len(xs), min(xs), max(xs))


def measure(name, options, sc, n_steps, native_steps, **kw):
    mpa = get_mpa(options)
    steps = record_steps(options, mpa, sc, n_steps, **kw)
    levels = [len(p["level_sizes"]) for p, _ in steps]
    h = Handle(options)
    h.upload_mpa(mpa)
    for prob, seeds in steps:  # (ii) equals (i), and both are warm
        fb = [f if f is not None else [] for f in prob["fallback"]]
        a = h.plan_step_sampled(prob["iters"], prob["preds"], fb, seeds)
        b = level_loop(h, prob, seeds, options.Hp)
        assert a.tobytes() == b.tobytes(), name
    args = [(h.step_args(p["iters"], p["preds"], [f if f is not None else [] for f in p["fallback"]]), s) for p, s in steps]
    rate = {"i": [], "ii": []}
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for prob, seeds in steps:
            level_loop(h, prob, seeds, options.Hp)
        rate["i"].append(len(steps) / (time.perf_counter() - t0))
        t0 = time.perf_counter()
        for (n, arr, off, idx, fb, _), seeds in args:
            out = abi.out_array(n)
            sd = (abi.C.c_uint32 * n)(*seeds)
            rc = h.L.pdmpc_plan_step_sampled(h.h, n, arr, abi.i32p(off), abi.i32p(idx), fb, sd, abi.out_ptr(out))
            assert rc == 0
        rate["ii"].append(len(steps) / (time.perf_counter() - t0))
    st = h.stats()
    h.close()
    # (iii) the native controller's closed loop
    h = Handle(options)
    h.upload_mpa(mpa)
    nat = NativeController(options, sc, mpa, h, coupling="distance", optimizer="sampled", **kw)
    nat.run(2)
    rate["iii"] = []
    for _ in range(RUNS):
        ms = nat.run(native_steps)
        rate["iii"].append(1e3 * len(ms) / float(np.sum(ms)))
    nat.close()
    h.close()
    print("%s: %d vehicles, Hp %d, %d recorded steps of %d-%d computation levels" % (name, options.amount, options.Hp, len(steps), min(levels), max(levels)))
    print("  (i)   one plan_batch_sampled per level, host hand-over:   %s" % spread(rate["i"]))
    print("  (ii)  pdmpc_plan_step_sampled, one launch per step:      %s" % spread(rate["ii"]))
    print("  (iii) native controller closed loop, host-inclusive:     %s" % spread(rate["iii"]))
    print("  last (ii) call: kernel %d, LDS %d B per workgroup" % (st["kernel"], st["lds_bytes"]))
    sys.stdout.flush()


def measure_budgets(budgets):
    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32, max_nodes=1 << 12)
    sc = commonroad_scenario(options, seed=1)
    mpa = get_mpa(options)
    steps = record_steps(options, mpa, sc, 3 if QUICK else 10)
    h = Handle(options)
    h.upload_mpa(mpa)
    step_ms, solo_ms, info = {b: [] for b in budgets}, {b: [] for b in budgets}, {}

    def launch_ms(call):
        call()
        st = h.stats()
        return st["kernel_ms"], st

    for run in range(RUNS + 1):  # (the first pass over the budgets warms up and is dropped)
        for b in budgets:
            h.set_sampled_budget(b)
            tot = solo = 0.0
            for prob, seeds in steps:
                fb = [f if f is not None else [] for f in prob["fallback"]]
                ms, st = launch_ms(lambda: h.plan_step_sampled(prob["iters"], prob["preds"], fb, seeds))
                tot += ms
                info[b] = (h.last_sampled_kernel(), st["lds_bytes"], st["safe_replans"])
                ms, _ = launch_ms(lambda: h.plan_batch_sampled(prob["iters"], seeds))
                solo = max(solo, ms)
            if run:
                step_ms[b].append(tot / len(steps))
                solo_ms[b].append(solo)
    h.close()
    print("C2-like: 20 vehicles, Hp 8, %d recorded steps; kernel time per step, median of %d alternating runs (min .. max)" % (len(steps), RUNS))
    print("  watchdog re-plans in resident slices since the handle was created: %d" % max(v[2] for v in info.values()))
    for b in budgets:
        print("  budget %5d  %-32s LDS %6d B  step %9.3f ms (%.3f .. %.3f)  independent searches, slowest launch %9.3f ms (%.3f .. %.3f)"
              % (b, info[b][0], info[b][1], float(np.median(step_ms[b])), min(step_ms[b]), max(step_ms[b]), float(np.median(solo_ms[b])), min(solo_ms[b]), max(solo_ms[b])))
    sys.stdout.flush()


if __name__ == "__main__":
    if "--budget" in sys.argv:
        measure_budgets([int(b) for b in sys.argv[sys.argv.index("--budget") + 1].split(",")])
        sys.exit(0)
    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32, max_nodes=1 << 12)
    measure("C2-like", options, commonroad_scenario(options, seed=1), 3 if QUICK else 10, 5 if QUICK else 20)
    options = Config(scenario_type=ScenarioType.commonroad, amount=512, Hp=10, max_vehicles=512, max_nodes=1 << 12)
    measure("C4-like", options, commonroad_scenario(options, seed=3, tiles=26), 2 if QUICK else 4, 2 if QUICK else 4, priority_strategy="coloring")
