"""Timing of the reachable-set coupler on the C2 / C3 / C4 road networks of bench.py.

For every workload: a closed loop of the native controller with a handle (distance coupling, the benchmark's configuration) records
the plant states of a few steps; on each recorded state the tool times
  kernel   the two coupling passes on the device (HIP events around them, pdmpc_reachable_set_coupling_kernel_ms)
  call     the whole device coupler call from Python (staging copy, launches, one read-back, synchronisation)
  host     the host twin (pdmpc_reachable_set_coupling_host)
and checks that device and host give the same adjacency.  It then runs the C3 configuration with both reachable-set features on
(reachable-set coupling, parallel predecessors as reachable sets) and reports the largest obstacle soup a slot's search sees.

    python tools/reachable_coupling_timing.py [--steps 6] [--reps 20] [--out profiles/reachable_coupling_timing.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd")]

import numpy as np  # noqa: E402

WORKLOADS = {  # bench.py workload_defaults: vehicles, Hp, priorities, max_num_CLs
    "c2": (20, 8, "constant", 99),
    "c3": (128, 8, "coloring", 2),
    "c4": (512, 10, "coloring", 99),
}


def world(name, seed=1, **extra):
    from pdmpc.config import Config, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.road_network import commonroad_scenario

    n, Hp, prio, cls = WORKLOADS[name]
    options = Config(scenario_type=ScenarioType.commonroad, amount=n, Hp=Hp, max_vehicles=max(n, 32), max_nodes=(1 << 17) if name == "c2" else (1 << 16),
                     max_num_CLs=cls, **extra)
    return options, get_mpa(options), commonroad_scenario(options, seed=seed, tiles=max(1, (n + 19) // 20)), prio


def recorded_states(name, steps):
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip

    options, mpa, sc, prio = world(name)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, sc, mpa, opt.handle, coupling="distance", priority_strategy=prio)
    states = []
    for _ in range(steps):
        nat.step()
        st = nat.state()
        trims = [mpa.trim_from_values(float(v), float(d)) for v, d in zip(st["speed"], st["steering"])]
        states.append((st["x"].copy(), st["y"].copy(), st["yaw"].copy(), np.array(trims)))
    nat.close()
    return options, mpa, opt.handle, states


def time_workload(name, steps, reps, lines):
    from pdmpc.backend import reachable_set_coupling_call

    options, mpa, handle, states = recorded_states(name, steps)
    L = mpa.local_reachable_sets_conv
    handle.upload_reachable_sets(L)
    kern, call, host, pairs = [], [], [], []
    for x, y, yaw, trim in states:
        adj_d, _ = handle.reachable_set_coupling(x, y, yaw, trim)  # warm-up
        for _ in range(reps):
            t0 = time.perf_counter()
            adj_d, _ = handle.reachable_set_coupling(x, y, yaw, trim)
            call.append(1e3 * (time.perf_counter() - t0))
            kern.append(handle.reachable_set_coupling_kernel_ms())
        for _ in range(max(1, reps // 4)):
            t0 = time.perf_counter()
            adj_h, _ = reachable_set_coupling_call(L, x, y, yaw, trim)
            host.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(adj_d, adj_h), name
        pairs.append(int(adj_d.sum()) // 2)
    handle.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    lines.append("%-3s n=%4d Hp=%2d  kernel %8.4f ms   call %8.4f ms   host twin %8.4f ms   coupled pairs/step %.1f   (%d states, median of %d / %d)"
                 % (name, options.amount, options.Hp, med(kern), med(call), med(host), float(np.mean(pairs)), len(states), reps, max(1, reps // 4)))


def c3_soup(steps, lines):
    """Largest obstacle soup of a slot (host-assembled polygons' columns plus up to PDMPC_VMAX columns per step of every sequential
    predecessor handed over on the device) in the C3 configuration with both reachable-set features on."""
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip

    options, mpa, sc, prio = world("c3", is_deal_prediction_inconsistency=True)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, sc, mpa, opt.handle, coupling="reachable_set", priority_strategy=prio)
    worst = (0, 0, 0)
    for k in range(steps):
        nat.step()
        prob = nat.problem()
        for s, it in enumerate(prob["iters"]):
            host_cols = sum(np.asarray(p).shape[1] for p in it.obstacles) + sum(np.asarray(p).shape[1] for row in it.dynamic_obstacle_area for p in row)
            cols = host_cols + 8 * options.Hp * len(prob["preds"][s])
            worst = max(worst, (cols, host_cols, len(it.dynamic_obstacle_area)))
    nat.close()
    opt.handle.close()
    lines.append("c3 with reachable-set coupling + parallel predecessors as reachable sets, %d steps, no capacity error: largest soup %d columns "
                 "(%d assembled on the host, %d dynamic-obstacle rows)" % (steps, worst[0], worst[1], worst[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", default="c2,c3,c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reachable_coupling_timing.txt"))
    args = ap.parse_args()
    lines = []
    for name in args.workloads.split(","):
        time_workload(name, args.steps, args.reps, lines)
        print(lines[-1], flush=True)
    c3_soup(args.steps, lines)
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
