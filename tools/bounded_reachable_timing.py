"""Timing of the lanelet bounding of the reachable sets and of the coupler on the bounded sets on the C2 / C3 / C4
road networks of bench.py.

For every workload: a closed loop of the native controller with a handle (distance coupling, the benchmark's configuration) records
the plant states of a few steps; the Python controller's traffic info gives every vehicle's predicted-lanelet polygon at each state.
On each recorded state the tool times
  bound     the bounding kernel, step-Hp sets only / every step (HIP events, pdmpc_bounded_reachable_kernel_ms[0])
  couple    the coupling kernels on the bounded step-Hp sets (pdmpc_bounded_reachable_kernel_ms[1])
  call      the whole device path from Python: pdmpc_bound_reachable_sets (step Hp) + pdmpc_bounded_set_coupling
  host      the host twins: pdmpc_bound_reachable_sets_host (step Hp) + pdmpc_polygon_set_coupling_host
checks that device and host give the same adjacency, and counts the coupled pairs with and without bounding.  It then runs the C3
configuration with bounding, reachable-set coupling and parallel predecessors as bounded reachable sets, and reports the largest
obstacle soup a slot's search sees.

    python tools/bounded_reachable_timing.py [--steps 6] [--reps 20] [--out profiles/bounded_reachable_timing.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

from reachable_coupling_timing import WORKLOADS, recorded_states, world  # noqa: E402


def lanelet_polygons(options, mpa, sc, state):
    """Every vehicle's raw predicted-lanelet polygon and 1-based trim at a recorded plant state (the Python controller's traffic info)."""
    from pdmpc.controller import Measurement, PrioritizedSequentialController
    from pdmpc.reachability import lanelet_polygon
    from pdmpc.road_network import boundary_provider

    x, y, yaw, speed, steer = state
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="none", boundary_provider=boundary_provider(sc))
    py.meas = [Measurement(float(a), float(b), float(c), float(d), float(e)) for a, b, c, d, e in zip(x, y, yaw, speed, steer)]
    py._traffic_info()
    return [lanelet_polygon(*b) for b in py.boundary], py.trims.copy()


def time_workload(name, steps, reps, lines):
    from pdmpc.backend import bound_reachable_sets_call, polygon_set_coupling_call

    options, mpa, handle, states = recorded_states(name, steps)
    _, _, sc, _ = world(name)
    L = mpa.local_reachable_sets_conv
    handle.upload_reachable_sets(L)
    kb, kb_all, kc, call, host, pairs_b, pairs_u = [], [], [], [], [], [], []
    for x, y, yaw, trim in states:
        speed = np.array([mpa.trims[t - 1].speed for t in trim])
        steer = np.array([mpa.trims[t - 1].steering for t in trim])
        lan, trims = lanelet_polygons(options, mpa, sc, (x, y, yaw, speed, steer))
        assert np.array_equal(trims, trim)
        adj_u, _ = handle.reachable_set_coupling(x, y, yaw, trim)
        pairs_u.append(int(adj_u.sum()) // 2)
        handle.bound_reachable_sets(x, y, yaw, trim, lan, True)
        for _ in range(reps):
            handle.bound_reachable_sets(x, y, yaw, trim, lan, True)
            kb_all.append(handle.bounded_reachable_kernel_ms()[0])
        handle.bound_reachable_sets(x, y, yaw, trim, lan, False)  # warm-up
        handle.bounded_set_coupling()
        for _ in range(reps):
            t0 = time.perf_counter()
            handle.bound_reachable_sets(x, y, yaw, trim, lan, False)
            adj_d, _ = handle.bounded_set_coupling()
            call.append(1e3 * (time.perf_counter() - t0))
            t = handle.bounded_reachable_kernel_ms()
            kb.append(t[0])
            kc.append(t[1])
        for _ in range(max(1, reps // 10)):
            t0 = time.perf_counter()
            sets, _ = bound_reachable_sets_call(L, x, y, yaw, trim, lan, False)
            adj_h, _ = polygon_set_coupling_call([s[-1] for s in sets])
            host.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(adj_d, adj_h), name
        pairs_b.append(int(adj_d.sum()) // 2)
    handle.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    lines.append("%-3s n=%4d Hp=%2d  bound kernel %8.4f ms (every step %8.4f ms)   couple kernel %8.4f ms   call %8.4f ms   host twins %9.3f ms   "
                 "coupled pairs/step %.1f bounded, %.1f unbounded   (%d states, median of %d / %d)"
                 % (name, options.amount, options.Hp, med(kb), med(kb_all), med(kc), med(call), med(host), float(np.mean(pairs_b)), float(np.mean(pairs_u)),
                    len(states), reps, max(1, reps // 10)))


def c3_soup(steps, lines):
    """Largest obstacle soup of a slot in the C3 configuration with bounding, reachable-set coupling and parallel predecessors as
    bounded reachable sets (host-assembled polygons' columns plus up to PDMPC_VMAX columns per step of every sequential predecessor)."""
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip

    options, mpa, sc, prio = world("c3", is_deal_prediction_inconsistency=True, bound_reachable_sets=True)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, sc, mpa, opt.handle, coupling="reachable_set", priority_strategy=prio)
    worst = (0, 0, 0)
    t_step = []
    for k in range(steps):
        t0 = time.perf_counter()
        nat.step()
        t_step.append(1e3 * (time.perf_counter() - t0))
        prob = nat.problem()
        for s, it in enumerate(prob["iters"]):
            host_cols = sum(np.asarray(p).shape[1] for p in it.obstacles) + sum(np.asarray(p).shape[1] for row in it.dynamic_obstacle_area for p in row)
            cols = host_cols + 8 * options.Hp * len(prob["preds"][s])
            worst = max(worst, (cols, host_cols, len(it.dynamic_obstacle_area)))
    nat.close()
    opt.handle.close()
    lines.append("c3 with bounding + reachable-set coupling + parallel predecessors as bounded reachable sets, %d steps, no capacity error: largest "
                 "soup %d columns (%d assembled on the host, %d dynamic-obstacle rows); step median %.2f ms" % (steps, worst[0], worst[1], worst[2], float(np.median(t_step))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", default="c2,c3,c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounded_reachable_timing.txt"))
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
