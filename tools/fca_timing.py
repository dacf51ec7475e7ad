"""Timing of the future collision assessment (FCA priorities) on the C2 and C4 road networks of bench.py.

For every workload a closed loop of the native controller with a handle (distance coupling, FCA priorities) records a few steps; on
each step's reference points and coupled pairs the tool times
  kernel   the two passes on the device (HIP events around them, pdmpc_fca_kernel_ms)
  call     the whole device call (staging copy, launches, one read-back of the counts, synchronisation, the sort on the host)
  host     the host twin (pdmpc_fca_collisions_host)
(both calls from arguments packed once, so no Python packing is timed) and checks that device and host give the same counts.  It also
reports part [0] of pdmpc_controller_last_timing (building the step problem, FCA included) of the same closed loop.

Grouped: M in {1, 2, 4, 8} C2-like closed loops (seeds 1 .. M), the last recorded step of each as one group:
one pdmpc_fca_collisions_grouped against M pdmpc_fca_collisions, in kernel time (HIP events) and as whole calls, with equal counts.

    python tools/fca_timing.py [--steps 6] [--reps 20] [--grouped 1] [--out profiles/fca_timing.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd")]

import numpy as np  # noqa: E402

WORKLOADS = {"c2": (20, 8), "c4": (512, 10)}  # bench.py workload_defaults: vehicles, Hp


GROUPED_MS = (1, 2, 4, 8)


def recorded_steps(name, steps, seed=1):
    from pdmpc.config import Config, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.native_controller import NativeController
    from pdmpc.optimizer import GraphSearchHip
    from pdmpc.road_network import commonroad_scenario

    n, Hp = WORKLOADS[name]
    options = Config(scenario_type=ScenarioType.commonroad, amount=n, Hp=Hp, max_vehicles=max(n, 32), max_nodes=(1 << 17) if name == "c2" else (1 << 16))
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=seed, tiles=max(1, (n + 19) // 20))
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, sc, mpa, opt.handle, coupling="distance", priority_strategy="fca")
    max_distance = 2 * mpa.get_max_speed_of_mpa() * options.dt_seconds * Hp  # DistanceCoupler (the controller's coupling)
    recs, build_ms = [], []
    for _ in range(steps):
        nat.step()
        build_ms.append(nat.last_timing()["build"])
        prob = nat.problem()
        refs, pos = [None] * n, np.zeros((n, 2))
        for s, v in enumerate(prob["order"]):
            it = prob["iters"][s]
            refs[v] = np.asarray(it.reference_trajectory_points, dtype=np.float64).reshape(Hp, 2)
            pos[v] = [it.x0[0], it.x0[1]]
        d = np.hypot(pos[:, None, 0] - pos[None, :, 0], pos[:, None, 1] - pos[None, :, 1])
        A = d <= max_distance
        np.fill_diagonal(A, False)
        recs.append((refs, A))
    nat.close()
    return options, sc, opt.handle, recs, build_ms


def time_workload(name, steps, reps, lines):
    from pdmpc.backend import fca_pack, fca_pairs, load_library

    L = load_library()
    options, sc, handle, recs, build_ms = recorded_steps(name, steps)
    veh = sc.vehicles[0]
    kern, call, host, pairs, hits = [], [], [], [], []
    for refs, A in recs:
        args, (coll, _), keep = fca_pack(refs, fca_pairs(A), veh.Length, veh.Width, options.offset, sc.obstacles)
        assert L.pdmpc_fca_collisions(handle.h, *args) == 0  # warm-up
        for _ in range(reps):
            t0 = time.perf_counter()
            rc = L.pdmpc_fca_collisions(handle.h, *args)
            call.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0
            kern.append(handle.fca_kernel_ms())
        dev = coll.copy()
        for _ in range(reps):
            t0 = time.perf_counter()
            rc = L.pdmpc_fca_collisions_host(*args)
            host.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0
        assert np.array_equal(dev, coll), name
        pairs.append(int(A.sum()) // 2)
        hits.append(int(coll.sum()))
        del keep
    handle.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    lines.append("%-3s n=%4d Hp=%2d  kernel %8.4f ms   call %8.4f ms   host twin %8.4f ms   coupled pairs/step %.1f   counted collisions/step %.1f   "
                 "controller build (part [0]) %.3f ms   (%d steps, median of %d)"
                 % (name, options.amount, options.Hp, med(kern), med(call), med(host), float(np.mean(pairs)), float(np.mean(hits)), med(build_ms), len(recs), reps))


def time_grouped(steps, reps, lines):
    from pdmpc.backend import Handle, fca_grouped_pack, fca_pack, fca_pairs, load_library
    from pdmpc.config import Config, ScenarioType

    L = load_library()
    loops = []
    for seed in range(1, max(GROUPED_MS) + 1):
        options, sc, handle, recs, _ = recorded_steps("c2", steps, seed)
        handle.close()
        refs, A = recs[-1]
        loops.append(dict(reference_points=refs, pairs=fca_pairs(A), length=sc.vehicles[0].Length, width=sc.vehicles[0].Width, offset=options.offset,
                          obstacles=sc.obstacles))
    n, Hp = WORKLOADS["c2"]
    h = Handle(Config(scenario_type=ScenarioType.commonroad, amount=n, Hp=Hp, max_vehicles=n * max(GROUPED_MS), max_nodes=1 << 12))
    lines.append("grouped: M C2-like groups (n=%d, Hp=%d, seeds 1..M, step %d of each closed loop), median of %d" % (n, Hp, steps, reps))
    for M in GROUPED_MS:
        groups = loops[:M]
        gargs, per_group, gkeep = fca_grouped_pack(groups)
        solo = [fca_pack(g["reference_points"], g["pairs"], g["length"], g["width"], g["offset"], g["obstacles"]) for g in groups]
        gk, gc, uk, uc = [], [], [], []
        for r in range(reps + 2):
            t0 = time.perf_counter()
            rc = L.pdmpc_fca_collisions_grouped(h.h, *gargs)
            t1 = time.perf_counter()
            assert rc == 0
            k = h.fca_kernel_ms()
            tu, ku = 0.0, 0.0
            for args, _, _ in solo:
                t2 = time.perf_counter()
                rc = L.pdmpc_fca_collisions(h.h, *args)
                tu += time.perf_counter() - t2
                assert rc == 0
                ku += h.fca_kernel_ms()
            if r >= 2:
                gk.append(k)
                gc.append(1e3 * (t1 - t0))
                uk.append(ku)
                uc.append(1e3 * tu)
        for (coll, prio), (_, (coll1, prio1), _) in zip(per_group(), solo):
            assert np.array_equal(coll, coll1) and np.array_equal(prio, prio1), M
        med = lambda v: float(np.median(v))  # noqa: E731
        lines.append("  M=%d  kernels (events) grouped %.4f ms, ungrouped %.4f ms   whole calls grouped %.4f ms, ungrouped %.4f ms   counted collisions %d"
                     % (M, med(gk), med(uk), med(gc), med(uc), sum(int(c.sum()) for c, _ in per_group())))
        print(lines[-1], flush=True)
        del gkeep
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workloads", default="c2,c4")
    ap.add_argument("--grouped", type=int, default=1, help="0: without the grouped call against M ungrouped ones")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fca_timing.txt"))
    args = ap.parse_args()
    lines = []
    for name in args.workloads.split(","):
        time_workload(name, args.steps, args.reps, lines)
        print(lines[-1], flush=True)
    if args.grouped:
        time_grouped(args.steps, args.reps, lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
