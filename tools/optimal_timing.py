"""What optimal-priority control costs: the enumeration of the unique prioritizations on the device (pdmpc_unique_priorities)
against its host twin, the host build of the K-instance batch, and the closed-loop step against the Python twin planned by the oracle.

    python tools/optimal_timing.py [--repeat R] [--steps S] [--out FILE]

  enumerate  K_6 (E = 15), K_7 (E = 21), K_8 (E = 28): wall-clock ms of pdmpc_unique_priorities (count + scan + read-back of K +
             write + order + read-back; median of R after one warm-up) and of pdmpc_unique_priorities_host (one call)
  build      pdmpc_controller_optimal_build without a handle (host twin enumeration + K assemble_step + flattening), circle 3..6
  step       pdmpc_controller_optimal_run on the circle with 3..6 vehicles (full coupling: K = n!), median ms per step and its
             parts (build incl. the device enumeration, pack, enqueue, wait + read-back, choose, apply); next to it the Python twin
             (pdmpc.optimal.optimal_step) with the CPU oracle as planner, seconds per step
Run under `rocprofv3 --kernel-trace --stats -- python tools/optimal_timing.py` for the profiler's kernel summary.
"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "p-dmpc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from pdmpc.backend import CapacityError, Handle, unique_priorities_call  # noqa: E402
from pdmpc.config import Config, ScenarioType  # noqa: E402
from pdmpc.controller import PrioritizedSequentialController  # noqa: E402
from pdmpc.mpa import get_mpa  # noqa: E402
from pdmpc.native_controller import NativeController  # noqa: E402
from pdmpc.optimal import optimal_step  # noqa: E402
from pdmpc.optimizer import GraphSearchHip  # noqa: E402
from pdmpc.scenario import circle_scenario  # noqa: E402


def complete(n):
    return np.ones((n, n), dtype=np.int64) - np.eye(n, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import math

    say("enumerate (pdmpc_unique_priorities on the device vs pdmpc_unique_priorities_host)")
    h = Handle(Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 12))
    for n in (6, 7, 8):
        A = complete(n)
        K = math.factorial(n)
        h.unique_priorities(A, K)
        dev = []
        for _ in range(args.repeat):
            t = time.perf_counter()
            prio, masks = h.unique_priorities(A, K)
            dev.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        hp, hm = unique_priorities_call(A, K)
        host = (time.perf_counter() - t) * 1e3
        same = np.array_equal(hp, prio) and np.array_equal(hm, masks)
        say("  K_%d  E=%2d  2^E=%10d  K=%6d  device %9.3f ms (min %.3f)  host twin %10.1f ms  equal=%s"
            % (n, n * (n - 1) // 2, 1 << (n * (n - 1) // 2), len(masks), statistics.median(dev), min(dev), host, same))
    h.close()

    say("build (pdmpc_controller_optimal_build without a handle: host twin enumeration, K x assemble_step, flattening)")
    for n in (3, 4, 5, 6):
        options = Config(scenario_type=ScenarioType.circle, amount=n, Hp=5, max_nodes=1 << 14)
        sc = circle_scenario(options)
        mpa = get_mpa(options)
        nat = NativeController(options, sc, mpa, None, coupling="full")
        ts = []
        for _ in range(args.repeat):
            t = time.perf_counter()
            K = nat.optimal_build(1000)
            ts.append((time.perf_counter() - t) * 1e3)
        nat.close()
        say("  circle %d  K=%4d  slots=%5d  build %8.3f ms (median of %d)" % (n, K, K * n, statistics.median(ts), len(ts)))

    say("step (pdmpc_controller_optimal_run, circle, full coupling; Python twin + CPU oracle alongside)")
    from oracle import oracle

    for n in (3, 4, 5, 6):
        K = math.factorial(n)
        options = Config(scenario_type=ScenarioType.circle, amount=n, Hp=5, max_vehicles=n * K, max_nodes=1 << 14)
        sc = circle_scenario(options)
        mpa = get_mpa(options)
        opt = GraphSearchHip(options)
        opt._ensure_mpa(mpa)
        nat = NativeController(options, sc, mpa, opt.handle, coupling="full")
        nat.optimal_run(K, 1)  # (warm-up: arenas, code objects)
        nat.timing_mean(reset=True)
        ms = nat.optimal_run(K, args.steps)
        parts = nat.timing_mean(reset=True)
        nat.close()
        opt.handle.close()
        py = PrioritizedSequentialController(options, sc, mpa, None, coupling="full")
        unbounded = copy.copy(options)
        unbounded.max_nodes = 1 << 30
        n_py = max(1, min(args.steps, 3 if n < 6 else 1))
        t = time.perf_counter()
        for _ in range(n_py):
            optimal_step(py, lambda b: oracle.plan_step(unbounded, mpa, b, n_threads=min(16, os.cpu_count() or 1))[0], K)
        py_s = (time.perf_counter() - t) / n_py
        say("  circle %d  K=%4d  slots=%5d  native %8.2f ms/step (median of %d)  [build %.2f pack %.2f enqueue %.2f wait+read %.2f choose %.2f apply %.2f]  python+oracle %.2f s/step"
            % (n, K, n * K, statistics.median(ms), len(ms), parts["build"], parts["pack"], parts["enqueue"], parts["wait_and_read_back"], parts["choose"],
               parts["apply"], py_s))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    try:
        main()
    except CapacityError as e:
        sys.exit("capacity: %s" % e)
