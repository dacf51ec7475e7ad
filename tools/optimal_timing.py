"""What optimal-priority control costs: the enumeration of the unique prioritizations on the device (pdmpc_unique_priorities)
against its host twin, the host build of the K-instance batch, and the closed-loop step against the Python twin planned by the oracle.

    python tools/optimal_timing.py [--repeat R] [--steps S] [--sections enumerate,build,step,grouped,solo] [--baseline-root DIR] [--out FILE]

  enumerate  K_6 (E = 15), K_7 (E = 21), K_8 (E = 28): wall-clock ms of pdmpc_unique_priorities (count + scan + read-back of K +
             write + order + read-back; median of R after one warm-up) and of pdmpc_unique_priorities_host (one call)
  build      pdmpc_controller_optimal_build without a handle (host twin enumeration + K assemble_step + flattening), circle 3..6
  step       pdmpc_controller_optimal_run on the circle with 3..6 vehicles (full coupling: K = n!), median ms per step and its
             parts (build incl. the device enumeration, pack, enqueue, wait + read-back, choose, apply); next to it the Python twin
             (pdmpc.optimal.optimal_step) with the CPU oracle as planner, seconds per step
  grouped    ONE pdmpc_unique_priorities_grouped against M pdmpc_unique_priorities calls, M in 1, 2, 4, 8, on the coupling graphs of M
             road-network members (6 vehicles, Hp 6, seeds 1 .. M) recorded at step 3 of their optimal-priority closed loops: whole calls,
             median of 20 x R
  solo       the solo optimal-priority step on the circle with 6 vehicles (K = 720) on this tree and on a built checkout of the parent
             commit (--baseline-root), five alternating fresh processes each: median and spread (max - min) of their medians
Run under `rocprofv3 --kernel-trace --stats -- python tools/optimal_timing.py` for the profiler's kernel summary.
"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("PDMPC_TREE", ROOT)  # (section solo: a worker imports the package and the library of this tree)
for p in (TREE, os.path.join(TREE, "p-dmpc_amd"), os.path.join(ROOT, "tests")):
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


def recorded_graphs(M):
    """the coupling graphs of M road-network members at step 3 of their optimal-priority closed loops"""
    from pdmpc.native_controller import NativeSweep
    from pdmpc.road_network import commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=6, Hp=6, max_vehicles=6 * 600 * M, max_nodes=1 << 12)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    cs = [NativeController(options, commonroad_scenario(options, seed=s), mpa, h, coupling="distance") for s in range(1, M + 1)]
    sweep = NativeSweep(cs, h)
    sweep.optimal_run(600, 3)
    graphs = []
    for c in cs:  # (instance 0 keeps every coupling: the step's graph is its predecessor lists, undirected)
        q = c.problem()
        A = np.zeros((c.n, c.n), dtype=np.int64)
        for s, preds in enumerate(q["preds"]):
            for t in preds:
                A[q["order"][s], q["order"][t]] = A[q["order"][t], q["order"][s]] = 1
        graphs.append(A)
    sweep.close()
    for c in cs:
        c.close()
    return h, graphs


def solo_worker(steps):
    """the solo step at K = 720 on the tree this process imports -> one RESULT line"""
    options = Config(scenario_type=ScenarioType.circle, amount=6, Hp=5, max_vehicles=6 * 720, max_nodes=1 << 14)
    sc = circle_scenario(options)
    mpa = get_mpa(options)
    opt = GraphSearchHip(options)
    opt._ensure_mpa(mpa)
    nat = NativeController(options, sc, mpa, opt.handle, coupling="full")
    nat.optimal_run(720, 2)
    ms = nat.optimal_run(720, steps)
    nat.close()
    opt.handle.close()
    print("RESULT %.6f" % statistics.median(ms), flush=True)


def solo_child(root, steps):
    import subprocess

    env = dict(os.environ, PDMPC_TREE=os.path.abspath(root))
    env.pop("PDMPC_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "solo", "--steps", str(steps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("a timing run failed with status %d: nothing more is started" % p.returncode)
    return float([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sections", default="enumerate,build,step,grouped")
    ap.add_argument("--baseline-root", help="a built checkout of the parent commit (section solo)")
    ap.add_argument("--worker")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker == "solo":
        return solo_worker(args.steps)
    sections = args.sections.split(",")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import math

    if "grouped" in sections:
        say("grouped (ONE pdmpc_unique_priorities_grouped vs M pdmpc_unique_priorities calls on the members' recorded graphs, whole calls, ms)")
        for M in (1, 2, 4, 8):
            h, graphs = recorded_graphs(M)
            counts = [len(h.unique_priorities(A, 100000)[1]) for A in graphs]
            h.unique_priorities_grouped(graphs, counts)
            one, each = [], []
            for _ in range(20 * args.repeat):
                t = time.perf_counter()
                got = h.unique_priorities_grouped(graphs, counts)
                one.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                alone = [h.unique_priorities(A, k) for A, k in zip(graphs, counts)]
                each.append((time.perf_counter() - t) * 1e3)
            same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, alone))
            say("  M=%d  E=%s  K=%s  grouped %.4f ms (min %.4f)  ungrouped %.4f ms (min %.4f)  ratio %.2f  equal=%s"
                % (M, [int(np.triu(A, 1).sum()) for A in graphs], counts, statistics.median(one), min(one), statistics.median(each), min(each),
                   statistics.median(each) / statistics.median(one), same))
            h.close()
    if "solo" in sections:
        if not args.baseline_root:
            raise SystemExit("--baseline-root: a built checkout of the parent commit is needed for the section solo")
        base, new = [], []
        for _ in range(5):
            base.append(solo_child(args.baseline_root, max(args.steps, 10)))
            new.append(solo_child(ROOT, max(args.steps, 10)))
        sb, sn = max(base) - min(base), max(new) - min(new)
        mb, mn = statistics.median(base), statistics.median(new)
        say("solo (pdmpc_controller_optimal_run, circle 6, K = 720, ms per step: median and spread of 5 alternating processes' medians)")
        say("  parent %.3f (spread %.3f, range %.3f .. %.3f)   this tree %.3f (spread %.3f)   %s"
            % (mb, sb, min(base), max(base), mn, sn, "inside the parent's range" if min(base) <= mn <= max(base) else
               ("below the parent's range" if mn < min(base) else "ABOVE the parent's range by %.3f ms" % (mn - max(base)))))
    if "enumerate" in sections:
        enumerate_section(args, say)
    if "build" in sections:
        build_section(args, say)
    if "step" in sections:
        step_section(args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def enumerate_section(args, say):
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


def build_section(args, say):
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



def step_section(args, say):
    import math

    from oracle import oracle

    say("step (pdmpc_controller_optimal_run, circle, full coupling; Python twin + CPU oracle alongside)")

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


if __name__ == "__main__":
    try:
        main()
    except CapacityError as e:
        sys.exit("capacity: %s" % e)
