"""What one joint search of centralized control costs on the GPU (pdmpc_plan_joint) and in the Python reference
(tests/joint_reference.py), on the same problems.

    python tools/joint_timing.py [--repeat R] [--out FILE] [--batched M [M ...]]

Workloads:
  systemtest  Config_systemtests_centralized.json on the circle: 2 vehicles, single_speed, Hp 5, the 20 problems of its closed loop
  n3          3 vehicles on the circle, Hp 4, the problem after two steps (63 769 joint nodes)
Per workload: kernel ms per joint search (HIP events of the launch, median of R repeats), pops and tree size per search, and the
reference's seconds for the same searches.  Run under `rocprofv3 --kernel-trace --stats -- python tools/joint_timing.py` for the
profiler's kernel summary.

--batched M: instead of the workloads above, M joint problems (the systemtest's 20, repeated) in ONE pdmpc_plan_joint -- one launch, one
wavefront per problem, what a sweep of M centralized closed loops hands over per time step -- against the same M problems in M calls
of one problem each: kernel ms (HIP events) and wall ms of the calls (the Python marshalling of the problems included in both).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "p-dmpc_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pdmpc.backend import Handle  # noqa: E402
from pdmpc.centralized import CentralizedController, centralized_mpa, centralized_options  # noqa: E402
from pdmpc.config import Config, MpaType, ScenarioType  # noqa: E402
from pdmpc.iteration_data import info_from_record  # noqa: E402
from pdmpc.scenario import circle_scenario  # noqa: E402

import joint_reference as jr  # noqa: E402


def closed_loop_problems(N, Hp, steps, max_vehicles=8):
    options = centralized_options(Config(scenario_type=ScenarioType.circle, amount=N, Hp=Hp, mpa_type=MpaType.single_speed, T_end=4, max_vehicles=max_vehicles))
    mpa = centralized_mpa(options)
    out = []
    ref_s = 0.0

    def plan(iters):
        nonlocal ref_s
        out.append(iters)
        t = time.perf_counter()
        recs = jr.plan_joint(options, mpa, [iters])
        ref_s += time.perf_counter() - t
        return [info_from_record(r, Hp) for r in recs]

    ctl = CentralizedController(options, circle_scenario(options), mpa, plan)
    for _ in range(steps):
        ctl.step()
    return options, mpa, out, ref_s


def measure(name, options, mpa, probs, ref_s, repeat, lines):
    h = Handle(options)
    h.upload_mpa(mpa)
    h.plan_joint(probs[:1])  # (first launch: code object load, arena touch)
    per, pops, nodes = [], [], []
    for prob in probs:
        ms = []
        for _ in range(repeat):
            rec = h.plan_joint([prob])
            st = h.stats()
            ms.append(st["kernel_ms"] / max(st["n_launches"], 1))
        per.append(statistics.median(ms))
        pops.append(int(rec["n_popped"][0]))
        nodes.append(int(rec["n_expanded"][0]))
    h.close()
    n = len(probs)
    lines.append("%s: %d joint searches of %d vehicles, Hp %d" % (name, n, len(probs[0]), options.Hp))
    lines.append("  GPU kernel ms per search: median %.3f  min %.3f  max %.3f  sum %.2f" % (statistics.median(per), min(per), max(per), sum(per)))
    lines.append("  pops per search: median %d  max %d   tree nodes: median %d  max %d" % (statistics.median(pops), max(pops), statistics.median(nodes), max(nodes)))
    lines.append("  us per pop (sum kernel / sum pops): %.2f" % (1e3 * sum(per) / max(sum(pops), 1)))
    lines.append("  Python reference: %.2f s for the %d searches (%.1f ms per search)" % (ref_s, n, 1e3 * ref_s / n))
    lines.append("  reference / GPU: %.1fx" % (ref_s * 1e3 / max(sum(per), 1e-9)))


def measure_batched(M, repeat, lines):
    """M problems in one launch against M launches of one problem"""
    options, mpa, probs, _ = closed_loop_problems(2, 5, 20, max_vehicles=2 * M)
    batch = [probs[i % len(probs)] for i in range(M)]
    h = Handle(options)
    h.upload_mpa(mpa)
    h.plan_joint(batch)  # (code object load, and the arena grows to what the largest problem needs)
    one_k, one_w, many_k, many_w = [], [], [], []
    for _ in range(repeat):
        t = time.perf_counter()
        h.plan_joint(batch)
        one_w.append(1e3 * (time.perf_counter() - t))
        st = h.stats()
        assert st["n_launches"] == 1, st
        one_k.append(st["kernel_ms"])
        t = time.perf_counter()
        k = 0.0
        for prob in batch:
            h.plan_joint([prob])
            k += h.stats()["kernel_ms"]
        many_w.append(1e3 * (time.perf_counter() - t))
        many_k.append(k)
    h.close()
    med = statistics.median
    lines.append("batched: %d joint searches of 2 vehicles, Hp 5 (the systemtest's 20 problems, repeated)" % M)
    lines.append("  ONE launch of %d problems: kernel ms median %.3f  min %.3f   wall ms of the call median %.3f" % (M, med(one_k), min(one_k), med(one_w)))
    lines.append("  %d launches of one problem: kernel ms (sum) median %.3f  min %.3f   wall ms of the calls median %.3f" % (M, med(many_k), min(many_k), med(many_w)))
    lines.append("  single launches / one launch: kernel %.1fx  wall %.1fx" % (med(many_k) / max(med(one_k), 1e-9), med(many_w) / max(med(one_w), 1e-9)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batched", type=int, nargs="+", default=None, metavar="M")
    a = ap.parse_args()
    lines = []
    if a.batched:
        for M in a.batched:
            measure_batched(M, a.repeat, lines)
    else:
        options, mpa, probs, ref_s = closed_loop_problems(2, 5, 20)
        measure("systemtest (circle, 2 vehicles)", options, mpa, probs, ref_s, a.repeat, lines)
        options, mpa, probs, _ = closed_loop_problems(3, 4, 3)
        prob = probs[2]
        t = time.perf_counter()
        jr.plan_joint(options, mpa, [prob])
        ref_s = time.perf_counter() - t
        measure("n3 (circle, 3 vehicles)", options, mpa, [prob], ref_s, a.repeat, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
