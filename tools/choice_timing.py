"""Timing of the choice on the device (pdmpc_plan_step_chosen, pdmpc_controller_set_device_choice, pdmpc_sweep_explore_run).

(a) C5 (20 vehicles x 64 prioritizations, Hp 8, bench.py's closed loop: 4 plain steps, then explorative steps that follow the
    controller's own prioritization): host-inclusive milliseconds per step of pdmpc_controller_explore_run under three variants --
    the parent commit's library, this commit with the switch off, this commit with the switch on -- and the kernel time of the two
    choice launches (pdmpc_choice_kernel_ms).
(b) A sweep of M = 1, 2, 4, 8 C2-sized explorative members (20 vehicles, Hp 8, n_perm 8, seeds 1 .. M) on one handle
    (pdmpc_sweep_explore_run) against the same M loops stepped one after the other by the parent commit's library
    (pdmpc_controller_explore_run(1) each per lock-step): steps/s per member.
Baseline: a built checkout of the parent commit in a directory of its own (--baseline-root: its p-dmpc_amd/pdmpc package and its
p-dmpc_amd/csrc/libpdmpc_hip.so).  Every measurement is a fresh process; the variants alternate, `--rounds` times, so the parent is
measured several times and its own run-to-run spread (max - min of its medians) is known.

    python tools/choice_timing.py --baseline-root DIR [--rounds 3] [--out profiles/choice_timing.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 2, 4, 8)
C5_PERM, SWEEP_PERM = 64, 8
SKIP, WARMUP, TIMED = 4, 8, 32


def c5_worker(device_choice):
    import numpy as np
    from pdmpc.backend import Handle
    from pdmpc.config import Config, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=20 * C5_PERM, max_nodes=1 << 16)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    nat = NativeController(options, commonroad_scenario(options, seed=1), mpa, h, coupling="distance")
    if device_choice:
        nat.set_device_choice(True)
    nat.run(SKIP)
    nat.explore_follow_own(True)
    nat.explore_run(C5_PERM, WARMUP)
    nat.timing_mean(reset=True)
    ms = nat.explore_run(C5_PERM, TIMED)
    out = {"median": float(np.median(ms)), "mean": float(np.mean(ms)), "parts": nat.timing_mean()}
    if device_choice:
        out["choice_kernel_ms"] = h.choice_kernel_ms()
    st = nat.state()
    out["state"] = [float(np.sum(st[k])) for k in ("x", "y", "yaw")]  # (the variants drive the same closed loop)
    nat.close()
    h.close()
    print("RESULT " + json.dumps(out), flush=True)


def sweep_worker(kind):
    import numpy as np
    from pdmpc.backend import Handle
    from pdmpc.config import Config, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import commonroad_scenario

    out = {}
    for M in MS:
        options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=20 * SWEEP_PERM * M, max_nodes=1 << 16)
        mpa = get_mpa(options)
        h = Handle(options)
        h.upload_mpa(mpa)
        cs = [NativeController(options, commonroad_scenario(options, seed=s), mpa, h, coupling="distance") for s in range(1, M + 1)]
        if kind == "baseline":
            ms = [sum(float(c.explore_run(SWEEP_PERM, 1)[0]) for c in cs) for _ in range(WARMUP + TIMED)][WARMUP:]
            out[str(M)] = {"median": float(np.median(ms))}
        else:
            from pdmpc.native_controller import NativeSweep

            sweep = NativeSweep(cs, h)
            sweep.explore_run(SWEEP_PERM, WARMUP)
            ms = sweep.explore_run(SWEEP_PERM, TIMED)
            out[str(M)] = {"median": float(np.median(ms)), "choice_kernel_ms": h.choice_kernel_ms(), "parts": sweep.last_timing()}
            sweep.close()
        for c in cs:
            c.close()
        h.close()
    print("RESULT " + json.dumps(out), flush=True)


def child(root, *args):
    """A fresh process on the tree under `root` (its package and its library) -> the JSON of its RESULT line."""
    env = dict(os.environ, PDMPC_TREE=root)
    env.pop("PDMPC_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("a timing run failed with status %d: nothing more is started" % p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "choice_timing.txt"))
    ap.add_argument("--worker")
    args = ap.parse_args()
    if args.worker:
        tree = os.environ.get("PDMPC_TREE", ROOT)
        sys.path[:0] = [tree, os.path.join(tree, "p-dmpc_amd")]
        if args.worker.startswith("c5"):
            c5_worker(args.worker == "c5-on")
        else:
            sweep_worker(args.worker[len("sweep-"):])
        return
    if not args.baseline_root or args.rounds < 2:
        raise SystemExit("--baseline-root: a built checkout of the parent commit is needed; --rounds: at least 2")
    import numpy as np

    base_root = os.path.abspath(args.baseline_root)
    c5 = {"parent": [], "off": [], "on": []}
    sw = {"parent": [], "sweep": []}
    for r in range(args.rounds):
        c5["parent"].append(child(base_root, "--worker", "c5-off"))
        c5["off"].append(child(ROOT, "--worker", "c5-off"))
        c5["on"].append(child(ROOT, "--worker", "c5-on"))
        sw["parent"].append(child(base_root, "--worker", "sweep-baseline"))
        sw["sweep"].append(child(ROOT, "--worker", "sweep-sweep"))
        print("round %d done" % (r + 1), flush=True)
    states = {json.dumps(run["state"]) for runs in c5.values() for run in runs}
    lines = ["(a) C5, 20 vehicles x %d prioritizations, Hp 8: pdmpc_controller_explore_run after %d plain and %d explorative warm-up steps, %d steps timed," % (C5_PERM, SKIP, WARMUP, TIMED),
             "    host-inclusive ms per step; median (and spread = max - min) of the medians of %d alternating fresh processes per variant" % args.rounds,
             "    the three variants end on the same plant state: %s" % ("yes" if len(states) == 1 else "NO")]
    med = {k: [run["median"] for run in v] for k, v in c5.items()}
    spread = max(med["parent"]) - min(med["parent"])
    for k, name in (("parent", "parent commit          "), ("off", "this commit, switch off"), ("on", "this commit, switch on ")):
        m = float(np.median(med[k]))
        parts = {p: float(np.median([run["parts"][p] for run in c5[k]])) for p in c5[k][0]["parts"]}
        lines.append("    %s %7.3f ms (spread %.3f)  %6.1f steps/s   parts: %s" % (name, m, max(med[k]) - min(med[k]), 1e3 / m, "  ".join("%s %.3f" % kv for kv in parts.items())))
    diff = float(np.median(med["on"])) - float(np.median(med["parent"]))
    lines.append("    switch on - parent: %+.3f ms; the parent's own spread: %.3f ms -> %s" % (
        diff, spread, "slower than the parent by more than its spread" if diff > spread else ("faster than the parent by more than its spread" if -diff > spread else "within the parent's spread")))
    lines.append("    pdmpc_choice_kernel_ms (both launches, HIP events): %.4f ms" % float(np.median([run["choice_kernel_ms"] for run in c5["on"]])))
    lines.append("(b) explorative sweep, M C2-sized members (20 vehicles, Hp 8, n_perm %d, seeds 1..M), %d lock-steps timed after %d: pdmpc_sweep_explore_run against" % (SWEEP_PERM, TIMED, WARMUP))
    lines.append("    the parent's pdmpc_controller_explore_run(1) of every member one after the other; median ms per lock-step -> steps/s per member")
    for M in MS:
        b = [run[str(M)]["median"] for run in sw["parent"]]
        s = [run[str(M)]["median"] for run in sw["sweep"]]
        mb, ms_ = float(np.median(b)), float(np.median(s))
        lines.append("    M=%d  parent %7.3f ms (spread %.3f) = %6.1f steps/s per member   sweep %7.3f ms (spread %.3f) = %6.1f steps/s per member   ratio %.2f   choice kernels %.4f ms" % (
            M, mb, max(b) - min(b), 1e3 / mb, ms_, max(s) - min(s), 1e3 / ms_, mb / ms_, float(np.median([run[str(M)]["choice_kernel_ms"] for run in sw["sweep"]]))))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
