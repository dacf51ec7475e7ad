"""Timing of the sweep (pdmpc_sweep_run): M closed loops in lock-step against the same M loops stepped one after
another by the parent commit's library.

Workload: M in {1, 2, 4, 8} C2-like members (20 vehicles, Hp 8, seeds 1 .. M) on one handle, steps 21-40 of each closed loop, with
  (a) distance coupling,
  (b) reachable-set coupling with lanelet bounding,
  (c) distance coupling, FCA priorities,
  (d) the optimal-priority step (pdmpc_sweep_optimal_run): M road-network members of 6 vehicles at Hp 6 (seeds 1 .. M, distance coupling,
      max_instances 600), and M circle members of 4 vehicles at Hp 5 (full coupling, K = 24), steps 4-15; the baseline steps every member
      with pdmpc_controller_optimal_run(max_instances, 1).
Sweep: the median wall time per lock-step of pdmpc_sweep_run and the six parts of pdmpc_sweep_last_timing.
Baseline: a built checkout of the parent commit in a directory of its own (--baseline-root: its p-dmpc_amd/pdmpc package and its
p-dmpc_amd/csrc/libpdmpc_hip.so); per lock-step every member takes one pdmpc_controller_run(1), the lock-step's time is their sum.
In (c) the baseline is the parent commit's library stepping the SAME SWEEP: what changes is the collision assessment inside the
lock-step, one grouped call here against one call per member there, so its lock-step and its build part are compared.
Five alternating runs of baseline and sweep, each in a fresh process; reported are the median of the five medians and their spread
(max - min).  For (b) also one grouped device call (pdmpc_bound_reachable_sets on all members' vehicles + pdmpc_bounded_set_coupling_grouped)
against M ungrouped pairs of calls on the members' recorded states, in kernel time (HIP events) and as whole calls.

    python tools/sweep_timing.py --baseline-root DIR [--rounds 5] [--modes a,b,c,d] [--out profiles/sweep_timing.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 2, 4, 8)
MODES = {"a": dict(coupling="distance"), "b": dict(coupling="reachable_set", bound_reachable_sets=True), "c": dict(coupling="distance", priority_strategy="fca")}
TITLES = {"a": "distance coupling", "b": "reachable-set coupling with lanelet bounding", "c": "distance coupling, FCA priorities"}
OPTIMAL = {"road": dict(amount=6, Hp=6, max_instances=600, coupling="distance"), "circle": dict(amount=4, Hp=5, max_instances=24, coupling="full")}  # (d)
OPTIMAL_WARMUP, OPTIMAL_TIMED = 3, 12
SWEEP_BASELINE = ("c",)  # the modes whose baseline is the parent's library stepping the same sweep
PARTS = ("build", "pack", "enqueue", "wait_and_read_back", "choose", "apply")
WARMUP, TIMED = 20, 20


def members_on_one_handle(M, mode):
    import numpy as np  # noqa: F401
    from pdmpc.backend import Handle
    from pdmpc.config import Config, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import commonroad_scenario

    kw = dict(MODES[mode])
    coupling = kw.pop("coupling")
    ctl = {k: kw.pop(k) for k in ("priority_strategy",) if k in kw}
    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=max(32, 20 * M), max_nodes=1 << 17, **kw)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    scs = [commonroad_scenario(options, seed=s) for s in range(1, M + 1)]
    return options, mpa, h, scs, [NativeController(options, sc, mpa, h, coupling=coupling, **ctl) for sc in scs]


def optimal_members(M, which):
    """(d): M optimal-priority members on one handle that holds every member's batch"""
    from pdmpc.backend import Handle
    from pdmpc.config import Config, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.native_controller import NativeController
    from pdmpc.road_network import commonroad_scenario
    from pdmpc.scenario import circle_scenario

    o = OPTIMAL[which]
    road = which == "road"
    options = Config(scenario_type=ScenarioType.commonroad if road else ScenarioType.circle, amount=o["amount"], Hp=o["Hp"],
                     max_vehicles=o["amount"] * o["max_instances"] * M, max_nodes=1 << 12)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    scs = [commonroad_scenario(options, seed=s) if road else circle_scenario(options) for s in range(1, M + 1)]
    return h, [NativeController(options, sc, mpa, h, coupling=o["coupling"]) for sc in scs], o["max_instances"]


def optimal_worker(kind, out):
    """(d) on the tree this process imports: the parent's library steps every member alone, this one's steps the sweep"""
    import numpy as np

    for which in OPTIMAL:
        for M in MS:
            h, cs, K = optimal_members(M, which)
            if kind == "baseline":
                ms = [sum(float(c.optimal_run(K, 1)[0]) for c in cs) for _ in range(OPTIMAL_WARMUP + OPTIMAL_TIMED)][OPTIMAL_WARMUP:]
                out["d%s%d" % (which, M)] = {"median": float(np.median(ms))}
            else:
                from pdmpc.native_controller import NativeSweep

                sweep = NativeSweep(cs, h)
                sweep.optimal_run(K, OPTIMAL_WARMUP)
                ms, parts = [], []
                for _ in range(OPTIMAL_TIMED):
                    ms.append(float(sweep.optimal_run(K, 1)[0]))
                    t = sweep.last_timing()
                    parts.append([t[p] for p in PARTS])
                out["d%s%d" % (which, M)] = {"median": float(np.median(ms)), "parts": [float(x) for x in np.median(np.array(parts), axis=0)]}
                sweep.close()
            for c in cs:
                c.close()
            h.close()


def worker(kind, modes):
    """One run: every mode and M on the tree this process imports -> one JSON line."""
    import numpy as np

    out = {}
    if "d" in modes:
        optimal_worker(kind, out)
    for mode in [m for m in modes if m != "d"]:
        for M in MS:
            options, mpa, h, scs, cs = members_on_one_handle(M, mode)
            if kind == "baseline" and mode not in SWEEP_BASELINE:
                step_ms = []
                for k in range(WARMUP + TIMED):
                    step_ms.append(sum(float(c.run(1)[0]) for c in cs))
                out["%s%d" % (mode, M)] = {"median": float(np.median(step_ms[WARMUP:]))}
            else:
                from pdmpc.native_controller import NativeSweep

                sweep = NativeSweep(cs, h)
                sweep.run(WARMUP)
                ms, parts = [], []
                for k in range(TIMED):
                    ms.append(float(sweep.run(1)[0]))
                    t = sweep.last_timing()
                    parts.append([t[p] for p in PARTS])
                out["%s%d" % (mode, M)] = {"median": float(np.median(ms)), "parts": [float(x) for x in np.median(np.array(parts), axis=0)]}
                sweep.close()
            for c in cs:
                c.close()
            h.close()
    print("RESULT " + json.dumps(out), flush=True)


def grouped_calls(reps):
    """(b): one grouped device call against M ungrouped ones on the members' states after 30 steps -> one JSON line."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bounded_reachable_timing import lanelet_polygons

    out = {}
    for M in MS:
        options, mpa, h, scs, cs = members_on_one_handle(M, "b")
        from pdmpc.native_controller import NativeSweep

        sweep = NativeSweep(cs, h)
        sweep.run(30)
        per = []
        for c, sc in zip(cs, scs):
            st = c.state()
            lan, trim = lanelet_polygons(options, mpa, sc, (st["x"], st["y"], st["yaw"], st["speed"], st["steering"]))
            per.append((st["x"].copy(), st["y"].copy(), st["yaw"].copy(), np.asarray(trim), lan))
        x, y, yaw, trim = (np.concatenate([p[q] for p in per]) for q in range(4))
        lan = [q for p in per for q in p[4]]
        sizes = [len(p[0]) for p in per]
        gk, gc, uk, uc = [], [], [], []
        for r in range(reps + 2):
            t0 = time.perf_counter()
            h.bound_reachable_sets(x, y, yaw, trim, lan, False)
            blocks = h.bounded_set_coupling_grouped(sizes)
            t1 = time.perf_counter()
            k = sum(h.bounded_reachable_kernel_ms())
            tu, ku, alone = 0.0, 0.0, []
            for p in per:
                t2 = time.perf_counter()
                h.bound_reachable_sets(p[0], p[1], p[2], p[3], p[4], False)
                alone.append(h.bounded_set_coupling())
                tu += time.perf_counter() - t2
                ku += sum(h.bounded_reachable_kernel_ms())
            assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) for a, b in zip(blocks, alone))
            if r >= 2:
                gk.append(k)
                gc.append(1e3 * (t1 - t0))
                uk.append(ku)
                uc.append(1e3 * tu)
        out[str(M)] = [float(np.median(v)) for v in (gk, gc, uk, uc)]
        sweep.close()
        for c in cs:
            c.close()
        h.close()
    print("RESULT " + json.dumps(out), flush=True)


def child(root, *args):
    """A fresh process on the tree under `root` (its package and its library) -> the JSON of its RESULT line."""
    env = dict(os.environ, PDMPC_TREE=root)
    env.pop("PDMPC_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("a timing run failed with status %d: nothing more is started" % p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_timing.txt"))
    ap.add_argument("--modes", default=",".join(list(MODES) + ["d"]))
    ap.add_argument("--worker")
    args = ap.parse_args()
    modes = [m for m in list(MODES) + ["d"] if m in args.modes.split(",")]
    if args.worker:
        tree = os.environ.get("PDMPC_TREE", ROOT)
        sys.path[:0] = [tree, os.path.join(tree, "p-dmpc_amd")]
        if args.worker == "grouped":
            grouped_calls(args.reps)
        else:
            worker(args.worker, modes)
        return
    if not args.baseline_root:
        raise SystemExit("--baseline-root: a built checkout of the parent commit is needed")
    import numpy as np

    base, sweep = [], []
    for r in range(args.rounds):
        base.append(child(os.path.abspath(args.baseline_root), "--worker", "baseline", "--modes", ",".join(modes)))
        sweep.append(child(ROOT, "--worker", "sweep", "--modes", ",".join(modes)))
        print("round %d done" % (r + 1), flush=True)
    grouped = child(ROOT, "--worker", "grouped", "--reps", str(args.reps)) if "b" in modes else None
    lines = ["sweep against the parent commit's library: M C2-like members (20 vehicles, Hp 8, seeds 1..M), steps %d-%d, ms per lock-step;"
             % (WARMUP + 1, WARMUP + TIMED),
             "median and spread (max - min) of %d alternating runs' medians; baseline = sum of the members' pdmpc_controller_run(1) unless a block says otherwise" % args.rounds]
    blocks = [(m, "%s%%d" % m, "(%s) %s" % (m, TITLES[m])) for m in modes if m != "d"]
    if "d" in modes:
        lines_d = {"road": "(d) optimal-priority step: road-network members of 6 vehicles, Hp 6, max_instances 600",
                   "circle": "(d) optimal-priority step: circle members of 4 vehicles, Hp 5, K = 24"}
        blocks += [("d", "d%s%%d" % w, lines_d[w] + "; steps %d-%d; baseline = sum of the members' pdmpc_controller_optimal_run(max_instances, 1)"
                    % (OPTIMAL_WARMUP + 1, OPTIMAL_WARMUP + OPTIMAL_TIMED)) for w in OPTIMAL]
    for mode, key_of, title in blocks:
        lines.append(title + ("; baseline = the parent commit's library stepping the same sweep" if mode in SWEEP_BASELINE else ""))
        for M in MS:
            key = key_of % M
            b = [r[key]["median"] for r in base]
            s = [r[key]["median"] for r in sweep]
            mb, ms_, sb, ss = float(np.median(b)), float(np.median(s)), max(b) - min(b), max(s) - min(s)
            spread = max(sb, ss)
            if M == 1:
                verdict = "agree within the spread" if abs(mb - ms_) <= spread else "DIFFER by more than the spread"
            else:
                verdict = "sweep faster by more than the spread" if mb - ms_ > spread else ("sweep faster, within the spread" if ms_ < mb else "sweep NOT faster")
            parts = np.median(np.array([r[key]["parts"] for r in sweep]), axis=0)
            lines.append("  M=%d  baseline %7.3f (spread %.3f)   sweep %7.3f (spread %.3f)   ratio %.2f   %s" % (M, mb, sb, ms_, ss, mb / ms_, verdict))
            lines.append("        sweep parts: " + "  ".join("%s %.3f" % (p, v) for p, v in zip(PARTS, parts)))
            if mode in SWEEP_BASELINE:  # the build part, where the collision assessment runs, by itself
                bb = [r[key]["parts"][0] for r in base]
                sb_ = [r[key]["parts"][0] for r in sweep]
                mbb, msb, spread_b = float(np.median(bb)), float(np.median(sb_)), max(max(bb) - min(bb), max(sb_) - min(sb_))
                lines.append("        build part: baseline %.4f  sweep %.4f  larger spread %.4f   %s"
                             % (mbb, msb, spread_b, "below the baseline by more than the spread" if mbb - msb > spread_b else "NOT below the baseline by more than the spread"))
    if grouped is not None:
        lines.append("(b) step preparation on the members' states after 30 steps, median of %d: one pdmpc_bound_reachable_sets + pdmpc_bounded_set_coupling_grouped"
                     " against M pairs of ungrouped calls" % args.reps)
        for M in MS:
            gk, gc, uk, uc = grouped[str(M)]
            lines.append("  M=%d  kernels (events) grouped %.4f ms, ungrouped %.4f ms   whole calls grouped %.4f ms, ungrouped %.4f ms" % (M, gk, uk, gc, uc))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
