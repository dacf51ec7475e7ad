"""What a step over a group costs by the way its results come back, on logical ranks that share one GPU.

Two batches, each planned over 4 logical ranks (PDMPC_COLLECTIVE_COPY, whole components dealt out):
  (a) C5's shape: 20 vehicles x 64 prioritizations, Hp 8 (one explorative step of bench.py's config C5);
  (b) a sweep's shape: 16 members of 20 vehicles (seeds 1 .. 16), 4 prioritizations each, Hp 8, their batches and choices concatenated.
Three ways, on the same marshalled inputs, each ending with the chosen prioritization per graph and the kept records on the host:
  (i)   pdmpc_group_plan_step: every record to every rank and to the host, the choice on the host (all the parent commit could do);
  (ii)  pdmpc_group_plan_step_lean + the choice on the host (pdmpc_choose_host) + pdmpc_group_fetch_records_at;
  (iii) pdmpc_group_plan_step_chosen: entries exchanged, the choice on every rank, the picks gathered by their holders.
Per way: host wall time per step (the calls end with the host's wait), pdmpc_group_last_timing's parts of the planning call, and the
three byte counts of pdmpc_group_last_exchange summed over the way's calls.  `--rounds` rounds (default 5) in which the ways alternate,
`--steps` timed steps per way and round after a warm-up; the median over the rounds' medians and their spread (max - min) are written.
Logical ranks share the GPU's CUs: no speed-up over one launch is expected, only the difference between the ways.

    python tools/group_closed_loop_timing.py [--rounds 5] [--steps 10] [--out profiles/group_closed_loop_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd")]

WORLD, HP = 4, 8


def explorative_batch(options, mpa, handle, seed, n_perm):
    """an explorative batch after three closed-loop steps of the scenario, with its choice: graph = weakly connected sub-graph,
    candidates = prioritizations, cell = the instance's slots of the graph's vehicles, one pick per vehicle"""
    from pdmpc.controller import PrioritizedSequentialController
    from pdmpc.distributed import weak_components
    from pdmpc.explorative import build_exploration_batch
    from pdmpc.iteration_data import info_from_record
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    sc = commonroad_scenario(options, seed=seed)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))

    def plan(prob):
        recs = handle.plan_step(prob["iters"], prob["preds"], [f or [] for f in prob["fallback"]])
        return [info_from_record(recs[i], options.Hp) for i in range(len(recs))]

    for _ in range(3):
        ctl.step(plan_step=plan)
    b = build_exploration_batch(ctl, n_perm, seed=ctl.k + 1)
    adj = b["graph_coupling"]
    n = adj.shape[0]
    labels = weak_components([[j for j in range(n) if adj[i, j] or adj[j, i]] for i in range(n)])
    graphs = sorted(set(labels))
    slot = {(p, v): s for s, (p, v) in enumerate(zip(b["instance"], b["vehicle"]))}
    cells = [[slot[(p, v)] for v in range(n) if labels[v] == g] for g in graphs for p in range(n_perm)]
    picks = [(graphs.index(labels[v]), [slot[(p, v)] for p in range(n_perm)]) for v in range(n)]
    return {"iters": b["iters"], "preds": b["preds"], "fb": [f or [] for f in b["fallback"]], "cells": cells, "graphs": [n_perm] * len(graphs), "picks": picks}


def concatenated(batches):
    out = {"iters": [], "preds": [], "fb": [], "cells": [], "graphs": [], "picks": []}
    graph_cells, stray = [], []
    for b in batches:
        first, first_graph = len(out["iters"]), len(out["graphs"])
        out["iters"] += b["iters"]
        out["fb"] += b["fb"]
        out["preds"] += [[first + q for q in pr] for pr in b["preds"]]
        graph_cells += [[first + s for s in cell] for cell in b["cells"]]
        out["graphs"] += b["graphs"]
        out["picks"] += [(first_graph + g, [first + s for s in sl]) for g, sl in b["picks"]]
    out["cells"] = graph_cells + stray
    return out


class Ways:
    """the three ways on one batch, its inputs marshalled once"""

    def __init__(self, group, batch):
        import numpy as np
        from pdmpc import abi, backend

        self.np, self.abi, self.g, self.L = np, abi, group, group.L
        self.n = len(batch["iters"])
        arr, off, idx, fb, keep = backend._step_args(HP, batch["iters"], batch["preds"], batch["fb"])
        self.keep = (arr, off, idx, fb, keep)
        self.step = (group.g, self.n, arr, abi.i32p(off), abi.i32p(idx), fb, None, backend.SHARD_COMPONENTS)
        self.choice = backend.Choice(batch["cells"], batch["graphs"], batch["picks"])
        self.ch = self.choice.struct()
        self.chosen, self.cost, self.picks = self.choice.outputs()
        self.out = abi.out_array(self.n)
        self.status, self.final = np.zeros(self.n, dtype=np.int32), np.zeros(self.n)
        self.want = np.zeros(max(self.choice.n_picks, 1), dtype=np.int32)
        self.parts, self.bytes = None, None

    def ok(self, rc, what):
        if rc != 0:
            raise SystemExit("%s failed with status %d: %s; nothing more is started" % (what, rc, (self.L.pdmpc_last_error() or b"").decode()))

    def account(self, first=True):
        x = self.g.last_exchange()
        if first:
            self.parts, self.bytes = self.g.timing(), dict(x)
        else:
            for k in x:
                self.bytes[k] += x[k]

    def pick_slots(self):
        c = self.choice
        for i in range(c.n_picks):
            g = int(c.pick_graph[i])
            self.want[i] = c.pick_slot[c.pick_offset[i] + (0 if g < 0 else self.chosen[g])]

    def choose_on_host(self):
        abi, L = self.abi, self.L
        self.ok(L.pdmpc_choose_host(self.n, abi.i32p(self.status), abi.dp(self.final), C.byref(self.ch), abi.i32p(self.chosen), abi.dp(self.cost)), "pdmpc_choose_host")
        self.pick_slots()

    def records(self):
        abi = self.abi
        self.ok(self.L.pdmpc_group_plan_step(*self.step, abi.out_ptr(self.out)), "pdmpc_group_plan_step")
        self.account()
        self.status[:] = self.out["status"]
        self.final[:] = self.out["path_nodes"][:, HP, 4]
        self.choose_on_host()
        self.picks[: self.choice.n_picks] = self.out[self.want[: self.choice.n_picks]]

    def lean(self):
        abi = self.abi
        self.ok(self.L.pdmpc_group_plan_step_lean(*self.step, abi.i32p(self.status), abi.dp(self.final)), "pdmpc_group_plan_step_lean")
        self.account()
        self.choose_on_host()
        self.ok(self.L.pdmpc_group_fetch_records_at(self.g.g, self.choice.n_picks, abi.i32p(self.want), abi.out_ptr(self.picks)), "pdmpc_group_fetch_records_at")
        self.account(False)

    def chosen_on_device(self):
        abi = self.abi
        rc = self.L.pdmpc_group_plan_step_chosen(*self.step, C.byref(self.ch), abi.i32p(self.chosen), abi.dp(self.cost), abi.out_ptr(self.picks))
        self.ok(rc, "pdmpc_group_plan_step_chosen")
        self.account()

    def result(self):
        return self.chosen.tobytes() + self.cost.view(self.np.uint64).tobytes() + self.picks[: self.choice.n_picks].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_closed_loop_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    from pdmpc import abi, backend
    from pdmpc.config import Config, ScenarioType
    from pdmpc.mpa import get_mpa

    options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=HP, max_vehicles=1280, max_nodes=1 << 15)
    mpa = get_mpa(options)
    single = backend.Handle(options)
    single.upload_mpa(mpa)
    shapes = [
        ("(a) C5's shape: 20 vehicles x 64 prioritizations", explorative_batch(options, mpa, single, 1, 64)),
        ("(b) a sweep's shape: 16 members x 20 vehicles x 4 prioritizations", concatenated([explorative_batch(options, mpa, single, s, 4) for s in range(1, 17)])),
    ]
    single.close()
    print("batches built", flush=True)
    group = backend.Group(options, n_devices=WORLD, devices=[0] * WORLD, collective=backend.COLLECTIVE_COPY)
    group.upload_mpa(mpa)
    rec = abi.VEHICLE_OUT_DTYPE.itemsize
    lines = ["%d logical ranks on one GPU, collective: %s (event-ordered peer copies); Hp %d; sizeof(pdmpc_vehicle_out) = %d; whole components dealt out" % (WORLD, group.collective, HP, rec),
             "host wall ms per step: median over %d rounds' medians of %d steps (spread = max - min of the rounds' medians); the ways alternate within a round" % (args.rounds, args.steps),
             "parts: pdmpc_group_last_timing of the planning call; bytes: pdmpc_group_last_exchange summed over the way's calls (per rank into collectives / to the host / host waits)"]
    for title, batch in shapes:
        w = Ways(group, batch)
        ways = [("(i)   plan_step, choice on the host   ", w.records), ("(ii)  plan_step_lean + fetch_records_at", w.lean), ("(iii) plan_step_chosen                ", w.chosen_on_device)]
        results = []
        for _, call in ways:  # warm-up of every way, and the three end with the same bytes
            for _ in range(3):
                call()
            results.append(w.result())
        same = results[0] == results[1] == results[2]
        print("%s: warmed up, same bytes: %s" % (title, same), flush=True)
        med = {name: [] for name, _ in ways}
        seen = {}
        for _ in range(args.rounds):
            for name, call in ways:
                ms = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    call()
                    ms.append(1e3 * (time.perf_counter() - t0))
                med[name].append(float(np.median(ms)))
                seen[name] = (dict(w.parts), dict(w.bytes))
            print("round done", flush=True)
        lines.append("%s: %d plans, %d graphs, %d cells, %d picks; the three ways return the same bytes: %s" % (title, w.n, w.choice.n_graphs, w.choice.n_cells, w.choice.n_picks, "yes" if same else "NO"))
        for name, _ in ways:
            parts, x = seen[name]
            lines.append("    %s %8.3f ms (spread %.3f)   parts: %s   bytes: %d / %d / %d waits" % (
                name, float(np.median(med[name])), max(med[name]) - min(med[name]), "  ".join("%s %.3f" % kv for kv in parts.items()), x["collective_bytes"], x["host_bytes"], x["host_waits"]))
        if not same:
            raise SystemExit("\n".join(lines))
    group.close()
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
