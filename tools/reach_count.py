#!/usr/bin/env python3
"""How many obstacle segments an edge check walks, and how many of them are in reach of its step (CPU only: the oracle's closed loop
and the host twins of the graph search's reach lists; include/pdmpc_reach.h): by the square of the disc bound
around the root (pdmpc_reach_lists_host) and by the automaton's reach rectangle in the root's frame, the rule the kernel's lists follow
(pdmpc_reach_lists_oriented_host).

Default: the C2 world of bench.py (20 vehicles, Hp 8, seed 1), closed-loop steps 21-40, predecessors' slots filled with their solved
areas (fallback areas for an exhausted predecessor).  "walks" counts what a check item loop of the kernel iterates over without the
lists: every soup column but the last of a step's vehicle soup (8-column slots per predecessor, NaN separators) and of the boundary.

usage: tools/reach_count.py [--vehicles N] [--hp H] [--seed S] [--first 21] [--last 40]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd")]

from oracle import oracle  # noqa: E402
from pdmpc import abi, backend  # noqa: E402
from pdmpc.config import Config, MpaType, ScenarioType  # noqa: E402
from pdmpc.controller import PrioritizedSequentialController  # noqa: E402
from pdmpc.iteration_data import info_from_record  # noqa: E402
from pdmpc.mpa import get_mpa  # noqa: E402
from pdmpc.road_network import boundary_provider, commonroad_scenario  # noqa: E402

VMAX = abi.VMAX
NAN = float("nan")
DP, IP = abi.c_double_p, abi.c_int32_p


def soup(polys, slots=()):
    """[polygon, NaN] ..., then one VMAX-column slot per predecessor area (NaN beyond its columns), as the kernel lays a step out."""
    xs, ys = [], []
    for p in polys:
        p = np.asarray(p, dtype=np.float64)
        xs += p[0].tolist() + [NAN]
        ys += p[1].tolist() + [NAN]
    for p in slots:
        cols = 0 if p is None else min(np.asarray(p).shape[1], VMAX)
        xs += ([] if p is None else np.asarray(p, dtype=np.float64)[0, :cols].tolist()) + [NAN] * (VMAX - cols)
        ys += ([] if p is None else np.asarray(p, dtype=np.float64)[1, :cols].tolist()) + [NAN] * (VMAX - cols)
    return np.array(xs, dtype=np.float64), np.array(ys, dtype=np.float64)


def in_reach(L, Hp, dmax, amax, rx, ry, x, y, only=None, oriented=None):
    """Segments in reach per step (all columns for every step, or for step `only` alone); oriented = (rectangles, root trim, root yaw):
    by the oriented rule."""
    if len(x) < 2:
        return [0] * Hp
    first = np.zeros(Hp, dtype=np.int32)
    count = np.array([len(x) if only in (None, k) else 0 for k in range(1, Hp + 1)], dtype=np.int32)
    lo = np.zeros(Hp + 1, dtype=np.int32)
    lst = np.zeros(max(int(count.sum()), 1), dtype=np.int32)
    if oriented is not None:
        rects, trim, yaw = oriented
        rc = L.pdmpc_reach_lists_oriented_host(Hp, rects.shape[0], rects.ctypes.data_as(DP), trim, rx, ry, yaw, x.ctypes.data_as(DP), y.ctypes.data_as(DP), first.ctypes.data_as(IP),
                                               count.ctypes.data_as(IP), lo.ctypes.data_as(IP), lst.ctypes.data_as(IP))
        assert rc == 0
        return np.diff(lo).tolist()
    rc = L.pdmpc_reach_lists_host(Hp, dmax, amax, rx, ry, x.ctypes.data_as(DP), y.ctypes.data_as(DP), first.ctypes.data_as(IP), count.ctypes.data_as(IP), lo.ctypes.data_as(IP),
                                  lst.ctypes.data_as(IP))
    assert rc == 0
    return np.diff(lo).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=20)
    ap.add_argument("--hp", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--first", type=int, default=21)
    ap.add_argument("--last", type=int, default=40)
    args = ap.parse_args()
    Hp = args.hp
    options = Config(scenario_type=ScenarioType.commonroad, amount=args.vehicles, Hp=Hp, mpa_type=MpaType.single_speed, max_vehicles=max(32, args.vehicles), max_nodes=1 << 30)
    mpa = get_mpa(options)
    L = backend.load_library()
    s, keep = abi.pack_mpa(mpa)
    d, a = C.c_double(), C.c_double()
    assert L.pdmpc_mpa_reach_host(C.byref(s), C.byref(d), C.byref(a)) == 0
    dmax, amax = d.value, a.value
    print("automaton: Dmax %.4f m, Amax %.4f m" % (dmax, amax))
    rects = np.zeros((mpa.n_trims, Hp, 4))
    assert L.pdmpc_mpa_reach_rects_host(C.byref(s), Hp, rects.ctypes.data_as(DP)) == 0
    print("first trim, step %d: x in [%.3f, %.3f], y in [%.3f, %.3f] m: %.2f m^2 against the square's %.2f m^2" % (
        Hp, *rects[0, Hp - 1], (rects[0, Hp - 1, 1] - rects[0, Hp - 1, 0]) * (rects[0, Hp - 1, 3] - rects[0, Hp - 1, 2]), (2 * ((Hp - 1) * dmax + amax)) ** 2))
    sc = commonroad_scenario(options, seed=args.seed, tiles=1)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc), priority_strategy="constant")
    rows = []  # (k, predecessors, vehicle soup walked, in reach, boundary walked, in reach, vehicle soup / boundary in reach by the oriented rule)
    step = [0]

    def plan_step(prob):
        recs, _, _ = oracle.plan_step_native(options, mpa, prob, n_threads=min(8, os.cpu_count() or 1))
        step[0] += 1
        if args.first <= step[0] <= args.last:
            for v, it in enumerate(prob["iters"]):
                rx, ry = float(it.x0[0]), float(it.x0[1])
                left, right = it.predicted_lanelet_boundary
                bx, by = soup([b for b in (left, right) if b is not None and np.size(b)])
                b_in = in_reach(L, Hp, dmax, amax, rx, ry, bx, by)
                how = (rects, int(it.trim_index), float(it.x0[2]))
                b_or = in_reach(L, Hp, dmax, amax, rx, ry, bx, by, oriented=how)
                for k in range(1, Hp + 1):
                    slots = []
                    for p in prob["preds"][v]:
                        if int(recs[p]["status"]) == 0:
                            slots.append(np.array(recs[p]["shapes"][k - 1][:, : int(recs[p]["shape_cols"][k - 1])]))
                        else:
                            fb = prob["fallback"][p]
                            slots.append(np.asarray(fb[k - 1], dtype=np.float64) if fb is not None and len(fb) else None)
                    vx, vy = soup(list(it.obstacles) + [dd[k - 1] for dd in it.dynamic_obstacle_area], slots)
                    v_in = in_reach(L, Hp, dmax, amax, rx, ry, vx, vy, only=k)[k - 1]
                    v_or = in_reach(L, Hp, dmax, amax, rx, ry, vx, vy, only=k, oriented=how)[k - 1]
                    rows.append((k, len(prob["preds"][v]), max(len(vx) - 1, 0), v_in, max(len(bx) - 1, 0), b_in[k - 1], v_or, b_or[k - 1]))
        return [info_from_record(recs[i], Hp) for i in range(len(recs))]

    for _ in range(args.last):
        ctl.step(plan_step=plan_step)
    del keep
    st = np.array(rows, dtype=float)
    print("%d (vehicle, step k) soups of closed-loop steps %d-%d" % (len(st), args.first, args.last))
    print("| | segments a check item loop walks | of them in reach of the square | in reach of the rectangle in the root's frame (the lists) |")
    print("|---|---|---|---|")

    def line(label, q):
        print("| %s | %.1f (vehicle soup %.1f, boundary %.1f) | %.1f (%.1f / %.1f) | %.1f (%.1f / %.1f) |" % (label, (q[:, 2] + q[:, 4]).mean(), q[:, 2].mean(), q[:, 4].mean(), (q[:, 3] + q[:, 5]).mean(),
                                                                                                          q[:, 3].mean(), q[:, 5].mean(), (q[:, 6] + q[:, 7]).mean(), q[:, 6].mean(), q[:, 7].mean()))

    line("all (mean)", st)
    for k in range(1, Hp + 1):
        line("k = %d" % k, st[st[:, 0] == k])
    for lo, hi in ((0, 0), (1, 5), (6, 12), (13, 10 ** 6)):
        q = st[(st[:, 1] >= lo) & (st[:, 1] <= hi)]
        if len(q):
            line("%s predecessors (walked: up to %d)" % ("%d-%d" % (lo, min(hi, int(st[:, 1].max()))) if hi else "0", int((q[:, 2] + q[:, 4]).max())), q)
    tot, act, lists = (st[:, 2] + st[:, 4]).sum(), (st[:, 3] + st[:, 5]).sum(), (st[:, 6] + st[:, 7]).sum()
    print("segment tests that cannot produce a hit: %.1f %% by the square, %.1f %% by the rectangle (%.1f %% of the square's)" % (100.0 * (1.0 - act / tot), 100.0 * (1.0 - lists / tot), 100.0 * (1.0 - lists / act)))


if __name__ == "__main__":
    main()
