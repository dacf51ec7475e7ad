"""Timing of the grouped HDV traffic call against the ungrouped calls it replaces.

M groups of 2 HDVs and 20 CAVs at Hp 8 on the lab map (the size of tools/hdv_timing.py: the CAVs where the C2 scenario of seed 1 starts
them, one HDV on the fork of lanelet 3, one on the point with 8 closest lanelets), each call with exactly the room its result needs:
  grouped    ONE pdmpc_hdv_traffic_grouped of M groups that share map slot 0 (wall: staging, five launches, read-back, the copies into
             the caller's arrays), and its kernel time (HIP events, pdmpc_hdv_kernel_ms)
  ungrouped  M pdmpc_hdv_traffic calls of the same groups, one after the other (wall of all M, and the sum of their kernel times)
  upload     one pdmpc_upload_hdv_map of the lab map: what a member that found another member's map on the handle paid per step
and, with --pack, one group of 64 HDVs at Hp --pack-hp through both calls (--pack-only: nothing else, for a kernel trace that compares
the scan and copy passes with pdmpc_hdv_pack_kernel).  The variants alternate inside the loop after a warm-up; one invocation is one session, its result one block of
lines appended to --out.  Every timed result is checked against the host twin first, bit for bit.

    python tools/hdv_grouped_timing.py [--groups 4] [--reps 200] [--pack] [--out profiles/hdv_grouped_timing.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd")]

import numpy as np  # noqa: E402


def same(a, b):
    return (a["closest"] == b["closest"] and a["row_hdv"] == b["row_hdv"] and np.array_equal(a["adjacency"], b["adjacency"]) and np.array_equal(a["set_offset"], b["set_offset"])
            and np.array_equal(a["flags"], b["flags"]) and all(p.tobytes() == q.tobytes() for ra, rb in zip(a["sets"], b["sets"]) for p, q in zip(ra, rb)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pack", action="store_true")
    ap.add_argument("--pack-hp", type=int, default=1, help="Hp of the one group of 64 HDVs (16 x Hp slots per HDV)")
    ap.add_argument("--pack-only", action="store_true", help="only the one group of 64 HDVs: for a kernel trace of the packing passes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from pdmpc import hdv
    from pdmpc import reachability as R
    from pdmpc.backend import Handle
    from pdmpc.config import Config, MpaType, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.road_network import commonroad_scenario

    n, Hp, M = 20, 8, a.groups
    options = Config(scenario_type=ScenarioType.commonroad, amount=n, Hp=Hp, max_vehicles=32)
    sc = commonroad_scenario(options, seed=1)
    lab = hdv.lab_hdv_map()
    hdv_sets = lambda hp: R.local_reachable_sets_conv(get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=hp, mpa_type=MpaType.single_speed, recursive_feasibility=False)))  # noqa: E731
    sets = hdv_sets(Hp)

    def on(lanelet, q):  # centre point q of a lanelet, heading along the centre line
        c = lab.centre[lanelet - 1]
        b = min(q + 1, c.shape[0] - 1)
        return float(c[q, 0]), float(c[q, 1]), math.atan2(c[b, 1] - c[b - 1, 1], c[b, 0] - c[b - 1, 0])

    poses = [on(3, 3), on(17, 10)]
    zero = (0.0, 0.0)
    cavs = ([v.x_start for v in sc.vehicles], [v.y_start for v in sc.vehicles], [int(v.lanelets_index[0]) for v in sc.vehicles], [zero] * n)
    args = ([p[0] for p in poses], [p[1] for p in poses], [p[2] for p in poses], [1, 1], [zero, zero]) + cavs
    handle = Handle(options)
    handle.upload_hdv_map(lab, sets)
    host = hdv.hdv_traffic_native(lab, sets, *args)
    total = int(host["set_offset"][-1])
    groups = [(0,) + args] * M
    assert all(same(r, host) for r in handle.hdv_traffic_grouped(groups, capacity=M * total)), "grouped = host twin, bit for bit"
    assert same(handle.hdv_traffic(*args, capacity=total), host), "ungrouped = host twin, bit for bit"
    q = lambda v: "median %.4f  min %.4f  p90 %.4f" % (np.median(v), np.min(v), np.percentile(v, 90))  # noqa: E731
    grouped, grouped_kernel, ungrouped, ungrouped_kernel, upload = [], [], [], [], []
    for rep in range(0 if a.pack_only else a.warmup + a.reps):
        keep = rep >= a.warmup
        ms = []
        handle.hdv_traffic_grouped(groups, capacity=M * total, call_ms=ms)
        if keep:
            grouped.append(ms[0])
            grouped_kernel.append(handle.hdv_kernel_ms())
        ms, kernel = [], 0.0
        for _ in range(M):
            handle.hdv_traffic(*args, capacity=total, call_ms=ms)
            kernel += handle.hdv_kernel_ms()
        if keep:
            ungrouped.append(sum(ms))
            ungrouped_kernel.append(kernel)
        t0 = time.perf_counter()
        handle.upload_hdv_map(lab, sets)
        if keep:
            upload.append(1e3 * (time.perf_counter() - t0))
    lines = [] if a.pack_only else ["grouped HDV traffic call, %d groups of 2 HDVs / 20 CAVs / Hp 8 on one map (%d vertices each); %d calls each after %d, ms" % (M, total, a.reps, a.warmup),
             "  grouped call (wall)                    " + q(grouped), "  %d ungrouped calls (wall, summed)       " % M + q(ungrouped),
             "  grouped kernel time (5 launches)       " + q(grouped_kernel), "  ungrouped kernel time (%2d launches)     " % (4 * M) + q(ungrouped_kernel),
             "  one map upload (wall, incl. Python)    " + q(upload),
             "  grouped / ungrouped (medians)          %.3f" % (np.median(grouped) / np.median(ungrouped))]
    if a.pack or a.pack_only:  # one group of 64 HDVs: 1024 x Hp slots through the scan + copy passes and through pdmpc_hdv_pack_kernel
        one = hdv_sets(a.pack_hp)
        handle.upload_hdv_map(lab, one)
        big = ([poses[i % 2][0] for i in range(64)], [poses[i % 2][1] for i in range(64)], [poses[i % 2][2] for i in range(64)], [1] * 64, [zero] * 64, [], [], [], [])
        ref = handle.hdv_traffic(*big)
        big_total = int(ref["set_offset"][-1])
        assert same(handle.hdv_traffic_grouped([(0,) + big], capacity=big_total)[0], ref)
        gk, uk = [], []
        for rep in range(a.warmup + a.reps):
            handle.hdv_traffic_grouped([(0,) + big], capacity=big_total)
            gk.append(handle.hdv_kernel_ms())
            handle.hdv_traffic(*big, capacity=big_total)
            uk.append(handle.hdv_kernel_ms())
        lines += ["one group of 64 HDVs at Hp %d (%d slots, %d vertices), kernel time of the whole call, ms" % (a.pack_hp, 1024 * a.pack_hp, big_total),
                  "  grouped (scan + copy)                  " + q(gk[a.warmup:]), "  ungrouped (pdmpc_hdv_pack_kernel)      " + q(uk[a.warmup:])]
    handle.close()
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
