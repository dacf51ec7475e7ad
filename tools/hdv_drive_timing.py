"""Timing of the HDV drivers' step on the device (the driver model and the six-launch call).

M groups of 2 HDVs and 20 CAVs at Hp 8 on the lab map (the size of tools/hdv_grouped_timing.py: the CAVs where the C2 scenario of seed 1
starts them; the HDVs 0.7 m and 2.9 m along loop 9, each call with exactly the room its result needs):
  traffic    ONE pdmpc_hdv_traffic_grouped of the M groups at the poses the HDVs stand at (five launches): what a step cost before
  combined   ONE pdmpc_hdv_drive_traffic_grouped in which every group drives (six launches): the drive pass, then the same five
and the drive pass on its own (pdmpc_hdv_drive_grouped, one launch) at 2 groups of 64 HDVs and 21 CAVs: 128 HDVs with 84 others each.
The variants alternate inside the loop after a warm-up; one invocation is one session, its result one block of lines appended to --out:
medians with their ranges (min .. max), wall and kernel time (HIP events, pdmpc_hdv_kernel_ms).  Every timed result is checked against
the host twins first, bit for bit.

and ms6[0] of a sweep's lock-step with 4 members whose HDVs have drivers (sweep_lock_steps).

    python tools/hdv_drive_timing.py [--groups 4] [--reps 200] [--out profiles/hdv_drive_timing.txt]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd")]

import numpy as np  # noqa: E402


def same_traffic(a, b):
    return (a["closest"] == b["closest"] and a["row_hdv"] == b["row_hdv"] and np.array_equal(a["adjacency"], b["adjacency"]) and np.array_equal(a["set_offset"], b["set_offset"])
            and np.array_equal(a["flags"], b["flags"]) and all(p.tobytes() == q.tobytes() for ra, rb in zip(a["sets"], b["sets"]) for p, q in zip(ra, rb)))


def same_drive(a, b):
    return a["states"] == b["states"] and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("x", "y", "cos_yaw", "sin_yaw", "speed", "gap"))


def sweep_lock_steps(a):
    """ms6[0] (the build part of pdmpc_sweep_last_timing: step preparation with the traffic stage) of a sweep's lock-step with 4 members of
    4 CAVs and 2 driven HDVs each on the lab map's loop 2 at Hp 6, against the same sweep with HDVs that stand (set_hdv_measurements once):
    medians with ranges over --sweep-steps lock-steps after 5"""
    from pdmpc import hdv
    from pdmpc.backend import Handle
    from pdmpc.config import Config, MpaType, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.native_controller import NativeController, NativeSweep
    from pdmpc.road_network import commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=4, Hp=6, mpa_type=MpaType.single_speed, path_ids=[9, 10, 12, 13], manual_control=2, max_nodes=1 << 16,
                     max_vehicles=64)
    hdv_mpa = get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=6, mpa_type=MpaType.single_speed, recursive_feasibility=False))
    route = hdv.route_from_loop(9)
    out = {}
    for kind in ("driven", "standing"):
        handle = Handle(options)
        handle.upload_mpa(get_mpa(options))
        members = []
        for m in range(4):
            sc = commonroad_scenario(options, seed=1)
            c = NativeController(options, sc, get_mpa(options), handle, coupling="distance")
            hmap = hdv.scenario_hdv_map(sc)
            c.set_hdvs(hdv_mpa, hmap.successors, hmap.relationship)
            starts = [0.7 + 0.1 * m, 2.9 + 0.1 * m]
            if kind == "driven":
                c.set_hdv_drivers([route, route], starts, [0.5, 0.5])
            else:
                poses = [hdv.state_pose(hmap, route[0], route[1], hdv.place(hmap, route[0], route[1], d)) for d in starts]
                c.set_hdv_measurements([p[0] for p in poses], [p[1] for p in poses], [math.atan2(p[3], p[2]) for p in poses])
            members.append(c)
        sweep = NativeSweep(members, handle)
        ms = []
        for step in range(5 + a.sweep_steps):
            sweep.step()
            if step >= 5:
                ms.append(sweep.last_timing()["build"])
                assert sweep.last_hdv_calls() == (1, 0)
        out[kind] = ms
        sweep.close()
        for c in members:
            c.close()
        handle.close()
    q = lambda v: "median %.4f  range %.4f .. %.4f" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    return ["ms6[0] of a sweep's lock-step, 4 members of 4 CAVs / 2 HDVs / Hp 6, %d lock-steps after 5, ms" % a.sweep_steps,
            "  HDVs with drivers (ONE six-launch call)    " + q(out["driven"]), "  HDVs that stand (ONE five-launch call)     " + q(out["standing"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sweep-steps", type=int, default=40)
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
    sets = R.local_reachable_sets_conv(get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=Hp, mpa_type=MpaType.single_speed, recursive_feasibility=False)))
    zero = (0.0, 0.0)
    route = hdv.route_from_loop(9)
    states = [hdv.place(lab, route[0], route[1], d) for d in (0.7, 2.9)]
    poses = [hdv.state_pose(lab, route[0], route[1], s) for s in states]
    cav_x, cav_y = [v.x_start for v in sc.vehicles], [v.y_start for v in sc.vehicles]
    cav_lanelet = [int(v.lanelets_index[0]) for v in sc.vehicles]
    group = dict(slot=0, routes=[route, route], states=states, tiles=[zero, zero], v_des=[0.5, 0.5], cav_x=cav_x, cav_y=cav_y, cav_tile=[zero] * n, drives=True, trim=[1, 1],
                 cav_lanelet=cav_lanelet)
    plain = (0, [p[0] for p in poses], [p[1] for p in poses], [math.atan2(p[3], p[2]) for p in poses], [1, 1], [zero, zero], cav_x, cav_y, cav_lanelet, [zero] * n)
    handle = Handle(options)
    handle.upload_hdv_map(lab, sets)
    # the references: the host twins, for one group
    driven = hdv.drive_native(lab, group["routes"], states, group["tiles"], group["v_des"], cav_x, cav_y, group["cav_tile"])
    after = hdv.hdv_traffic_native(lab, sets, driven["x"], driven["y"], [0.0, 0.0], [1, 1], [zero, zero], cav_x, cav_y, cav_lanelet, [zero] * n,
                                   cos_sin=(driven["cos_yaw"], driven["sin_yaw"]))
    before = hdv.hdv_traffic_native(lab, sets, *plain[1:])
    cap_after, cap_before = M * int(after["set_offset"][-1]), M * int(before["set_offset"][-1])
    assert all(same_drive(d, driven) and same_traffic(t, after) for d, t in hdv.drive_traffic_grouped_native(handle, [group] * M, capacity=cap_after)), "combined = host twins"
    assert all(same_traffic(t, before) for t in handle.hdv_traffic_grouped([plain] * M, capacity=cap_before)), "traffic = host twin"
    # 2 groups of 64 HDVs 0.45 m apart round the longest loop and 21 CAVs: 63 + 21 = 84 others for every HDV
    long_route = hdv.route_from_loop(54)
    many = [hdv.place(lab, long_route[0], long_route[1], 0.45 * q) for q in range(64)]
    cx = [hdv.state_pose(lab, long_route[0], long_route[1], hdv.place(lab, long_route[0], long_route[1], 1.5 * q + 0.2))[:2] for q in range(21)]
    big = dict(slot=0, routes=[long_route] * 64, states=many, tiles=[zero] * 64, v_des=[0.5] * 64, cav_x=[p[0] for p in cx], cav_y=[p[1] for p in cx], cav_tile=[zero] * 21)
    big_ref = hdv.drive_native(lab, big["routes"], many, big["tiles"], big["v_des"], big["cav_x"], big["cav_y"], big["cav_tile"])
    assert all(same_drive(d, big_ref) for d in hdv.drive_grouped_native(handle, [big, big])), "drive = host twin"

    q = lambda v: "median %.4f  range %.4f .. %.4f" % (np.median(v), np.min(v), np.max(v))  # noqa: E731
    t_wall, t_kernel, c_wall, c_kernel, d_wall, d_kernel = [], [], [], [], [], []
    for rep in range(a.warmup + a.reps):
        keep = rep >= a.warmup
        for call, wall, kernel in ((lambda ms: handle.hdv_traffic_grouped([plain] * M, capacity=cap_before, call_ms=ms), t_wall, t_kernel),
                                   (lambda ms: hdv.drive_traffic_grouped_native(handle, [group] * M, capacity=cap_after, call_ms=ms), c_wall, c_kernel),
                                   (lambda ms: hdv.drive_grouped_native(handle, [big, big], call_ms=ms), d_wall, d_kernel)):
            ms = []
            call(ms)
            if keep:
                wall.append(ms[0])
                kernel.append(handle.hdv_kernel_ms())
    handle.close()
    lo, hi = np.min(t_kernel), np.max(t_kernel)
    med = np.median(c_kernel)
    where = "inside" if lo <= med <= hi else "%.4f ms %s" % ((med - hi) if med > hi else (lo - med), "above" if med > hi else "below")
    lines = ["HDV drivers on the device, %d groups of 2 HDVs / 20 CAVs / Hp 8 on one map; %d calls each after %d, alternating, ms" % (M, a.reps, a.warmup),
             "  traffic call, kernel time (5 launches)     " + q(t_kernel), "  combined call, kernel time (6 launches)    " + q(c_kernel),
             "  traffic call (wall)                        " + q(t_wall), "  combined call (wall)                       " + q(c_wall),
             "  the sixth launch (difference of the kernel medians)   %.4f" % (med - np.median(t_kernel)),
             "  the combined call's kernel median against the range of the traffic call's runs of this session: " + where,
             "drive pass alone, 2 groups of 64 HDVs / 21 CAVs (128 HDVs, 84 others each), ms",
             "  kernel time (1 launch)                     " + q(d_kernel), "  call (wall)                                " + q(d_wall)]
    lines += sweep_lock_steps(a)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
