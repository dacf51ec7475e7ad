"""Timing of the HDV traffic call at the size of bench.py's C2 road network: 2 HDVs, 20 CAVs, Hp 8.

The CAVs stand where the C2 scenario (seed 1) starts them; one HDV stands on the fork of lanelet 3, the other on the point of the lab
map with 8 closest lanelets (10 rows, 80 reachable lanes).  Timed over --reps calls after a warm-up, each with exactly the room the
result needs:
  kernel   the four launches on the device (HIP events around them, pdmpc_hdv_kernel_ms)
  call     the whole device call (staging copy, launches, one read-back, synchronisation, the copies into the caller's arrays)
  host     the host twin (pdmpc_hdv_traffic_host), which also takes the map over on every call
and checks that device and host give the same bits.  Device and host calls alternate; one invocation is one session.

    python tools/hdv_timing.py [--reps 200] [--out profiles/hdv_timing.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd")]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import math

    from pdmpc import hdv
    from pdmpc import reachability as R
    from pdmpc.backend import Handle
    from pdmpc.config import Config, MpaType, ScenarioType
    from pdmpc.mpa import get_mpa
    from pdmpc.road_network import commonroad_scenario

    n, Hp = 20, 8
    options = Config(scenario_type=ScenarioType.commonroad, amount=n, Hp=Hp, max_vehicles=32)
    sc = commonroad_scenario(options, seed=1)
    lab = hdv.lab_hdv_map()
    # the HDVs' automaton: single_speed without the recursive-feasibility mask (ManualVehicle.m:20-27)
    sets = R.local_reachable_sets_conv(get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=1, Hp=Hp, mpa_type=MpaType.single_speed, recursive_feasibility=False)))

    def on(lanelet, q):  # centre point q of a lanelet, heading along the centre line
        c = lab.centre[lanelet - 1]
        b = min(q + 1, c.shape[0] - 1)
        return float(c[q, 0]), float(c[q, 1]), math.atan2(c[b, 1] - c[b - 1, 1], c[b, 0] - c[b - 1, 0])

    poses = [on(3, 3), on(17, 10)]
    zero = (0.0, 0.0)
    args = ([p[0] for p in poses], [p[1] for p in poses], [p[2] for p in poses], [1, 1], [zero, zero], [v.x_start for v in sc.vehicles], [v.y_start for v in sc.vehicles],
            [int(v.lanelets_index[0]) for v in sc.vehicles], [zero] * n)
    handle = Handle(options)
    handle.upload_hdv_map(lab, sets)
    host = hdv.hdv_traffic_native(lab, sets, *args)
    total = int(host["set_offset"][-1])
    dev = handle.hdv_traffic(*args, capacity=total)
    assert dev["closest"] == host["closest"] and dev["row_hdv"] == host["row_hdv"] and np.array_equal(dev["adjacency"], host["adjacency"])
    assert np.array_equal(dev["set_offset"], host["set_offset"]) and np.array_equal(dev["flags"], host["flags"])
    assert all(a.tobytes() == b.tobytes() for ra, rb in zip(dev["sets"], host["sets"]) for a, b in zip(ra, rb)), "device = host twin, bit for bit"
    kern, call, twin = [], [], []
    for _ in range(a.reps):
        handle.hdv_traffic(*args, capacity=total, call_ms=call)
        kern.append(handle.hdv_kernel_ms())
        hdv.hdv_traffic_native(lab, sets, *args, capacity=total, call_ms=twin)
    handle.close()
    q = lambda v: "median %.4f  min %.4f  p90 %.4f" % (np.median(v), np.min(v), np.percentile(v, 90))  # noqa: E731
    lines = ["HDV traffic call, 2 HDVs / 20 CAVs / Hp 8: %d rows, %d reachable lanes, %d vertices, %d adjacent pairs; %d calls each, ms" %
             (len(host["row_hdv"]), len(host["row_hdv"]) * Hp, total, int(host["adjacency"].sum()), a.reps),
             "  kernel (4 launches, HIP events)   " + q(kern), "  device call (wall)                " + q(call), "  host twin (wall)                  " + q(twin)]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
