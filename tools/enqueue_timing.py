"""Enqueue time on the host (pdmpc_last_call_timing's us3[1]: launch_range -- plan, arguments, boards, events, launch) of 500
pdmpc_plan_step and 500 pdmpc_plan_step_sampled calls: 20 recorded steps of a 20-vehicle closed loop (road network seed 1, Hp 8), 25 passes
after 5 warm-up passes.  One process per run; PDMPC_LIB selects the library.  profiles/sampled_host_side.txt holds its output.

    python tools/enqueue_timing.py
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-dmpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np

from pdmpc import abi
from pdmpc.backend import Handle
from pdmpc.config import Config, ScenarioType
from pdmpc.mpa import get_mpa
from pdmpc.road_network import commonroad_scenario
from sampled_step_timing import record_steps

options = Config(scenario_type=ScenarioType.commonroad, amount=20, Hp=8, max_vehicles=32, max_nodes=1 << 17)
sc = commonroad_scenario(options, seed=1)
mpa = get_mpa(options)
steps = record_steps(options, mpa, sc, 20)
h = Handle(options)
h.upload_mpa(mpa)
args = [(h.step_args(p["iters"], p["preds"], [f if f is not None else [] for f in p["fallback"]]), s) for p, s in steps]
us3 = (C.c_double * 3)()
for name in ("pdmpc_plan_step", "pdmpc_plan_step_sampled"):
    enq, pack = [], []
    for p in range(30):
        for (n, arr, off, idx, fb, _), seeds in args:
            out = abi.out_array(n)
            if name == "pdmpc_plan_step":
                rc = h.L.pdmpc_plan_step(h.h, n, arr, abi.i32p(off), abi.i32p(idx), fb, abi.out_ptr(out))
            else:
                sd = (C.c_uint32 * n)(*seeds)
                rc = h.L.pdmpc_plan_step_sampled(h.h, n, arr, abi.i32p(off), abi.i32p(idx), fb, sd, abi.out_ptr(out))
            assert rc == 0
            assert h.L.pdmpc_last_call_timing(h.h, us3) == 0
            if p >= 5:
                pack.append(us3[0])
                enq.append(us3[1])
    print("%-24s enqueue us median %.3f [p10 %.3f .. p90 %.3f] of %d calls   pack us median %.3f" % (name, np.median(enq), np.percentile(enq, 10), np.percentile(enq, 90), len(enq), np.median(pack)))
h.close()
