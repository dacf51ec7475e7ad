"""ctypes wrapper of the native step controller (csrc/step_controller.cpp and its stages csrc/step_*.hpp, declared in include/pdmpc.h).

`NativeController` is the C++ twin of `pdmpc.controller.PrioritizedSequentialController` (constant and colouring priorities,
full / distance / reachable-set coupling, parallel predecessors by previous plan or by reachable sets, GreedyCutter grouping): a whole MPC time step — traffic info, coupling, levels, obstacle assembly,
one kernel launch, fallbacks, plant update — is one C call (`pdmpc_controller_step`), so a closed loop has no interpreter
on its critical path.  The scenario is handed over once as flat arrays.
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import ControllerConfig, ScenarioStruct  # noqa: F401  (their home; importable from here as before)
from .backend import BackendError  # noqa: F401  (importable from here as before)
from .backend import _check, load_library
from .config import ConstraintFromSuccessor

COUPLING = {"full": 0, "distance": 1, "none": 2, "reachable_set": 3}
PARALLEL_PREVIOUS_TRAJECTORY, PARALLEL_REACHABLE_SETS = 0, 1
PRIORITY = {"constant": 0, "coloring": 1, "random": 2, "fca": 3}
WEIGHT = {"distance": 0, "constant": 1, "random": 2}
OPTIMIZER = {"graph_search": 0, "sampled": 1}  # PDMPC_OPTIMIZER_*
SUCCESSOR = {ConstraintFromSuccessor.none: 0, ConstraintFromSuccessor.area_of_standstill: 1, ConstraintFromSuccessor.area_of_previous_trajectory: 2}


TIMING_PARTS = ("build", "pack", "enqueue", "wait_and_read_back", "choose", "apply")  # pdmpc_controller_last_timing, pdmpc_sweep_last_timing


def _run(check, what, fn, obj, *counts):
    """An n_steps call `fn` (n_steps: the last count) -> wall-clock milliseconds of every step."""
    ms = np.zeros(max(counts[-1], 1))
    check(fn(obj, *counts, abi.dp(ms)), what)
    return ms[: counts[-1]]


def _flat(arrays, dtype):
    off = np.zeros(len(arrays) + 1, dtype=np.int32)
    for i, a in enumerate(arrays):
        off[i + 1] = off[i] + len(a)
    data = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=dtype).ravel() for a in arrays] + [np.zeros(1, dtype=dtype)]))
    return off, data


def _polys(ps):
    """PolygonSet -> list of (2, V) arrays."""
    out = []
    for p in range(ps.n_polygons):
        a, b = ps.offset[p], ps.offset[p + 1]
        out.append(np.array([[ps.x[q] for q in range(a, b)], [ps.y[q] for q in range(a, b)]]).reshape(2, b - a))
    return out


def _decode_iters(Hp, n, vin):
    """n VehicleIn -> list[VehicleIter] (for tests)."""
    from .iteration_data import VehicleIter

    iters = []
    for s in range(n):
        v = vin[s]
        dyn = _polys(v.dynamic_obstacles)
        hdv_sets = _polys(v.hdv_reachable_sets)
        left = np.array([[v.left_x[q] for q in range(v.n_left)], [v.left_y[q] for q in range(v.n_left)]]) if v.n_left else None
        right = np.array([[v.right_x[q] for q in range(v.n_right)], [v.right_y[q] for q in range(v.n_right)]]) if v.n_right else None
        iters.append(VehicleIter(
            x0=np.array([v.x0, v.y0, v.yaw0, 0.0]), trim_index=int(v.trim0),
            reference_trajectory_points=np.array([[v.ref_x[q], v.ref_y[q]] for q in range(Hp)]), v_ref=np.array([v.v_ref[q] for q in range(Hp)]),
            predicted_lanelet_boundary=(left, right), obstacles=_polys(v.obstacles),
            dynamic_obstacle_area=[dyn[r * Hp : (r + 1) * Hp] for r in range(len(dyn) // Hp)],
            hdv_reachable_sets=[hdv_sets[r * Hp : (r + 1) * Hp] for r in range(len(hdv_sets) // Hp)],
        ))
    return iters


class NativeController:
    def __init__(self, options, scenario, mpa, handle=None, coupling="full", priority_strategy="constant", weight_strategy="distance", optimizer="graph_search"):
        if scenario.dynamic_obstacle_area:
            raise ValueError("the native controller takes static scenario obstacles only")
        self.L = load_library()
        self.options, self.mpa, self.n, self.Hp = options, mpa, options.amount, options.Hp
        veh = scenario.vehicles
        keep = []

        def d(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            return abi.dp(a)

        def i32(a):
            a = np.ascontiguousarray(a, dtype=np.int32)
            keep.append(a)
            return abi.i32p(a)

        s = ScenarioStruct()
        s.n_vehicles = self.n
        s.x_start, s.y_start, s.yaw_start = d([v.x_start for v in veh]), d([v.y_start for v in veh]), d([v.yaw_start for v in veh])
        s.reference_speed = d([v.reference_speed for v in veh])
        po, px = _flat([v.reference_path[:, 0] for v in veh], np.float64)
        _, py = _flat([v.reference_path[:, 1] for v in veh], np.float64)
        s.path_offset, s.path_x, s.path_y = i32(po), d(px), d(py)
        if veh[0].lanelets_index is not None:
            lo, li = _flat([v.lanelets_index for v in veh], np.int32)
            _, pi = _flat([v.points_index for v in veh], np.int32)
            s.lanelets_offset, s.lanelets_index, s.points_index = i32(lo), i32(li), i32(pi)
            s.is_loop = i32([1 if v.is_loop else 0 for v in veh])
            off = getattr(scenario, "tile_offset", [(0.0, 0.0)] * self.n)
            s.tile_dx, s.tile_dy = d([o[0] for o in off]), d([o[1] for o in off])
            bl = scenario.lanelet_boundary
            s.n_lanelets = len(bl)
            lo_, lx = _flat([b[0][:, 0] for b in bl], np.float64)
            _, ly = _flat([b[0][:, 1] for b in bl], np.float64)
            ro_, rx = _flat([b[1][:, 0] for b in bl], np.float64)
            _, ry = _flat([b[1][:, 1] for b in bl], np.float64)
            s.left_offset, s.right_offset = i32(lo_), i32(ro_)
            s.left_x, s.left_y, s.right_x, s.right_y = d(lx), d(ly), d(rx), d(ry)
        k2 = abi._Keep()
        s.obstacles = abi.pack_polygon_set(list(scenario.obstacles), k2)
        keep.append(k2)
        s.n_trims = len(mpa.trims)
        s.trim_speed, s.trim_steering = d([t.speed for t in mpa.trims]), d([t.steering for t in mpa.trims])
        cfg = ControllerConfig(
            Hp=options.Hp, coupling=COUPLING[coupling], priority_strategy=PRIORITY[priority_strategy], weight_strategy=WEIGHT[weight_strategy],
            max_num_CLs=options.max_num_CLs, constraint_from_successor=SUCCESSOR[options.constraint_from_successor], dt_seconds=options.dt_seconds,
            offset=options.offset, vehicle_length=veh[0].Length, vehicle_width=veh[0].Width,
        )
        self.handle = handle  # keeps the backend handle alive as long as the controller that drives it
        self.c = C.c_void_p()
        rc = self.L.pdmpc_controller_create(handle.h if handle is not None else None, C.byref(cfg), C.byref(s), C.byref(self.c))
        self._check(rc, "pdmpc_controller_create")
        del keep
        if coupling == "reachable_set" or options.is_deal_prediction_inconsistency:
            # the automaton's local reachable sets, computed natively (and uploaded to the handle's device, if any)
            ms, mkeep = abi.pack_mpa(mpa)
            self._check(self.L.pdmpc_controller_set_reachability(self.c, C.byref(ms)), "pdmpc_controller_set_reachability")
            del mkeep
        if options.is_deal_prediction_inconsistency:
            self._check(self.L.pdmpc_controller_set_parallel_coupling(self.c, PARALLEL_REACHABLE_SETS), "pdmpc_controller_set_parallel_coupling")
        if options.bound_reachable_sets:
            self._check(self.L.pdmpc_controller_set_lanelet_bounding(self.c, 1), "pdmpc_controller_set_lanelet_bounding")
        if optimizer != "graph_search":
            self.set_optimizer(optimizer)

    def set_optimizer(self, which):
        """"graph_search" (default) or "sampled" (pdmpc_controller_set_optimizer): what step / run, explore_* and optimal_* plan with."""
        self._check(self.L.pdmpc_controller_set_optimizer(self.c, OPTIMIZER[which] if isinstance(which, str) else int(which)), "pdmpc_controller_set_optimizer")

    def seeds(self):
        """The sampled optimizer's seed per slot of the last built step or batch (pdmpc_controller_seeds)."""
        n = C.c_int32()
        p = C.POINTER(C.c_uint32)()
        self._check(self.L.pdmpc_controller_seeds(self.c, C.byref(n), C.byref(p)), "pdmpc_controller_seeds")
        return [int(p[i]) for i in range(n.value)]

    def priorities(self):
        """(priorities, collisions) of the last built step (pdmpc_controller_priorities): the 1-based priorities of a constant, random or
        FCA step and the collision counts of an FCA step; empty where the strategy has none."""
        n_p, n_c = C.c_int32(), C.c_int32()
        p, q = abi.c_int32_p(), abi.c_int32_p()
        self._check(self.L.pdmpc_controller_priorities(self.c, C.byref(n_p), C.byref(p), C.byref(n_c), C.byref(q)), "pdmpc_controller_priorities")
        return [int(p[i]) for i in range(n_p.value)], [int(q[i]) for i in range(n_c.value)]

    def _check(self, rc, what):
        _check(self.L, rc, what, "pdmpc_controller_last_error")

    # ---- human-driven vehicles: twin of PrioritizedSequentialController.set_hdvs / set_hdv_measurements / hdv_info
    def set_hdvs(self, hdv_mpa, successors, relationship, tile=None):
        """pdmpc_controller_set_hdvs: options.manual_control HDVs on the scenario's lanelets with the lanelet graph given here
        (successors: per lanelet its successor ids; relationship: (n, n) uint8), hdv_mpa their own automaton, tile[h] = (dx, dy)."""
        n_hdv = int(self.options.manual_control)
        so = np.zeros(len(successors) + 1, dtype=np.int32)
        so[1:] = np.cumsum([len(s) for s in successors])
        si = np.array([int(s) for row in successors for s in row] + [0], dtype=np.int32)
        rel = np.ascontiguousarray(relationship, dtype=np.uint8)
        ms, keep = abi.pack_mpa(hdv_mpa)
        t = np.zeros((max(n_hdv, 1), 2)) if tile is None else np.ascontiguousarray(tile, dtype=np.float64).reshape(-1, 2)
        tx, ty = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])
        rc = self.L.pdmpc_controller_set_hdvs(self.c, n_hdv, C.byref(ms), abi.i32p(so), abi.i32p(si), abi.u8p(rel), abi.dp(tx), abi.dp(ty))
        del keep
        self._check(rc, "pdmpc_controller_set_hdvs")

    def set_hdv_measurements(self, x, y, yaw):
        """pdmpc_controller_set_hdv_measurements: the HDVs' measured poses, kept until set again."""
        n_hdv = int(self.options.manual_control)
        a = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (x, y, yaw)]
        if any(v.size != n_hdv for v in a):
            raise ValueError("set_hdv_measurements: %d poses" % n_hdv)
        self._check(self.L.pdmpc_controller_set_hdv_measurements(self.c, abi.dp(a[0]), abi.dp(a[1]), abi.dp(a[2])), "pdmpc_controller_set_hdv_measurements")

    def set_hdv_poses(self, x, y, cos_yaw, sin_yaw):
        """pdmpc_controller_set_hdv_poses: measurements given as directions (cos and sin as they are)."""
        a = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (x, y, cos_yaw, sin_yaw)]
        if any(v.size != int(self.options.manual_control) for v in a):
            raise ValueError("set_hdv_poses: %d poses" % int(self.options.manual_control))
        self._check(self.L.pdmpc_controller_set_hdv_poses(self.c, *[abi.dp(v) for v in a]), "pdmpc_controller_set_hdv_poses")

    def set_hdv_drivers(self, routes, start_distance, v_des, params=None):
        """pdmpc_controller_set_hdv_drivers: twin of PrioritizedSequentialController.set_hdv_drivers (routes [(lanelet ids, closed)])."""
        from . import hdv

        n_hdv = int(self.options.manual_control)
        if not (len(routes) == len(start_distance) == len(v_des) == n_hdv):
            raise ValueError("set_hdv_drivers: %d routes, start distances and speeds" % n_hdv)
        off, lan, closed = hdv._route_arrays(routes)
        d = np.array([float(v) for v in start_distance] + [0.0])
        v = np.array([float(a) for a in v_des] + [0.0])
        par = np.array([float(p) for p in (hdv.DRIVE_DEFAULTS if params is None else params)], dtype=np.float64)
        self._check(self.L.pdmpc_controller_set_hdv_drivers(self.c, abi.i32p(off), abi.i32p(lan), abi.u8p(closed), abi.dp(d), abi.dp(v), abi.dp(par)),
                    "pdmpc_controller_set_hdv_drivers")

    def hdv_driver_state(self):
        """pdmpc_controller_hdv_driver_state -> dict: states [(r, j, u)], x, y, yaw, speed, gap of the last built step"""
        n = int(self.options.manual_control)
        seg, out = np.zeros(2 * n, dtype=np.int32), [np.zeros(n) for _ in range(6)]
        self._check(self.L.pdmpc_controller_hdv_driver_state(self.c, abi.i32p(seg), *[abi.dp(a) for a in out]), "pdmpc_controller_hdv_driver_state")
        u, x, y, yaw, speed, gap = out
        return dict(states=[(int(seg[q]), int(seg[n + q]), float(u[q])) for q in range(n)], x=x.tolist(), y=y.tolist(), yaw=yaw.tolist(), speed=speed.tolist(), gap=gap.tolist())

    def set_hdv_recording(self, x, y, yaw):
        """pdmpc_controller_set_hdv_recording: (T, n_hdv) recorded poses; built step s (from 1) takes row min(s, T) - 1."""
        n = int(self.options.manual_control)
        a = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, n)) for v in (x, y, yaw)]
        if not (a[0].shape == a[1].shape == a[2].shape):
            raise ValueError("set_hdv_recording: (T, %d) poses" % n)
        self._check(self.L.pdmpc_controller_set_hdv_recording(self.c, int(a[0].shape[0]), *[abi.dp(v) for v in a]), "pdmpc_controller_set_hdv_recording")

    def hdv_info(self):
        """pdmpc_controller_hdv_info: the traffic info of the last built step in the dict form of hdv.hdv_traffic."""
        n, rows = C.c_int32(), C.c_int32()
        co, ci, rh, so = (abi.c_int32_p() for _ in range(4))
        sx, sy = abi.c_double_p(), abi.c_double_p()
        fl, adj = abi.c_uint8_p(), abi.c_uint8_p()
        self._check(self.L.pdmpc_controller_hdv_info(self.c, C.byref(n), C.byref(co), C.byref(ci), C.byref(rows), C.byref(rh), C.byref(so), C.byref(sx), C.byref(sy), C.byref(fl),
                                                      C.byref(adj)), "pdmpc_controller_hdv_info")
        H, R, Hp = n.value, rows.value, self.Hp
        sets = [[np.array([[sx[q] for q in range(so[r * Hp + k], so[r * Hp + k + 1])], [sy[q] for q in range(so[r * Hp + k], so[r * Hp + k + 1])]]).reshape(2, -1)
                 for k in range(Hp)] for r in range(R)]
        return dict(closest=[[int(ci[q]) for q in range(co[h], co[h + 1])] for h in range(H)], row_hdv=[int(rh[r]) for r in range(R)], sets=sets,
                    flags=np.array([fl[q] for q in range(R * Hp)], dtype=np.uint8).reshape(R, Hp),
                    adjacency=np.array([adj[q] for q in range(self.n * H)], dtype=np.uint8).reshape(self.n, H))

    def close(self):
        if self.c:
            self.L.pdmpc_controller_destroy(self.c)
            self.c = C.c_void_p()

    def records(self):
        """The records of the member's last step in its own slot order (pdmpc_controller_records), also after a sweep's step."""
        return abi.records_copy(self.L.pdmpc_controller_records(self.c), self.n)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self):
        """One whole MPC time step natively (build, one launch, apply); returns the records in slot order."""
        self._check(self.L.pdmpc_controller_step(self.c), "pdmpc_controller_step")
        return abi.records_copy(self.L.pdmpc_controller_records(self.c), self.n)

    def run(self, n_steps):
        """n_steps closed-loop steps in one native call -> wall-clock milliseconds of every step."""
        return _run(self._check, "pdmpc_controller_run", self.L.pdmpc_controller_run, self.c, n_steps)

    def last_timing(self):
        """Host milliseconds of the last step by part (pdmpc_controller_last_timing)."""
        t = (C.c_double * 6)()
        self._check(self.L.pdmpc_controller_last_timing(self.c, t), "pdmpc_controller_last_timing")
        return dict(zip(TIMING_PARTS, (float(x) for x in t)))

    def timing_mean(self, reset=True):
        """Mean host milliseconds per step by part over the steps since the last reset (pdmpc_controller_timing_sum)."""
        t = (C.c_double * 6)()
        k = C.c_int64(0)
        self._check(self.L.pdmpc_controller_timing_sum(self.c, t, C.byref(k), 1 if reset else 0), "pdmpc_controller_timing_sum")
        return dict(zip(TIMING_PARTS, (float(x) / max(k.value, 1) for x in t)))

    def build_step(self):
        self._check(self.L.pdmpc_controller_build_step(self.c), "pdmpc_controller_build_step")

    def apply(self, records):
        recs = np.ascontiguousarray(records)
        self._check(self.L.pdmpc_controller_apply(self.c, abi.out_ptr(recs)), "pdmpc_controller_apply")

    def problem(self):
        """The last built step problem decoded into the dict form of controller.build_step_problem (for tests)."""
        n = C.c_int32()
        vin = C.POINTER(abi.VehicleIn)()
        po, pi, order, levels = abi.c_int32_p(), abi.c_int32_p(), abi.c_int32_p(), abi.c_int32_p()
        fb = C.POINTER(abi.PolygonSet)()
        self._check(self.L.pdmpc_controller_problem(self.c, C.byref(n), C.byref(vin), C.byref(po), C.byref(pi), C.byref(fb), C.byref(order), C.byref(levels)), "pdmpc_controller_problem")
        iters, preds, fallback = self._decode(n.value, vin, po, pi, fb)
        order_l = [int(order[s]) for s in range(n.value)]
        lv = [int(levels[v]) for v in range(n.value)]
        level_sizes = [sum(1 for x in lv if x == l) for l in range(1, max(lv) + 1)]
        return {"order": order_l, "iters": iters, "preds": preds, "fallback": fallback, "level_sizes": level_sizes, "levels": [lv[v] for v in order_l]}

    def _decode(self, n, vin, po, pi, fb):
        iters, preds, fallback = _decode_iters(self.Hp, n, vin), [], []
        for s in range(n):
            preds.append([int(pi[q]) for q in range(po[s], po[s + 1])])
            f = _polys(fb[s])
            fallback.append(f if f else None)
        return iters, preds, fallback

    # ---- the explorative step: twin of pdmpc.explorative
    def explore_build(self, n_perm, seed):
        self._check(self.L.pdmpc_controller_explore_build(self.c, n_perm, int(seed)), "pdmpc_controller_explore_build")
        self.n_perm = n_perm

    def explore_problem(self):
        """The flattened batch of the last explore_build in the dict form of explorative.build_exploration_batch (for tests)."""
        n = C.c_int32()
        vin = C.POINTER(abi.VehicleIn)()
        po, pi, inst, veh, lvl = (abi.c_int32_p() for _ in range(5))
        fb = C.POINTER(abi.PolygonSet)()
        self._check(self.L.pdmpc_controller_explore_problem(self.c, C.byref(n), C.byref(vin), C.byref(po), C.byref(pi), C.byref(fb), C.byref(inst), C.byref(veh), C.byref(lvl)),
                    "pdmpc_controller_explore_problem")
        iters, preds, fallback = self._decode(n.value, vin, po, pi, fb)
        N = n.value
        levels = [int(lvl[s]) for s in range(N)]
        vehicles = [int(veh[s]) for s in range(N)]
        return {"order": vehicles, "iters": iters, "preds": preds, "fallback": fallback, "levels": levels, "instance": [int(inst[s]) for s in range(N)], "vehicle": vehicles,
                "level_sizes": [sum(1 for x in levels if x == l) for l in range(1, max(levels) + 1)], "n_instances": self.n_perm}

    def explore_choose(self, records):
        """-> (instance chosen per vehicle, cost table n_perm x n_graphs)."""
        recs = np.ascontiguousarray(records)
        chosen = np.zeros(self.n, dtype=np.int32)
        g = C.c_int32()
        cost = np.zeros(self.n_perm * self.n)
        self._check(self.L.pdmpc_controller_explore_choose(self.c, abi.out_ptr(recs), abi.i32p(chosen), C.byref(g), abi.dp(cost)),
                    "pdmpc_controller_explore_choose")
        return chosen, cost[: self.n_perm * g.value].reshape(self.n_perm, g.value)

    def explore_step(self, n_perm):
        """One explorative time step natively (batch, ONE launch, choice, apply) -> (records of the batch, chosen instance per vehicle)."""
        self._check(self.L.pdmpc_controller_explore_step(self.c, n_perm), "pdmpc_controller_explore_step")
        self.n_perm = n_perm
        chosen = np.zeros(self.n, dtype=np.int32)
        p = C.POINTER(abi.VehicleOut)()
        self._check(self.L.pdmpc_controller_explore_result(self.c, abi.i32p(chosen), None, None, C.byref(p)), "pdmpc_controller_explore_result")
        return abi.records_copy(p, self.n * n_perm), chosen

    def explore_follow_own(self, on=True):
        self._check(self.L.pdmpc_controller_explore_follow_own(self.c, 1 if on else 0), "pdmpc_controller_explore_follow_own")

    def set_group(self, group, mode=0):
        """pdmpc_controller_set_group: the steps plan over `group` (a backend.Group whose rank 0 handle -- group.rank0() -- the controller
        was created on) with sharding `mode` (backend.SHARD_*); None: back on the handle.  The state after every step is the handle's."""
        self._check(self.L.pdmpc_controller_set_group(self.c, group.g if group is not None else None, mode), "pdmpc_controller_set_group")
        self._group = group  # (kept alive as long as the controller plans on it)

    def set_device_choice(self, on=True):
        """explore_run / optimal_run choose and gather the chosen plans on the device, ONE call per step (pdmpc_controller_set_device_choice)."""
        self._check(self.L.pdmpc_controller_set_device_choice(self.c, 1 if on else 0), "pdmpc_controller_set_device_choice")

    def explore_result(self):
        """The last explorative choice, also of a sweep's member -> (instance chosen per vehicle, cost table n_perm x n_graphs)."""
        chosen = np.zeros(self.n, dtype=np.int32)
        g = C.c_int32()
        cost = abi.c_double_p()
        self._check(self.L.pdmpc_controller_explore_result(self.c, abi.i32p(chosen), C.byref(g), C.byref(cost), None), "pdmpc_controller_explore_result")
        return chosen, np.array([cost[q] for q in range(self.n_perm * g.value)]).reshape(self.n_perm, g.value)

    def optimal_result(self):
        """The last optimal-priority choice -> (instance chosen per vehicle, cost table n x K)."""
        chosen = np.zeros(self.n, dtype=np.int32)
        k = C.c_int32()
        cost = abi.c_double_p()
        self._check(self.L.pdmpc_controller_optimal_result(self.c, abi.i32p(chosen), C.byref(k), C.byref(cost), None), "pdmpc_controller_optimal_result")
        return chosen, np.array([cost[q] for q in range(self.n * k.value)]).reshape(self.n, k.value)

    def explore_run(self, n_perm, n_steps):
        self.n_perm = n_perm
        return _run(self._check, "pdmpc_controller_explore_run", self.L.pdmpc_controller_explore_run, self.c, n_perm, n_steps)

    # ---- the optimal-priority step: twin of pdmpc.optimal
    def optimal_build(self, max_instances):
        """Every unique prioritization of the step as one batch (pdmpc_controller_optimal_build) -> K."""
        self._check(self.L.pdmpc_controller_optimal_build(self.c, max_instances), "pdmpc_controller_optimal_build")
        n = C.c_int32()
        self._check(self.L.pdmpc_controller_explore_problem(self.c, C.byref(n), None, None, None, None, None, None, None), "pdmpc_controller_explore_problem")
        self.n_perm = n.value // self.n
        return self.n_perm

    def optimal_problem(self):
        """The flattened batch of the last optimal_build in the dict form of optimal.build_optimal_batch (for tests)."""
        return self.explore_problem()

    def optimal_choose(self, records):
        """-> (instance chosen per vehicle, cost table n x K)."""
        recs = np.ascontiguousarray(records)
        chosen = np.zeros(self.n, dtype=np.int32)
        cost = np.zeros(self.n * self.n_perm)
        self._check(self.L.pdmpc_controller_optimal_choose(self.c, abi.out_ptr(recs), abi.i32p(chosen), abi.dp(cost)),
                    "pdmpc_controller_optimal_choose")
        return chosen, cost.reshape(self.n, self.n_perm)

    def optimal_step(self, max_instances):
        """One optimal-priority time step natively (batch, ONE launch, choice, apply) -> (records of the batch, chosen instance per vehicle)."""
        self._check(self.L.pdmpc_controller_optimal_step(self.c, max_instances), "pdmpc_controller_optimal_step")
        chosen = np.zeros(self.n, dtype=np.int32)
        k = C.c_int32()
        p = C.POINTER(abi.VehicleOut)()
        self._check(self.L.pdmpc_controller_optimal_result(self.c, abi.i32p(chosen), C.byref(k), None, C.byref(p)), "pdmpc_controller_optimal_result")
        self.n_perm = k.value
        return abi.records_copy(p, self.n * k.value), chosen

    def optimal_run(self, max_instances, n_steps):
        """n_steps optimal-priority steps in one native call (status + final cost of every plan, the chosen records only) -> ms per step."""
        return _run(self._check, "pdmpc_controller_optimal_run", self.L.pdmpc_controller_optimal_run, self.c, max_instances, n_steps)

    # ---- centralized control: twin of pdmpc.centralized.CentralizedController (pdmpc_controller_centralized_*)
    def centralized_build(self):
        """The joint problem of the next time step (CentralizedController.build_iters); advances the time step."""
        self._check(self.L.pdmpc_controller_centralized_build(self.c), "pdmpc_controller_centralized_build")

    def centralized_problem(self, raw=False):
        """The joint problem of the last centralized_build -> list[VehicleIter] in vehicle order (raw: the VehicleIn array itself,
        valid until the next build)."""
        n = C.c_int32()
        vin = C.POINTER(abi.VehicleIn)()
        self._check(self.L.pdmpc_controller_centralized_problem(self.c, C.byref(n), C.byref(vin)), "pdmpc_controller_centralized_problem")
        return (n.value, vin) if raw else _decode_iters(self.Hp, n.value, vin)

    def centralized_apply(self, records):
        """The records of the joint problem in vehicle order: the plant update.  An exhausted search raises BackendError with
        .status == abi.EXHAUSTED and applies nothing."""
        recs = np.ascontiguousarray(records)
        if recs.shape[0] != self.n:
            raise ValueError("a joint problem of %d vehicles takes %d records, not %d" % (self.n, self.n, recs.shape[0]))
        self._check(self.L.pdmpc_controller_centralized_apply(self.c, abi.out_ptr(recs)), "pdmpc_controller_centralized_apply")

    def centralized_step(self):
        """One centralized time step natively (build, ONE joint search, apply) -> the records in vehicle order."""
        self._check(self.L.pdmpc_controller_centralized_step(self.c), "pdmpc_controller_centralized_step")
        return self.records()

    def centralized_run(self, n_steps):
        """n_steps centralized steps in one native call -> wall-clock milliseconds of every step."""
        return _run(self._check, "pdmpc_controller_centralized_run", self.L.pdmpc_controller_centralized_run, self.c, n_steps)

    def state(self):
        n = self.n
        arr = [np.zeros(n) for _ in range(5)]
        nf = np.zeros(n, dtype=np.int32)
        k = C.c_int32()
        self._check(self.L.pdmpc_controller_state(self.c, *[abi.dp(a) for a in arr], abi.i32p(nf), C.byref(k)), "pdmpc_controller_state")
        return {"x": arr[0], "y": arr[1], "yaw": arr[2], "speed": arr[3], "steering": arr[4], "needs_fallback": nf != 0, "k": k.value}


class NativeSweep:
    """Several closed loops in lock-step (pdmpc_sweep_*): `members` are NativeControllers created on `handle` (or all
    without one); a step is every member's build with the device's step preparation grouped over the members, ONE launch for all of
    them, every member's apply.  Each member ends a sweep step byte for byte where its own step() would have left it.  The members
    stay the caller's (and are kept alive by the sweep)."""

    def __init__(self, members, handle=None):
        self.members = list(members)
        self.handle = handle
        self.L = load_library()
        self.n = sum(m.n for m in self.members)
        self.s = C.c_void_p()
        arr = (C.c_void_p * max(len(self.members), 1))(*[m.c for m in self.members])
        rc = self.L.pdmpc_sweep_create(handle.h if handle is not None else None, len(self.members), arr, C.byref(self.s))
        self._check(rc, "pdmpc_sweep_create")

    def _check(self, rc, what):
        _check(self.L, rc, what, "pdmpc_controller_last_error")

    def close(self):
        if self.s:
            self.L.pdmpc_sweep_destroy(self.s)
            self.s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build(self):
        self._check(self.L.pdmpc_sweep_build(self.s), "pdmpc_sweep_build")

    def problem(self):
        """The concatenated problem of the last build, decoded as NativeController.problem decodes a member's, plus member / member_slot
        per sweep slot."""
        n = C.c_int32()
        vin = C.POINTER(abi.VehicleIn)()
        po, pi, mem, slot = (abi.c_int32_p() for _ in range(4))
        fb = C.POINTER(abi.PolygonSet)()
        self._check(self.L.pdmpc_sweep_problem(self.s, C.byref(n), C.byref(vin), C.byref(po), C.byref(pi), C.byref(fb), C.byref(mem), C.byref(slot)), "pdmpc_sweep_problem")
        iters, preds, fallback = self.members[0]._decode(n.value, vin, po, pi, fb)
        return {"iters": iters, "preds": preds, "fallback": fallback, "member": [int(mem[q]) for q in range(n.value)],
                "member_slot": [int(slot[q]) for q in range(n.value)]}

    def apply(self, records):
        recs = np.ascontiguousarray(records)
        if recs.shape[0] != self.n:
            raise ValueError("a sweep of %d slots takes %d records, not %d" % (self.n, self.n, recs.shape[0]))
        self._check(self.L.pdmpc_sweep_apply(self.s, abi.out_ptr(recs)), "pdmpc_sweep_apply")

    def set_group(self, group, mode=0):
        """pdmpc_sweep_set_group: the lock-steps plan over `group` (the sweep and its members were created on group.rank0()); None: back
        on the handle."""
        self._check(self.L.pdmpc_sweep_set_group(self.s, group.g if group is not None else None, mode), "pdmpc_sweep_set_group")
        self._group = group

    def step(self):
        """One lock-step natively -> every member's records in its own slot order."""
        self._check(self.L.pdmpc_sweep_step(self.s), "pdmpc_sweep_step")
        return [m.records() for m in self.members]

    def run(self, n_steps):
        """n_steps lock-steps in one native call -> wall-clock milliseconds of every lock-step."""
        return _run(self._check, "pdmpc_sweep_run", self.L.pdmpc_sweep_run, self.s, n_steps)

    # ---- the explorative step of a sweep
    def explore_build(self, n_perm):
        self._check(self.L.pdmpc_sweep_explore_build(self.s, n_perm), "pdmpc_sweep_explore_build")
        self._n_perm(n_perm)

    def _n_perm(self, n_perm):
        for m in self.members:
            m.n_perm = n_perm

    def _batch_problem(self, name):
        """the concatenated batch behind the entry point `name`, decoded as NativeController.explore_problem decodes a member's, plus the
        member per slot"""
        n = C.c_int32()
        vin = C.POINTER(abi.VehicleIn)()
        po, pi, mem, inst, veh, lvl = (abi.c_int32_p() for _ in range(6))
        fb = C.POINTER(abi.PolygonSet)()
        self._check(getattr(self.L, name)(self.s, C.byref(n), C.byref(vin), C.byref(po), C.byref(pi), C.byref(fb), C.byref(mem), C.byref(inst), C.byref(veh), C.byref(lvl)), name)
        iters, preds, fallback = self.members[0]._decode(n.value, vin, po, pi, fb)
        col = lambda a: [int(a[q]) for q in range(n.value)]  # noqa: E731
        return {"iters": iters, "preds": preds, "fallback": fallback, "member": col(mem), "instance": col(inst), "vehicle": col(veh), "levels": col(lvl)}

    def _batch_apply(self, name, kind, records):
        """the records of every slot of the concatenated batch (`kind`, for the message) to the entry point `name`"""
        recs = np.ascontiguousarray(records)
        want = sum(m.n * m.n_perm for m in self.members)
        if recs.shape[0] != want:
            raise ValueError("the %s batch of this sweep has %d slots, not %d" % (kind, want, recs.shape[0]))
        self._check(getattr(self.L, name)(self.s, abi.out_ptr(recs)), name)

    def explore_problem(self):
        """The concatenated batch of the last explore_build, decoded as NativeController.explore_problem decodes a member's, plus the
        member per slot."""
        return self._batch_problem("pdmpc_sweep_explore_problem")

    def explore_apply(self, records):
        """The records of every slot of the concatenated batch: the choice per member on the host, every member's apply."""
        self._batch_apply("pdmpc_sweep_explore_apply", "explorative", records)

    def explore_step(self, n_perm):
        """One explorative lock-step natively -> every member's kept (chosen) records in its own slot order."""
        self._check(self.L.pdmpc_sweep_explore_step(self.s, n_perm), "pdmpc_sweep_explore_step")
        self._n_perm(n_perm)
        return [m.records() for m in self.members]

    def explore_run(self, n_perm, n_steps):
        """n_steps explorative lock-steps in one native call -> wall-clock milliseconds of every lock-step."""
        ms = _run(self._check, "pdmpc_sweep_explore_run", self.L.pdmpc_sweep_explore_run, self.s, n_perm, n_steps)
        self._n_perm(n_perm)
        return ms

    # ---- the optimal-priority step of a sweep
    def _n_instances(self):
        """every member's K after an optimal build or step -> the K per member"""
        ks = []
        for m in self.members:
            n = C.c_int32()
            m._check(self.L.pdmpc_controller_explore_problem(m.c, C.byref(n), None, None, None, None, None, None, None), "pdmpc_controller_explore_problem")
            m.n_perm = n.value // m.n
            ks.append(m.n_perm)
        return ks

    def optimal_build(self, max_instances):
        """Every member's optimal-priority batch behind ONE enumeration of all members' coupling graphs -> K per member."""
        self._check(self.L.pdmpc_sweep_optimal_build(self.s, max_instances), "pdmpc_sweep_optimal_build")
        return self._n_instances()

    def optimal_problem(self):
        """The concatenated batch of the last optimal_build, decoded as explore_problem decodes the explorative one."""
        return self._batch_problem("pdmpc_sweep_optimal_problem")

    def optimal_apply(self, records):
        """The records of every slot of the concatenated batch: the choice per member on the host, every member's apply."""
        self._batch_apply("pdmpc_sweep_optimal_apply", "optimal-priority", records)

    def optimal_step(self, max_instances):
        """One optimal-priority lock-step natively -> every member's kept (chosen) records in its own slot order."""
        self._check(self.L.pdmpc_sweep_optimal_step(self.s, max_instances), "pdmpc_sweep_optimal_step")
        self._n_instances()
        return [m.records() for m in self.members]

    def optimal_run(self, max_instances, n_steps):
        """n_steps optimal-priority lock-steps in one native call -> wall-clock milliseconds of every lock-step."""
        ms = _run(self._check, "pdmpc_sweep_optimal_run", self.L.pdmpc_sweep_optimal_run, self.s, max_instances, n_steps)
        self._n_instances()
        return ms

    def optimal_calls(self):
        """[enumeration calls of the last optimal build, launches of the searches of the last optimal_step] (pdmpc_sweep_optimal_last_calls)."""
        calls = np.zeros(2, dtype=np.int32)
        self._check(self.L.pdmpc_sweep_optimal_last_calls(self.s, abi.i32p(calls)), "pdmpc_sweep_optimal_last_calls")
        return calls.tolist()

    # ---- centralized members
    def centralized_build(self):
        """Every live member's joint problem (pdmpc_sweep_centralized_build)."""
        self._check(self.L.pdmpc_sweep_centralized_build(self.s), "pdmpc_sweep_centralized_build")

    def centralized_problem(self, raw=False):
        """The live members' joint problems of the last centralized_build -> {"problems": list of list[VehicleIter], "problem_offset",
        "member": whose each problem is} (raw: the VehicleIn array in place of the decoded problems)."""
        n = C.c_int32()
        off, mem = abi.c_int32_p(), abi.c_int32_p()
        vin = C.POINTER(abi.VehicleIn)()
        self._check(self.L.pdmpc_sweep_centralized_problem(self.s, C.byref(n), C.byref(off), C.byref(vin), C.byref(mem)), "pdmpc_sweep_centralized_problem")
        offs = [int(off[p]) for p in range(n.value + 1)]
        out = {"problem_offset": offs, "member": [int(mem[p]) for p in range(n.value)]}
        if raw:
            out["in"] = vin
        else:
            iters = _decode_iters(self.members[0].Hp, offs[-1], vin)
            out["problems"] = [iters[offs[p] : offs[p + 1]] for p in range(n.value)]
        return out

    def centralized_apply(self, records):
        """The records of the built problems, problem after problem: every member's apply; an exhausted member is retired."""
        recs = np.ascontiguousarray(records)
        self._check(self.L.pdmpc_sweep_centralized_apply(self.s, abi.out_ptr(recs)), "pdmpc_sweep_centralized_apply")

    def centralized_step(self):
        """One centralized lock-step natively (ONE pdmpc_plan_joint for all live members) -> centralized_status()."""
        self._check(self.L.pdmpc_sweep_centralized_step(self.s), "pdmpc_sweep_centralized_step")
        return self.centralized_status()

    def centralized_run(self, n_steps):
        """n_steps centralized lock-steps in one native call -> wall-clock milliseconds of every lock-step."""
        return _run(self._check, "pdmpc_sweep_centralized_run", self.L.pdmpc_sweep_centralized_run, self.s, n_steps)

    def centralized_status(self):
        """Per member 0, or the time step at which its search ran empty (pdmpc_sweep_centralized_status)."""
        st = np.zeros(max(len(self.members), 1), dtype=np.int32)
        self._check(self.L.pdmpc_sweep_centralized_status(self.s, abi.i32p(st)), "pdmpc_sweep_centralized_status")
        return st[: len(self.members)].tolist()

    def prep_calls(self):
        """The step-preparation calls of the last build, whatever the number of members (pdmpc_sweep_last_prep_calls): [lanelet
        bounding, coupler on the bounded sets, coupler on the plain hulls, future collision assessment]."""
        calls = np.zeros(4, dtype=np.int32)
        self._check(self.L.pdmpc_sweep_last_prep_calls(self.s, abi.i32p(calls)), "pdmpc_sweep_last_prep_calls")
        return calls.tolist()

    def last_hdv_calls(self):
        """(HDV traffic calls, map uploads) of the last build (pdmpc_sweep_last_hdv_calls): with a handle one grouped call for all
        members with HDVs, and no upload of a map that is still resident in a map slot of the handle."""
        calls = np.zeros(2, dtype=np.int32)
        self._check(self.L.pdmpc_sweep_last_hdv_calls(self.s, abi.i32p(calls)), "pdmpc_sweep_last_hdv_calls")
        return int(calls[0]), int(calls[1])

    def last_timing(self):
        """Host milliseconds of the last lock-step by part (pdmpc_sweep_last_timing)."""
        t = (C.c_double * 6)()
        self._check(self.L.pdmpc_sweep_last_timing(self.s, t), "pdmpc_sweep_last_timing")
        return dict(zip(TIMING_PARTS, (float(x) for x in t)))


Sweep = NativeSweep  # (the short name)
