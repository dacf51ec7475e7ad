"""Human-driven vehicles (HDVs): closest lanelets, chains, reachable lanes and CAV/HDV adjacency in numpy.

The Python twin of include/pdmpc_hdv.h, csrc/hdv.cpp and csrc/hdv_kernel.hip, operation by operation:
    closest lanelets    hlc/controller/common/map_position_to_closest_lanelets.m:1-25, literally
    reachable lane      scenarios/ManualVehicle.m:30-49 with the semantics of DESIGN.md §3.24 (b), (c); the intersection is the
                        bounding rule of pdmpc.reachability (bound_reachable_sets), an empty one a polygon of 0 columns
    adjacency           hlc/controller/common/is_hdv_behind.m:13-92 as restated in §3.24 (d)
    traffic info        HighLevelController.update_hdv_traffic_info (hlc/controller/HighLevelController.m:394-447)
`hdv_traffic_native` is the same call on the host twin or on a handle's device; the three give the same bits.
"""
import ctypes as C
import math
import time
from typing import List

import numpy as np

from . import abi
from . import reachability as R

MAX_CHAINS = 16  # PDMPC_HDV_MAX_CHAINS
MAP_SLOTS = 8  # PDMPC_HDV_MAP_SLOTS
CLOSEST_BAND = 0.1  # map_position_to_closest_lanelets.m:4 (added to a distance; the reference calls it "squared")
POINT_TOLERANCE = 1e-6  # is_hdv_behind.m:6
LONGITUDINAL, MERGING, FORKING = 1, 3, 4  # LaneletRelationshipType.m (road_network.RELATIONSHIP_*)


class HdvMap:
    """The map the HDV functions read: per lanelet (id - 1) its left and right points (P, 2), its successor ids in the map's order, and
    the relationship-type table (n, n) uint8 read at (min id, max id)."""

    def __init__(self, left, right, successors, relationship):
        self.left = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 2) for p in left]
        self.right = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 2) for p in right]
        self.centre = [0.5 * (l + r) for l, r in zip(self.left, self.right)]  # RoadDataCommonRoad.m:57-58
        self.successors = [[int(s) for s in row] for row in successors]
        self.relationship = np.ascontiguousarray(relationship, dtype=np.uint8)
        self.n = len(self.left)
        assert self.relationship.shape == (self.n, self.n)

    def arrays(self):
        """-> the arguments of pdmpc_upload_hdv_map / pdmpc_hdv_traffic_host up to the relationship table, and what keeps them alive"""
        off = np.zeros(self.n + 1, dtype=np.int32)
        off[1:] = np.cumsum([p.shape[0] for p in self.left])
        lx, ly = (np.ascontiguousarray(np.concatenate([p[:, c] for p in self.left])) for c in (0, 1))
        rx, ry = (np.ascontiguousarray(np.concatenate([p[:, c] for p in self.right])) for c in (0, 1))
        so = np.zeros(self.n + 1, dtype=np.int32)
        so[1:] = np.cumsum([len(s) for s in self.successors])
        si = np.array([s for row in self.successors for s in row] + [0], dtype=np.int32)
        keep = (off, lx, ly, rx, ry, so, si, self.relationship)
        return [self.n, abi.i32p(off), abi.i32p(off), abi.dp(lx), abi.dp(ly), abi.dp(rx), abi.dp(ry), abi.i32p(so), abi.i32p(si), abi.u8p(self.relationship)], keep


def lab_hdv_map() -> HdvMap:
    """The lab map's lanelets, successors and relationship types (road_network.lanelet_relationship_types)."""
    from .road_network import lab_map, lanelet_relationship_types

    m = lab_map()
    return HdvMap([lan[:, 2:4] for lan in m.lanelets], [lan[:, 0:2] for lan in m.lanelets], [[s for s in row if s] for row in m.succ], lanelet_relationship_types(m))


def scenario_hdv_map(scenario) -> HdvMap:
    """The map the native controller's HDV stage reads: the scenario's per-lanelet left / right points (scenario.lanelet_boundary, what
    pdmpc_scenario carries) with the lab map's successors and relationship types."""
    from .road_network import lab_map, lanelet_relationship_types

    m = lab_map()
    return HdvMap([b[0] for b in scenario.lanelet_boundary], [b[1] for b in scenario.lanelet_boundary], [[s for s in row if s] for row in m.succ],
                  lanelet_relationship_types(m))


def lanelet_distances(hmap: HdvMap, px: float, py: float) -> np.ndarray:
    """d_i of map_position_to_closest_lanelets.m:8-15: the smallest distance from (px, py) to a centre point of every lanelet."""
    d = np.empty(hmap.n)
    for i, c in enumerate(hmap.centre):
        ex, ey = c[:, 0] - px, c[:, 1] - py
        d[i] = np.min(np.sqrt(ex * ex + ey * ey))
    return d


def closest_scan(d) -> List[int]:
    """map_position_to_closest_lanelets.m:17-22: order-dependent on purpose."""
    best, out = math.inf, []
    for i, di in enumerate(np.asarray(d).tolist()):
        if di < best:
            best, out = di, [i + 1]
        elif di <= best + CLOSEST_BAND:
            out.append(i + 1)
    return out


def closest_lanelets(hmap: HdvMap, x: float, y: float, dx: float = 0.0, dy: float = 0.0) -> List[int]:
    return closest_scan(lanelet_distances(hmap, x - dx, y - dy))


def chains(hmap: HdvMap, closest) -> List[tuple]:
    """(id, successor) for every successor of every closest lanelet, (id, 0) for one without successor."""
    return [(i, s) for i in closest for s in (hmap.successors[i - 1] or [0])]


def chain_polygon(hmap: HdvMap, lanelet: int, successor: int, dx: float = 0.0, dy: float = 0.0) -> np.ndarray:
    """The raw chain polygon (2, N): left(id) ++ left(successor), then reversed(right(id) ++ right(successor)), moved by (dx, dy)."""
    ids = [lanelet] + ([successor] if successor else [])
    left = np.vstack([hmap.left[i - 1] for i in ids])
    right = np.vstack([hmap.right[i - 1] for i in ids])
    p = np.vstack([left, right[::-1]])
    return np.array([p[:, 0] + dx, p[:, 1] + dy])


def _sets_at_direction(local_sets, x, y, c, s, trim):
    """reachability.reachable_sets_at_pose with the direction (c, s) as it is in place of the cosine and sine of a yaw (translate_global's
    arithmetic: pdmpc_move_point)"""
    out = []
    for h in local_sets[trim - 1]:
        xl, yl = np.asarray(h[0], dtype=np.float64), np.asarray(h[1], dtype=np.float64)
        gx, gy = c * xl + (-s) * yl + x, s * xl + c * yl + y
        out.append(np.array([np.append(gx, gx[0]), np.append(gy, gy[0])]))
    return out


def reachable_lane(local_sets, x, y, yaw, trim, raw_chain, cos_sin=None):
    """The Hp sets of one row: K ∩ L by pdmpc.reachability.bound_reachable_sets, closed (2, c); (2, 0) where the intersection is empty
    -> (sets, flags).  cos_sin: the HDV's direction as it is (a driver step's), in place of yaw."""
    at = R.reachable_sets_at_pose(local_sets, x, y, yaw, trim) if cos_sin is None else _sets_at_direction(local_sets, x, y, cos_sin[0], cos_sin[1], trim)
    sets, flags = R.bound_reachable_sets(at, raw_chain)
    return [np.zeros((2, 0)) if f & R.BOUND_RESTORED else s for s, f in zip(sets, flags)], flags


def _differ(a, b):
    dx, dy = float(a[0]) - float(b[0]), float(a[1]) - float(b[1])
    return math.sqrt(dx * dx + dy * dy) > POINT_TOLERANCE


def is_hdv_behind(hmap: HdvMap, lanelet_cav: int, cav_xy, closest, hdv_xy, hdv_yaw, cos_sin=None) -> bool:
    """is_hdv_behind.m:13-92 with the CAV's own position and without the assert :64.  cos_sin: the HDV's direction in place of hdv_yaw."""
    hc, hs = (math.cos(hdv_yaw), math.sin(hdv_yaw)) if cos_sin is None else cos_sin
    on_predecessor = on_overlapping = False
    for lanelet_hdv in closest:
        t = int(hmap.relationship[min(lanelet_cav, lanelet_hdv) - 1, max(lanelet_cav, lanelet_hdv) - 1])
        if t in (MERGING, FORKING):
            on_overlapping = True
            continue
        if t != LONGITUDINAL:
            continue
        s, e = lanelet_cav - 1, lanelet_hdv - 1
        if _differ(hmap.centre[s][0], hmap.centre[e][-1]) and _differ(hmap.left[s][0], hmap.right[e][-1]) and _differ(hmap.right[s][0], hmap.left[e][-1]):
            continue
        on_predecessor = True
    if on_predecessor:
        return True
    if lanelet_cav in closest or on_overlapping:
        vx, vy = float(hdv_xy[0]) - float(cav_xy[0]), float(hdv_xy[1]) - float(cav_xy[1])
        if hc * vx + hs * vy < 0.0:
            return True
    return False


def hdv_traffic(hmap: HdvMap, local_sets, hdv_x, hdv_y, hdv_yaw, hdv_trim, hdv_tile, cav_x, cav_y, cav_lanelet, cav_tile, cos_sin=None):
    """update_hdv_traffic_info for HDVs at (x, y, yaw) in trim (1-based) on the map copy moved by hdv_tile[h] = (dx, dy), and CAVs at
    (x, y) on lanelet cav_lanelet of the copy moved by cav_tile[v] -> dict: closest [hdv] id lists, row_hdv [row], sets [row][k]
    closed (2, c) arrays ((2, 0): empty), flags (rows, Hp) uint8, adjacency (n_cav, n_hdv) uint8.  cos_sin: (cos_yaw, sin_yaw) lists as
    they are -- the directions a driver step gives -- in place of the cosines and sines of hdv_yaw."""
    n_hdv, n_cav = len(hdv_x), len(cav_x)
    cs = [None] * n_hdv if cos_sin is None else [(float(cos_sin[0][h]), float(cos_sin[1][h])) for h in range(n_hdv)]
    closest, row_hdv, sets, flags = [], [], [], []
    for h in range(n_hdv):
        dx, dy = float(hdv_tile[h][0]), float(hdv_tile[h][1])
        lst = closest_lanelets(hmap, float(hdv_x[h]), float(hdv_y[h]), dx, dy)
        closest.append(lst)
        ch = chains(hmap, lst)
        if len(lst) > MAX_CHAINS or len(ch) > MAX_CHAINS:
            raise OverflowError("HDV %d has more than %d closest lanelets or chains" % (h, MAX_CHAINS))
        for lanelet, successor in ch:
            s, f = reachable_lane(local_sets, float(hdv_x[h]), float(hdv_y[h]), float(hdv_yaw[h]), int(hdv_trim[h]), chain_polygon(hmap, lanelet, successor, dx, dy), cs[h])
            row_hdv.append(h)
            sets.append(s)
            flags.append(f)
    adjacency = np.zeros((n_cav, n_hdv), dtype=np.uint8)
    for v in range(n_cav):
        for h in range(n_hdv):
            if float(cav_tile[v][0]) == float(hdv_tile[h][0]) and float(cav_tile[v][1]) == float(hdv_tile[h][1]):
                adjacency[v, h] = not is_hdv_behind(hmap, int(cav_lanelet[v]), (cav_x[v], cav_y[v]), closest[h], (hdv_x[h], hdv_y[h]), float(hdv_yaw[h]), cs[h])
    Hp = len(local_sets[0])
    return dict(closest=closest, row_hdv=row_hdv, sets=sets, flags=np.array(flags, dtype=np.uint8).reshape(len(sets), Hp), adjacency=adjacency)


def cav_rows(result, v: int) -> List[List[np.ndarray]]:
    """What CAV v's search receives (vectorize_all_obstacles.m:33-62, IterationData.filter :113): the rows of every HDV adjacent to it,
    in row order -> hdv_reachable_sets [row][k]."""
    return [result["sets"][r] for r, h in enumerate(result["row_hdv"]) if result["adjacency"][v, h]]


# ---- the native calls (include/pdmpc.h: human-driven vehicles)


def lanelet_distances_native(hmap: HdvMap, px: float, py: float) -> np.ndarray:
    """pdmpc_hdv_lanelet_distances_host."""
    from . import backend

    L = backend.load_library()
    args, keep = hmap.arrays()
    d = np.zeros(hmap.n)
    rc = L.pdmpc_hdv_lanelet_distances_host(*args[:7], float(px), float(py), abi.dp(d))
    del keep
    backend._check(L, rc, "pdmpc_hdv_lanelet_distances_host", last_error=None)
    return d


def upload_hdv_map(handle, hmap: HdvMap, local_sets, slot: int = 0):
    """pdmpc_upload_hdv_map_slot: the map and the HDV automaton's local sets ([trim][k] (2, m) hulls) into map slot `slot` of the
    handle (slot 0: pdmpc_upload_hdv_map, what pdmpc_hdv_traffic reads)."""
    from . import backend

    L = backend.load_library()
    args, keep = hmap.arrays()
    ps, pkeep = backend.pack_local_sets(local_sets)
    rc = L.pdmpc_upload_hdv_map_slot(handle.h, int(slot), *args, len(local_sets), len(local_sets[0]), C.byref(ps))
    del keep, pkeep
    backend._check(L, rc, "pdmpc_upload_hdv_map_slot")
    if slot == 0:
        handle.hdv_shape = (hmap.n, len(local_sets[0]))


def hdv_map_slot_state(handle, slot: int = 0):
    """pdmpc_hdv_map_slot_state -> (generation of the slot, uploads into all slots of the handle so far)"""
    from . import backend

    L = backend.load_library()
    gen, ups = C.c_int64(0), C.c_int64(0)
    backend._check(L, L.pdmpc_hdv_map_slot_state(handle.h, int(slot), C.byref(gen), C.byref(ups), None), "pdmpc_hdv_map_slot_state")
    return int(gen.value), int(ups.value)


def hdv_map_slot_hp(handle, slot: int = 0) -> int:
    """The Hp of the hulls map slot `slot` of the handle holds, whoever uploaded them (pdmpc_hdv_map_slot_state); 0: the slot is empty."""
    from . import backend

    L = backend.load_library()
    hp = C.c_int32(0)
    backend._check(L, L.pdmpc_hdv_map_slot_state(handle.h, int(slot), None, None, C.byref(hp)), "pdmpc_hdv_map_slot_state")
    return int(hp.value)


def hdv_map_slot_holds(handle, slot: int, hmap: HdvMap, local_sets) -> bool:
    """pdmpc_hdv_map_slot_holds: does the slot hold exactly this map and these local sets, byte for byte?"""
    from . import backend

    L = backend.load_library()
    args, keep = hmap.arrays()
    ps, pkeep = backend.pack_local_sets(local_sets)
    holds = C.c_int32(0)
    rc = L.pdmpc_hdv_map_slot_holds(handle.h, int(slot), *args, len(local_sets), len(local_sets[0]), C.byref(ps), C.byref(holds))
    del keep, pkeep
    backend._check(L, rc, "pdmpc_hdv_map_slot_holds")
    return bool(holds.value)


def grouped_layout(hdv_offset, cav_offset, Hp: int):
    """pdmpc_hdv_grouped_layout_host -> dict of the block starts (arrays of n_groups + 1 entries, the last the room the array needs):
    closest (closest_offset), lists (closest_index, row_hdv), set_offset, sets (set_flags), adjacency."""
    from . import backend

    L = backend.load_library()
    ho, co = np.ascontiguousarray(hdv_offset, dtype=np.int32), np.ascontiguousarray(cav_offset, dtype=np.int32)
    G = ho.size - 1
    out = {k: np.zeros(G + 1, dtype=np.int32) for k in ("closest", "lists", "set_offset", "sets")}
    out["adjacency"] = np.zeros(G + 1, dtype=np.int64)
    rc = L.pdmpc_hdv_grouped_layout_host(G, abi.i32p(ho), abi.i32p(co), int(Hp), abi.i32p(out["closest"]), abi.i32p(out["lists"]), abi.i32p(out["set_offset"]),
                                         abi.i32p(out["sets"]), out["adjacency"].ctypes.data_as(C.POINTER(C.c_int64)))
    backend._check(L, rc, "pdmpc_hdv_grouped_layout_host", last_error=None)
    return out


def hdv_traffic_grouped_native(handle, groups, capacity=None, call_ms=None, raw=None, guard=0):
    """pdmpc_hdv_traffic_grouped on `handle`'s device.  groups: one (slot, hdv_x, hdv_y, hdv_yaw, hdv_trim, hdv_tile, cav_x, cav_y,
    cav_lanelet, cav_tile) per group, the arguments of hdv_traffic behind the map slot the group drives on.  capacity None: a first
    call sizes a second one; a number: ONE call with that room for the vertices of all groups, which raises backend.CapacityError
    (count = the vertices needed) if it is too small.  raw: a dict that receives the call's arrays as it left them (set_base, n_rows,
    set_offset, set_x, set_y, ... and `layout`), also when the call fails; guard: entries kept behind the `capacity` entries of set_x /
    set_y (NaN before the call).  -> per group the dict of hdv_traffic, sliced by pdmpc_hdv_grouped_layout_host; None for a group
    whose HDV ran over its lists (the call then raises unless raw is given)."""
    from . import backend

    L = backend.load_library()
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)  # noqa: E731
    cat = lambda parts, dtype: np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=dtype).reshape(-1) for p in parts] + [np.zeros(0, dtype=dtype)]))  # noqa: E731
    G = len(groups)
    slot = i32([g[0] for g in groups])
    ho = np.zeros(G + 1, dtype=np.int32)
    co = np.zeros(G + 1, dtype=np.int32)
    for g, grp in enumerate(groups):
        ho[g + 1] = ho[g] + len(f64(grp[1]))
        co[g + 1] = co[g] + len(f64(grp[6]))
    x, y, yaw = (cat([g[i] for g in groups], np.float64) for i in (1, 2, 3))
    trim = cat([g[4] for g in groups], np.int32)
    tile = cat([g[5] for g in groups], np.float64).reshape(-1, 2)
    c = np.array([math.cos(float(a)) for a in yaw], dtype=np.float64)  # the host's libm, as the Python twin moves the sets
    s = np.array([math.sin(float(a)) for a in yaw], dtype=np.float64)
    tdx, tdy = np.ascontiguousarray(tile[:, 0]), np.ascontiguousarray(tile[:, 1])
    cx, cy = (cat([g[i] for g in groups], np.float64) for i in (6, 7))
    cl = cat([g[8] for g in groups], np.int32)
    ctile = cat([g[9] for g in groups], np.float64).reshape(-1, 2)
    cdx, cdy = np.ascontiguousarray(ctile[:, 0]), np.ascontiguousarray(ctile[:, 1])
    # the arrays are sized by the Hp the handle itself reports for the groups' slots (a controller's traffic stage uploads maps too); an
    # empty slot, a slot out of range and slots of different Hp are refused by the call before it writes anything
    in_range = [int(k) for k in slot if 0 <= int(k) < MAP_SLOTS]
    Hp = max([hdv_map_slot_hp(handle, k) for k in in_range] + [1])
    lay = grouped_layout(ho, co, Hp)
    closest_offset = np.zeros(max(int(lay["closest"][G]), 1), dtype=np.int32)
    closest_index = np.zeros(max(int(lay["lists"][G]), 1), dtype=np.int32)
    row_hdv = np.zeros(max(int(lay["lists"][G]), 1), dtype=np.int32)
    set_offset = np.zeros(max(int(lay["set_offset"][G]), 1), dtype=np.int32)
    flags = np.zeros(max(int(lay["sets"][G]), 1), dtype=np.uint8)
    adjacency = np.zeros(max(int(lay["adjacency"][G]), 1), dtype=np.uint8)
    n_rows = np.zeros(max(G, 1), dtype=np.int32)
    set_base = np.zeros(G + 1, dtype=np.int32)
    head = [handle.h, G, abi.i32p(slot), abi.i32p(ho), abi.i32p(co), abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), abi.i32p(trim), abi.dp(tdx), abi.dp(tdy), abi.dp(cx),
            abi.dp(cy), abi.i32p(cl), abi.dp(cdx), abi.dp(cdy), abi.i32p(closest_offset), abi.i32p(closest_index)]

    def call(cap):
        sx, sy = np.full(max(cap, 1) + guard, np.nan), np.full(max(cap, 1) + guard, np.nan)
        tail = [cap, abi.i32p(n_rows), abi.i32p(row_hdv), abi.i32p(set_offset), abi.i32p(set_base), abi.dp(sx), abi.dp(sy), abi.u8p(flags), abi.u8p(adjacency)]
        t0 = time.perf_counter()
        rc = L.pdmpc_hdv_traffic_grouped(*head, *tail)
        if call_ms is not None:
            call_ms.append(1e3 * (time.perf_counter() - t0))
        return rc, sx, sy

    cap = 0 if capacity is None else int(capacity)
    rc, sx, sy = call(cap)
    sized = rc == backend.ERR_CAPACITY and int(set_base[G]) > cap  # (the totals are there: they size a second call)
    if sized and capacity is None:
        cap = int(set_base[G])
        rc, sx, sy = call(cap)
    if raw is not None:
        raw.update(rc=rc, layout=lay, closest_offset=closest_offset, closest_index=closest_index, n_rows=n_rows[:G].copy(), row_hdv=row_hdv, set_offset=set_offset,
                   set_base=set_base.copy(), set_x=sx, set_y=sy, set_flags=flags, adjacency=adjacency, Hp=Hp)
    if sized and capacity is not None and rc == backend.ERR_CAPACITY and raw is None:
        raise backend.CapacityError("pdmpc_hdv_traffic_grouped: %d vertices do not fit the capacity %d" % (int(set_base[G]), capacity), int(set_base[G]))
    if raw is None:
        backend._check(L, rc, "pdmpc_hdv_traffic_grouped")
    out = []
    for g in range(G):
        rows, nh, ncv = int(n_rows[g]), int(ho[g + 1] - ho[g]), int(co[g + 1] - co[g])
        if rows < 0:
            out.append(None)
            continue
        cof = closest_offset[lay["closest"][g] : lay["closest"][g] + nh + 1]
        cidx = closest_index[lay["lists"][g] :]
        so = set_offset[lay["set_offset"][g] : lay["set_offset"][g] + rows * Hp + 1].copy()
        b = int(set_base[g])
        gx, gy = sx[b:], sy[b:]
        fits = int(set_base[G]) <= cap
        sets = [[np.array([gx[so[r * Hp + k] : so[r * Hp + k + 1]], gy[so[r * Hp + k] : so[r * Hp + k + 1]]]) for k in range(Hp)] for r in range(rows)] if fits else None
        a0 = int(lay["adjacency"][g])
        out.append(dict(closest=[cidx[cof[q] : cof[q + 1]].tolist() for q in range(nh)], row_hdv=row_hdv[lay["lists"][g] : lay["lists"][g] + rows].tolist(), sets=sets,
                        flags=flags[lay["sets"][g] : lay["sets"][g] + rows * Hp].reshape(rows, Hp).copy(), adjacency=adjacency[a0 : a0 + ncv * nh].reshape(ncv, nh).copy(),
                        set_offset=so))
    return out


def hdv_traffic_native(hmap, local_sets, hdv_x, hdv_y, hdv_yaw, hdv_trim, hdv_tile, cav_x, cav_y, cav_lanelet, cav_tile, handle=None, capacity=None, call_ms=None, cos_sin=None):
    """pdmpc_hdv_traffic on `handle`'s device (after upload_hdv_map; hmap and local_sets are not read then) or, without a handle,
    pdmpc_hdv_traffic_host.  capacity None: a first call sizes a second one; a number: ONE call with that room, which raises
    backend.CapacityError(count = the vertices needed) if it is too small.  call_ms: a list that receives the wall time (ms) of every
    native call, without the packing around it.  cos_sin: (cos_yaw, sin_yaw) as they are, in place of the cosines and sines of hdv_yaw.
    -> the dict of hdv_traffic."""
    from . import backend

    L = backend.load_library()
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)  # noqa: E731
    x, y, yaw, trim = f64(hdv_x), f64(hdv_y), f64(hdv_yaw), i32(hdv_trim)
    n_hdv = x.size
    c = np.array([math.cos(float(a)) for a in yaw], dtype=np.float64)  # the host's libm, as the Python twin moves the sets
    s = np.array([math.sin(float(a)) for a in yaw], dtype=np.float64)
    if cos_sin is not None:  # (the directions a driver step gives: hdv_yaw is not read)
        c, s = f64(cos_sin[0]), f64(cos_sin[1])
    tile = f64(hdv_tile).reshape(-1, 2)
    tdx, tdy = np.ascontiguousarray(tile[:, 0]), np.ascontiguousarray(tile[:, 1])
    cx, cy, cl = f64(cav_x), f64(cav_y), i32(cav_lanelet)
    n_cav = cx.size
    ctile = f64(cav_tile).reshape(-1, 2)
    cdx, cdy = np.ascontiguousarray(ctile[:, 0]), np.ascontiguousarray(ctile[:, 1])
    Hp = handle.hdv_shape[1] if handle is not None else len(local_sets[0])
    lists = max(n_hdv * MAX_CHAINS, 1)
    closest_offset = np.zeros(n_hdv + 1, dtype=np.int32)
    closest_index = np.zeros(lists, dtype=np.int32)
    n_rows = np.zeros(1, dtype=np.int32)
    row_hdv = np.zeros(lists, dtype=np.int32)
    set_offset = np.zeros(lists * Hp + 1, dtype=np.int32)
    flags = np.zeros(lists * Hp, dtype=np.uint8)
    adjacency = np.zeros(max(n_cav * n_hdv, 1), dtype=np.uint8)
    head = [n_hdv, abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), abi.i32p(trim), abi.dp(tdx), abi.dp(tdy), n_cav, abi.dp(cx), abi.dp(cy), abi.i32p(cl), abi.dp(cdx),
            abi.dp(cdy), abi.i32p(closest_offset), abi.i32p(closest_index)]
    if handle is None:
        margs, mkeep = hmap.arrays()
        ps, pkeep = backend.pack_local_sets(local_sets)
        fn = lambda *tail: L.pdmpc_hdv_traffic_host(*margs, len(local_sets), Hp, C.byref(ps), *head, *tail)  # noqa: E731
        what, last = "pdmpc_hdv_traffic_host", None
    else:
        fn = lambda *tail: L.pdmpc_hdv_traffic(handle.h, *head, *tail)  # noqa: E731
        what, last = "pdmpc_hdv_traffic", "pdmpc_last_error"

    def call(cap):
        sx, sy = np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
        tail = [cap, abi.i32p(n_rows), abi.i32p(row_hdv), abi.i32p(set_offset), abi.dp(sx), abi.dp(sy), abi.u8p(flags), abi.u8p(adjacency)]
        t0 = time.perf_counter()
        rc = fn(*tail)
        if call_ms is not None:
            call_ms.append(1e3 * (time.perf_counter() - t0))
        return rc, sx, sy

    rc, sx, sy = call(0 if capacity is None else int(capacity))
    rows = int(n_rows[0])
    if rc == backend.ERR_CAPACITY and rows >= 0:
        total = int(set_offset[rows * Hp])
        if capacity is not None:
            raise backend.CapacityError("%s: %d vertices do not fit the capacity %d" % (what, total, capacity), total)
        rc, sx, sy = call(total)
    backend._check(L, rc, what, last_error=last)
    rows = int(n_rows[0])
    sets = [[np.array([sx[set_offset[r * Hp + k] : set_offset[r * Hp + k + 1]], sy[set_offset[r * Hp + k] : set_offset[r * Hp + k + 1]]]) for k in range(Hp)]
            for r in range(rows)]
    return dict(closest=[closest_index[closest_offset[h] : closest_offset[h + 1]].tolist() for h in range(n_hdv)], row_hdv=row_hdv[:rows].tolist(), sets=sets,
                flags=flags[: rows * Hp].reshape(rows, Hp).copy(), adjacency=adjacency[: n_cav * n_hdv].reshape(n_cav, n_hdv).copy(), set_offset=set_offset[: rows * Hp + 1].copy())


def hdv_kernel_ms(handle) -> float:
    """kernel time (ms) of the handle's last pdmpc_hdv_traffic"""
    from . import backend

    L = backend.load_library()
    ms = C.c_double(0.0)
    backend._check(L, L.pdmpc_hdv_kernel_ms(handle.h, C.byref(ms)), "pdmpc_hdv_kernel_ms")
    return float(ms.value)


# ---- the driver model (include/pdmpc_hdv.h: "the driver model"; csrc/hdv_drive_host.hpp): an HDV follows a route of lanelets along their
# centre lines and keeps a gap to the vehicle ahead.  Python floats are IEEE doubles and math.sqrt is the IEEE square root, so `drive`
# gives the bits of pdmpc_hdv_drive_host and of the kernel, operation by operation.

ROUTE_MAX, WINDOW_MAX, WALK_MAX = 64, 64, 4096  # PDMPC_HDV_ROUTE_MAX, PDMPC_HDV_WINDOW_MAX, PDMPC_HDV_WALK_MAX
DRIVE_DEFAULTS = (2.0, 0.3, 1.0, 0.125)  # look_ahead, gap_min, headway, lateral (PDMPC_HDV_*_DEFAULT)


def route_from_loop(path_id: int):
    """The closed route of a lab-map loop: the lanelets of get_reference_lanelets_loop(path_id) -> (ids, True)"""
    from .road_network import get_reference_lanelets_loop

    return [int(i) for i in get_reference_lanelets_loop(path_id)], True


def _route_segments(hmap, ids, closed, r):
    return hmap.centre[ids[r] - 1].shape[0] - 1 + (1 if closed or r < len(ids) - 1 else 0)


def _route_segment(hmap, ids, closed, r, j):
    """segment (r, j) -> (ax, ay, dx, dy, len)"""
    c = hmap.centre[ids[r] - 1]
    ax, ay = float(c[j, 0]), float(c[j, 1])
    if j + 1 < c.shape[0]:
        bx, by = float(c[j + 1, 0]), float(c[j + 1, 1])
    else:
        n = hmap.centre[ids[r + 1 if r + 1 < len(ids) else 0] - 1]
        bx, by = float(n[0, 0]), float(n[0, 1])
    dx, dy = bx - ax, by - ay
    return ax, ay, dx, dy, math.sqrt(dx * dx + dy * dy)


def _route_next(hmap, ids, closed, r, j):
    """the segment behind (r, j), or None at the end of an open route"""
    nr, nj = r, j + 1
    for _ in range(len(ids) + 1):
        if nj < _route_segments(hmap, ids, closed, nr):
            return nr, nj
        nj, nr = 0, nr + 1
        if nr == len(ids):
            if not closed:
                return None
            nr = 0
    return None


def check_route(hmap: HdvMap, ids, closed, h: int = 0):
    """hdv_check_routes for one route: raises ValueError naming the HDV and the position"""
    who = "HDV %d: " % h
    n = len(ids)
    if n < 1 or n > ROUTE_MAX:
        raise ValueError(who + "a route of %d lanelets (1 .. PDMPC_HDV_ROUTE_MAX)" % n)
    for r, i in enumerate(ids):
        if i < 1 or i > hmap.n:
            raise ValueError(who + "route position %d: lanelet id %d out of range" % (r, i))
    for r in range(n):
        if r == n - 1 and not closed:
            break
        to = ids[r + 1 if r + 1 < n else 0]
        if to not in hmap.successors[ids[r] - 1]:
            raise ValueError(who + "route position %d: lanelet %d is no successor of lanelet %d" % (r + 1 if r + 1 < n else 0, to, ids[r]))
    if not any(_route_segment(hmap, ids, closed, r, j)[4] > 0.0 for r in range(n) for j in range(_route_segments(hmap, ids, closed, r))):
        raise ValueError(who + "a route without a segment of positive length")


def walk(hmap, ids, closed, state, distance):
    """pdmpc_hdv_walk: `distance` metres forward from state (r, j, u) -> ((r, j, u), 1 if the end of an open route stopped it)"""
    r, j, u = state
    length = _route_segment(hmap, ids, closed, r, j)[4]
    left = distance
    nr, nj, passed = r, j, 0
    while True:
        room = length - u
        if left < room:
            return (r, j, u + left), 0
        nxt = 0.0
        while nxt == 0.0:
            if passed == WALK_MAX:  # the cap
                return (r, j, length), 0
            step = _route_next(hmap, ids, closed, nr, nj)
            if step is None:  # the end of an open route
                return (r, j, length), 1
            nr, nj = step
            passed += 1
            nxt = _route_segment(hmap, ids, closed, nr, nj)[4]
        left = left - room
        r, j, u, length = nr, nj, 0.0, nxt


def state_pose(hmap, ids, closed, state, tile=(0.0, 0.0)):
    """pdmpc_hdv_state_pose -> (x, y, cos_yaw, sin_yaw)"""
    r, j, u = state
    ax, ay, dx, dy, length = _route_segment(hmap, ids, closed, r, j)
    t = u / length
    return ax + t * dx + float(tile[0]), ay + t * dy + float(tile[1]), dx / length, dy / length


def place(hmap, ids, closed, distance):
    """hdv_place: the state `distance` metres from the start of the route"""
    if not (distance >= 0.0) or math.isinf(distance):
        raise ValueError("a start distance that is negative or not finite")
    at = (0, -1)
    while True:
        at = _route_next(hmap, ids, closed, at[0], at[1])
        if at is None:
            raise ValueError("a route without a segment of positive length")
        if _route_segment(hmap, ids, closed, at[0], at[1])[4] > 0.0:
            break
    state, ended = walk(hmap, ids, closed, (at[0], at[1], 0.0), float(distance))
    if ended:
        raise ValueError("a start distance at or beyond the end of an open route")
    return state


def build_window(hmap, ids, closed, state, look_ahead):
    """pdmpc_hdv_build_window -> [(ax, ay, dx, dy, len, start)]"""
    r, j, u = state
    run = -u
    out = []
    for _ in range(WALK_MAX):
        ax, ay, dx, dy, length = _route_segment(hmap, ids, closed, r, j)
        if length != 0.0:
            out.append((ax, ay, dx, dy, length, run))
            run = run + length
            if len(out) == WINDOW_MAX or run >= look_ahead:
                break
        step = _route_next(hmap, ids, closed, r, j)
        if step is None:
            break
        r, j = step
    return out


def gap_item(window, w, u, px, py, lateral):
    """pdmpc_hdv_gap_item"""
    ax, ay, dx, dy, length, start = window[w]
    qx, qy = px - ax, py - ay
    lo = u / length if w == 0 else 0.0
    t = (qx * dx + qy * dy) / (dx * dx + dy * dy)
    if not (t >= lo):
        t = lo
    if t > 1.0:
        t = 1.0
    ex, ey = qx - t * dx, qy - t * dy
    off = math.sqrt(ex * ex + ey * ey)
    ahead = start + t * length
    return ahead if off <= lateral and ahead > 0.0 else math.inf


def drive_speed(gap, v_des, gap_min, headway):
    s = (gap - gap_min) / headway
    if not (s > 0.0):
        s = 0.0
    return v_des if s > v_des else s


def check_drive(params, dt, v_des):
    """hdv_check_drive"""
    if any(not (float(p) > 0.0) or math.isinf(float(p)) for p in list(params) + [dt]):
        raise ValueError("look_ahead, gap_min, headway, lateral and dt must be positive and finite")
    if params[2] < dt:
        raise ValueError("headway < dt: an HDV could close more than gap - gap_min in one step")
    if any(not (float(v) >= 0.0) or math.isinf(float(v)) for v in v_des):
        raise ValueError("a desired speed that is negative or not finite")


def drive(hmap: HdvMap, routes, states, tiles, v_des, cav_x, cav_y, cav_tile, params=DRIVE_DEFAULTS, dt=0.2):
    """One step of the HDVs of one member (hdv_drive_member): routes [(ids, closed)], states [(r, j, u)], tiles [(dx, dy)], the CAVs at
    (cav_x, cav_y) on the map copies cav_tile.  Gaps are taken from the old states; all HDVs move at once.
    -> dict: states, x, y, cos_yaw, sin_yaw, speed, gap (lists)"""
    n = len(routes)
    look_ahead, gap_min, headway, lateral = (float(p) for p in params)
    old = [state_pose(hmap, routes[q][0], routes[q][1], states[q], tiles[q]) for q in range(n)]
    out = dict(states=[], x=[], y=[], cos_yaw=[], sin_yaw=[], speed=[], gap=[])
    for h in range(n):
        ids, closed = routes[h]
        tdx, tdy = float(tiles[h][0]), float(tiles[h][1])
        W = build_window(hmap, ids, closed, states[h], look_ahead)
        best = math.inf
        others = [(float(cav_x[v]), float(cav_y[v]), cav_tile[v]) for v in range(len(cav_x))] + [(old[q][0], old[q][1], tiles[q]) for q in range(n) if q != h]
        for px, py, tile in others:
            if not (float(tile[0]) == tdx and float(tile[1]) == tdy):
                continue
            for w in range(len(W)):
                ahead = gap_item(W, w, states[h][2], px - tdx, py - tdy, lateral)
                if ahead < best:
                    best = ahead
        speed = drive_speed(best, float(v_des[h]), gap_min, headway)
        state, ended = walk(hmap, ids, closed, states[h], speed * float(dt))
        x, y, c, s = state_pose(hmap, ids, closed, state, tiles[h])
        for key, value in (("states", state), ("x", x), ("y", y), ("cos_yaw", c), ("sin_yaw", s), ("speed", 0.0 if ended else speed), ("gap", best)):
            out[key].append(value)
    return out


def _route_arrays(routes):
    off = np.zeros(len(routes) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(ids) for ids, _ in routes])
    lan = np.array([i for ids, _ in routes for i in ids] + [0], dtype=np.int32)
    closed = np.array([1 if c else 0 for _, c in routes] + [0], dtype=np.uint8)
    return off, lan, closed


def _state_arrays(states):
    n = len(states)
    seg = np.array([s[0] for s in states] + [s[1] for s in states] + [0], dtype=np.int32)
    u = np.array([float(s[2]) for s in states] + [0.0], dtype=np.float64)
    return n, seg, u


def _driven(n, seg, u, x, y, c, s, speed, gap, h0=0, count=None, stride=None):
    count = n if count is None else count
    stride = n if stride is None else stride
    sl = slice(h0, h0 + count)
    return dict(states=[(int(seg[h0 + q]), int(seg[stride + h0 + q]), float(u[h0 + q])) for q in range(count)], x=x[sl].tolist(), y=y[sl].tolist(), cos_yaw=c[sl].tolist(),
                sin_yaw=s[sl].tolist(), speed=speed[sl].tolist(), gap=gap[sl].tolist())


def route_check_native(hmap: HdvMap, routes):
    """pdmpc_hdv_route_check_host: raises backend.BackendError (status -1) with the reason"""
    from . import backend

    L = backend.load_library()
    margs, keep = hmap.arrays()
    off, lan, closed = _route_arrays(routes)
    rc = L.pdmpc_hdv_route_check_host(*margs, len(routes), abi.i32p(off), abi.i32p(lan), abi.u8p(closed))
    del keep
    backend._check(L, rc, "pdmpc_hdv_route_check_host")


def place_native(hmap: HdvMap, routes, start_distance, tiles):
    """pdmpc_hdv_place_host -> (states, x, y, cos_yaw, sin_yaw)"""
    from . import backend

    L = backend.load_library()
    margs, keep = hmap.arrays()
    off, lan, closed = _route_arrays(routes)
    n = len(routes)
    d = np.array([float(v) for v in start_distance] + [0.0])
    tile = np.asarray(list(tiles) + [(0.0, 0.0)], dtype=np.float64).reshape(-1, 2)
    tdx, tdy = np.ascontiguousarray(tile[:, 0]), np.ascontiguousarray(tile[:, 1])
    seg, u = np.zeros(2 * n + 1, dtype=np.int32), np.zeros(n + 1)
    x, y, c, s = (np.zeros(n + 1) for _ in range(4))
    rc = L.pdmpc_hdv_place_host(*margs, n, abi.i32p(off), abi.i32p(lan), abi.u8p(closed), abi.dp(d), abi.dp(tdx), abi.dp(tdy), abi.i32p(seg), abi.dp(u), abi.dp(x), abi.dp(y),
                                abi.dp(c), abi.dp(s))
    del keep
    backend._check(L, rc, "pdmpc_hdv_place_host")
    return [(int(seg[q]), int(seg[n + q]), float(u[q])) for q in range(n)], x[:n].tolist(), y[:n].tolist(), c[:n].tolist(), s[:n].tolist()


def drive_native(hmap: HdvMap, routes, states, tiles, v_des, cav_x, cav_y, cav_tile, params=DRIVE_DEFAULTS, dt=0.2):
    """pdmpc_hdv_drive_host -> the dict of drive"""
    from . import backend

    L = backend.load_library()
    margs, keep = hmap.arrays()
    off, lan, closed = _route_arrays(routes)
    n, seg, u = _state_arrays(states)
    tile = np.asarray(list(tiles) + [(0.0, 0.0)], dtype=np.float64).reshape(-1, 2)
    tdx, tdy = np.ascontiguousarray(tile[:, 0]), np.ascontiguousarray(tile[:, 1])
    v = np.array([float(a) for a in v_des] + [0.0])
    cx, cy = np.array([float(a) for a in cav_x] + [0.0]), np.array([float(a) for a in cav_y] + [0.0])
    ctile = np.asarray(list(cav_tile) + [(0.0, 0.0)], dtype=np.float64).reshape(-1, 2)
    cdx, cdy = np.ascontiguousarray(ctile[:, 0]), np.ascontiguousarray(ctile[:, 1])
    par = np.array([float(p) for p in params], dtype=np.float64)
    nseg, nu = np.zeros(2 * n + 1, dtype=np.int32), np.zeros(n + 1)
    x, y, c, s, speed, gap = (np.zeros(n + 1) for _ in range(6))
    rc = L.pdmpc_hdv_drive_host(*margs, n, abi.i32p(off), abi.i32p(lan), abi.u8p(closed), abi.i32p(seg), abi.dp(u), abi.dp(tdx), abi.dp(tdy), abi.dp(v), len(cav_x), abi.dp(cx),
                                abi.dp(cy), abi.dp(cdx), abi.dp(cdy), abi.dp(par), float(dt), abi.i32p(nseg), abi.dp(nu), abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), abi.dp(speed),
                                abi.dp(gap))
    del keep
    backend._check(L, rc, "pdmpc_hdv_drive_host")
    return _driven(n, nseg, nu, x, y, c, s, speed, gap)


def _drive_group_arrays(groups):
    """groups: one dict per group -- slot, routes, states, tiles, v_des, cav_x, cav_y, cav_tile, params, dt (drive's arguments behind the
    map slot) -> the arrays of the grouped driver calls over all groups"""
    G = len(groups)
    ho, co = np.zeros(G + 1, dtype=np.int32), np.zeros(G + 1, dtype=np.int32)
    for g, grp in enumerate(groups):
        ho[g + 1] = ho[g] + len(grp["states"])
        co[g + 1] = co[g] + len(grp["cav_x"])
    routes = [r for grp in groups for r in (grp["routes"] if grp.get("routes") else [([], False)] * len(grp["states"]))]
    states = [s for grp in groups for s in grp["states"]]
    off, lan, closed = _route_arrays(routes)
    n, seg, u = _state_arrays(states)
    flat = lambda key: np.array([float(a) for grp in groups for a in grp[key]] + [0.0])  # noqa: E731
    tile = np.asarray([t for grp in groups for t in grp["tiles"]] + [(0.0, 0.0)], dtype=np.float64).reshape(-1, 2)
    ctile = np.asarray([t for grp in groups for t in grp["cav_tile"]] + [(0.0, 0.0)], dtype=np.float64).reshape(-1, 2)
    par = np.array([float(p) for grp in groups for p in grp.get("params", DRIVE_DEFAULTS)] + [0.0])
    dt = np.array([float(grp.get("dt", 0.2)) for grp in groups] + [0.0])
    return dict(G=G, n=n, slot=np.array([grp["slot"] for grp in groups] + [0], dtype=np.int32), ho=ho, co=co, off=off, lan=lan, closed=closed, seg=seg, u=u,
                tdx=np.ascontiguousarray(tile[:, 0]), tdy=np.ascontiguousarray(tile[:, 1]), v=flat("v_des"), cx=flat("cav_x"), cy=flat("cav_y"),
                cdx=np.ascontiguousarray(ctile[:, 0]), cdy=np.ascontiguousarray(ctile[:, 1]), par=par, dt=dt)


def drive_grouped_native(handle, groups, call_ms=None):
    """pdmpc_hdv_drive_grouped on `handle`'s device (the groups' maps uploaded into their slots) -> per group the dict of drive"""
    from . import backend

    L = backend.load_library()
    A = _drive_group_arrays(groups)
    n = A["n"]
    nseg, nu = np.zeros(2 * n + 1, dtype=np.int32), np.zeros(n + 1)
    x, y, c, s, speed, gap = (np.zeros(n + 1) for _ in range(6))
    args = [handle.h, A["G"], abi.i32p(A["slot"]), abi.i32p(A["ho"]), abi.i32p(A["co"]), abi.i32p(A["off"]), abi.i32p(A["lan"]), abi.u8p(A["closed"]), abi.i32p(A["seg"]),
            abi.dp(A["u"]), abi.dp(A["tdx"]), abi.dp(A["tdy"]), abi.dp(A["v"]), abi.dp(A["cx"]), abi.dp(A["cy"]), abi.dp(A["cdx"]), abi.dp(A["cdy"]), abi.dp(A["par"]),
            abi.dp(A["dt"]), abi.i32p(nseg), abi.dp(nu), abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), abi.dp(speed), abi.dp(gap)]
    t0 = time.perf_counter()
    rc = L.pdmpc_hdv_drive_grouped(*args)
    if call_ms is not None:
        call_ms.append(1e3 * (time.perf_counter() - t0))
    backend._check(L, rc, "pdmpc_hdv_drive_grouped")
    ho = A["ho"]
    return [_driven(n, nseg, nu, x, y, c, s, speed, gap, int(ho[g]), int(ho[g + 1] - ho[g]), n) for g in range(A["G"])]


def drive_traffic_grouped_native(handle, groups, capacity, call_ms=None, raw=None, guard=0):
    """pdmpc_hdv_drive_traffic_grouped on `handle`'s device: ONE call with room for `capacity` vertices.  groups: the dicts of
    drive_grouped_native with `drives` (False: the group keeps the poses x, y, yaw it brings and needs no routes), `trim` and
    `cav_lanelet`.  raw: receives rc and the traffic arrays as the call left them, also when it fails (else a failure raises).
    -> per group (the dict of drive or None for a group that did not drive, the dict of hdv_traffic)"""
    from . import backend

    L = backend.load_library()
    A = _drive_group_arrays(groups)
    G, n, ho, co = A["G"], A["n"], A["ho"], A["co"]
    drives = np.array([1 if grp.get("drives", True) else 0 for grp in groups] + [0], dtype=np.uint8)
    x, y, c, s = (np.zeros(n + 1) for _ in range(4))
    for g, grp in enumerate(groups):
        if not drives[g]:
            for q in range(len(grp["states"])):
                x[ho[g] + q], y[ho[g] + q] = float(grp["x"][q]), float(grp["y"][q])
                c[ho[g] + q], s[ho[g] + q] = math.cos(float(grp["yaw"][q])), math.sin(float(grp["yaw"][q]))
    trim = np.array([int(t) for grp in groups for t in grp["trim"]] + [1], dtype=np.int32)
    cl = np.array([int(t) for grp in groups for t in grp["cav_lanelet"]] + [1], dtype=np.int32)
    nseg, nu, speed, gap = np.zeros(2 * n + 1, dtype=np.int32), np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)
    in_range = [int(k) for k in A["slot"][:G] if 0 <= int(k) < MAP_SLOTS]
    Hp = max([hdv_map_slot_hp(handle, k) for k in in_range] + [1])
    lay = grouped_layout(ho, co, Hp)
    closest_offset = np.zeros(max(int(lay["closest"][G]), 1), dtype=np.int32)
    closest_index = np.zeros(max(int(lay["lists"][G]), 1), dtype=np.int32)
    row_hdv = np.zeros(max(int(lay["lists"][G]), 1), dtype=np.int32)
    set_offset = np.zeros(max(int(lay["set_offset"][G]), 1), dtype=np.int32)
    flags = np.zeros(max(int(lay["sets"][G]), 1), dtype=np.uint8)
    adjacency = np.zeros(max(int(lay["adjacency"][G]), 1), dtype=np.uint8)
    n_rows = np.zeros(max(G, 1), dtype=np.int32)
    set_base = np.zeros(G + 1, dtype=np.int32)
    cap = int(capacity)
    sx, sy = np.full(max(cap, 1) + guard, np.nan), np.full(max(cap, 1) + guard, np.nan)
    args = [handle.h, G, abi.i32p(A["slot"]), abi.i32p(ho), abi.i32p(co), abi.u8p(drives), abi.i32p(A["off"]), abi.i32p(A["lan"]), abi.u8p(A["closed"]), abi.i32p(A["seg"]),
            abi.dp(A["u"]), abi.dp(A["v"]), abi.dp(A["par"]), abi.dp(A["dt"]), abi.i32p(nseg), abi.dp(nu), abi.dp(speed), abi.dp(gap), abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s),
            abi.i32p(trim), abi.dp(A["tdx"]), abi.dp(A["tdy"]), abi.dp(A["cx"]), abi.dp(A["cy"]), abi.i32p(cl), abi.dp(A["cdx"]), abi.dp(A["cdy"]), abi.i32p(closest_offset),
            abi.i32p(closest_index), cap, abi.i32p(n_rows), abi.i32p(row_hdv), abi.i32p(set_offset), abi.i32p(set_base), abi.dp(sx), abi.dp(sy), abi.u8p(flags), abi.u8p(adjacency)]
    t0 = time.perf_counter()
    rc = L.pdmpc_hdv_drive_traffic_grouped(*args)
    if call_ms is not None:
        call_ms.append(1e3 * (time.perf_counter() - t0))
    if raw is not None:
        raw.update(rc=rc, layout=lay, closest_offset=closest_offset, closest_index=closest_index, n_rows=n_rows[:G].copy(), row_hdv=row_hdv, set_offset=set_offset,
                   set_base=set_base.copy(), set_x=sx, set_y=sy, set_flags=flags, adjacency=adjacency, Hp=Hp)
    elif rc == backend.ERR_CAPACITY and int(set_base[G]) > cap:
        raise backend.CapacityError("pdmpc_hdv_drive_traffic_grouped: %d vertices do not fit the capacity %d" % (int(set_base[G]), cap), int(set_base[G]))
    else:
        backend._check(L, rc, "pdmpc_hdv_drive_traffic_grouped")
    out = []
    fits = rc == 0
    for g in range(G):
        rows, nh, ncv = int(n_rows[g]), int(ho[g + 1] - ho[g]), int(co[g + 1] - co[g])
        driven = _driven(n, nseg, nu, x, y, c, s, speed, gap, int(ho[g]), nh, n) if drives[g] else None
        if rows < 0:
            out.append((driven, None))
            continue
        cof = closest_offset[lay["closest"][g] : lay["closest"][g] + nh + 1]
        cidx = closest_index[lay["lists"][g] :]
        so = set_offset[lay["set_offset"][g] : lay["set_offset"][g] + rows * Hp + 1].copy()
        gx, gy = sx[int(set_base[g]) :], sy[int(set_base[g]) :]
        sets = [[np.array([gx[so[r * Hp + k] : so[r * Hp + k + 1]], gy[so[r * Hp + k] : so[r * Hp + k + 1]]]) for k in range(Hp)] for r in range(rows)] if fits else None
        a0 = int(lay["adjacency"][g])
        out.append((driven, dict(closest=[cidx[cof[q] : cof[q + 1]].tolist() for q in range(nh)], row_hdv=row_hdv[lay["lists"][g] : lay["lists"][g] + rows].tolist(), sets=sets,
                                 flags=flags[lay["sets"][g] : lay["sets"][g] + rows * Hp].reshape(rows, Hp).copy(),
                                 adjacency=adjacency[a0 : a0 + ncv * nh].reshape(ncv, nh).copy(), set_offset=so)))
    return out
