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


def reachable_lane(local_sets, x, y, yaw, trim, raw_chain):
    """The Hp sets of one row: K ∩ L by pdmpc.reachability.bound_reachable_sets, closed (2, c); (2, 0) where the intersection is empty
    -> (sets, flags)."""
    sets, flags = R.bound_reachable_sets(R.reachable_sets_at_pose(local_sets, x, y, yaw, trim), raw_chain)
    return [np.zeros((2, 0)) if f & R.BOUND_RESTORED else s for s, f in zip(sets, flags)], flags


def _differ(a, b):
    dx, dy = float(a[0]) - float(b[0]), float(a[1]) - float(b[1])
    return math.sqrt(dx * dx + dy * dy) > POINT_TOLERANCE


def is_hdv_behind(hmap: HdvMap, lanelet_cav: int, cav_xy, closest, hdv_xy, hdv_yaw) -> bool:
    """is_hdv_behind.m:13-92 with the CAV's own position and without the assert :64."""
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
        if math.cos(hdv_yaw) * vx + math.sin(hdv_yaw) * vy < 0.0:
            return True
    return False


def hdv_traffic(hmap: HdvMap, local_sets, hdv_x, hdv_y, hdv_yaw, hdv_trim, hdv_tile, cav_x, cav_y, cav_lanelet, cav_tile):
    """update_hdv_traffic_info for HDVs at (x, y, yaw) in trim (1-based) on the map copy moved by hdv_tile[h] = (dx, dy), and CAVs at
    (x, y) on lanelet cav_lanelet of the copy moved by cav_tile[v] -> dict: closest [hdv] id lists, row_hdv [row], sets [row][k]
    closed (2, c) arrays ((2, 0): empty), flags (rows, Hp) uint8, adjacency (n_cav, n_hdv) uint8."""
    n_hdv, n_cav = len(hdv_x), len(cav_x)
    closest, row_hdv, sets, flags = [], [], [], []
    for h in range(n_hdv):
        dx, dy = float(hdv_tile[h][0]), float(hdv_tile[h][1])
        lst = closest_lanelets(hmap, float(hdv_x[h]), float(hdv_y[h]), dx, dy)
        closest.append(lst)
        ch = chains(hmap, lst)
        if len(lst) > MAX_CHAINS or len(ch) > MAX_CHAINS:
            raise OverflowError("HDV %d has more than %d closest lanelets or chains" % (h, MAX_CHAINS))
        for lanelet, successor in ch:
            s, f = reachable_lane(local_sets, float(hdv_x[h]), float(hdv_y[h]), float(hdv_yaw[h]), int(hdv_trim[h]), chain_polygon(hmap, lanelet, successor, dx, dy))
            row_hdv.append(h)
            sets.append(s)
            flags.append(f)
    adjacency = np.zeros((n_cav, n_hdv), dtype=np.uint8)
    for v in range(n_cav):
        for h in range(n_hdv):
            if float(cav_tile[v][0]) == float(hdv_tile[h][0]) and float(cav_tile[v][1]) == float(hdv_tile[h][1]):
                adjacency[v, h] = not is_hdv_behind(hmap, int(cav_lanelet[v]), (cav_x[v], cav_y[v]), closest[h], (hdv_x[h], hdv_y[h]), float(hdv_yaw[h]))
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


def hdv_traffic_native(hmap, local_sets, hdv_x, hdv_y, hdv_yaw, hdv_trim, hdv_tile, cav_x, cav_y, cav_lanelet, cav_tile, handle=None, capacity=None, call_ms=None):
    """pdmpc_hdv_traffic on `handle`'s device (after upload_hdv_map; hmap and local_sets are not read then) or, without a handle,
    pdmpc_hdv_traffic_host.  capacity None: a first call sizes a second one; a number: ONE call with that room, which raises
    backend.CapacityError(count = the vertices needed) if it is too small.  call_ms: a list that receives the wall time (ms) of every
    native call, without the packing around it.  -> the dict of hdv_traffic."""
    from . import backend

    L = backend.load_library()
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)  # noqa: E731
    x, y, yaw, trim = f64(hdv_x), f64(hdv_y), f64(hdv_yaw), i32(hdv_trim)
    n_hdv = x.size
    c = np.array([math.cos(float(a)) for a in yaw], dtype=np.float64)  # the host's libm, as the Python twin moves the sets
    s = np.array([math.sin(float(a)) for a in yaw], dtype=np.float64)
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
