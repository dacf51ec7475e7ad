"""Loader and thin object wrapper for libpdmpc_hip.so (the C ABI of include/pdmpc.h).

There is deliberately NO CPU fallback: if the shared library is missing or no gfx950 device is
present, construction raises.  The library is built in-tree by `__graft_entry__.build()` /
`make -C p-dmpc_amd/csrc`.
"""
import ctypes as C
import math
import os

import numpy as np

from . import abi
from .abi import ChoiceStruct, FcaGroup  # noqa: F401  (their home; importable from here as before)
from .prototypes import PROTOTYPES, declare

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDMPC_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libpdmpc_hip.so")

_LIB = None

EXPORTS = list(PROTOTYPES)  # every function of include/pdmpc.h
SAMPLED_BUDGET_DEFAULT, SAMPLED_BUDGET_MAX = 250, 16384  # PDMPC_SAMPLED_BUDGET_*
SAMPLED_ENSEMBLE_MAX, SAMPLED_ENSEMBLE_STRIDE = 16, 1000003  # PDMPC_SAMPLED_ENSEMBLE_*
_SAMPLED_EXTRA = ("node_cap", "tree_in_lds", "tree_hbm_bytes", "rand_chunk", "member_bytes", "ensemble_tree_bytes", "grid", "n_members")


def sampled_member_seed(seed, member):
    """pdmpc_sampled_member_seed (no GPU): PDMPC_SAMPLED_MEMBER_SEED of include/pdmpc.h, evaluated by the library."""
    return int(load_library().pdmpc_sampled_member_seed(int(seed) & 0xFFFFFFFF, int(member)))


def sampled_ensemble_plan_host(query, n_expansions_max, n_members, tuning=None):
    """pdmpc_sampled_ensemble_plan_host (no GPU): sampled_plan_host with an ensemble size; the extra dict has 8 entries."""
    L = load_library()
    q, p = abi.LaunchQuery(**query), abi.LaunchPlan()
    x = (C.c_int64 * 8)()
    rc = L.pdmpc_sampled_ensemble_plan_host(tuning.encode() if tuning is not None else None, C.byref(q), int(n_expansions_max), int(n_members), C.byref(p), x)
    plan = {f: getattr(p, f) for f, _ in abi.LaunchPlan._fields_}
    plan["kernel"] = plan["kernel"].decode() if plan["kernel"] else ""
    return rc, plan, dict(zip(_SAMPLED_EXTRA, (int(v) for v in x)))


def sampled_plan_host(query, n_expansions_max, tuning=None):
    """pdmpc_sampled_plan_host (no GPU): the plan of a sampled launch with a budget -> (rc, {field: value} incl. kernel, extra dict)."""
    L = load_library()
    q, p = abi.LaunchQuery(**query), abi.LaunchPlan()
    x = (C.c_int64 * 4)()
    rc = L.pdmpc_sampled_plan_host(tuning.encode() if tuning is not None else None, C.byref(q), int(n_expansions_max), C.byref(p), x)
    plan = {f: getattr(p, f) for f, _ in abi.LaunchPlan._fields_}
    plan["kernel"] = plan["kernel"].decode() if plan["kernel"] else ""
    return rc, plan, dict(zip(("node_cap", "tree_in_lds", "tree_hbm_bytes", "rand_chunk"), (int(v) for v in x)))


class BackendError(RuntimeError):
    pass


class CapacityError(BackendError):
    """PDMPC_ERR_CAPACITY from pdmpc_unique_priorities(_host): `count` is the true number of unique prioritizations (-1 when the
    graph is outside the limits: more than 64 vehicles or 32 coupling edges)."""

    def __init__(self, msg, count, counts=None):
        super().__init__(msg)
        self.count = count
        self.counts = [count] if counts is None else list(counts)  # of a grouped call: every graph's count


ERR_CAPACITY = -4


def unique_priorities_call(adjacency, max_out, handle=None):
    """pdmpc_unique_priorities on `handle`'s device, or pdmpc_unique_priorities_host without one -> (priorities n x K, masks [K]),
    the reference's column layout.  Raises CapacityError for PDMPC_ERR_CAPACITY."""
    L = load_library()
    A = np.ascontiguousarray(np.asarray(adjacency) != 0, dtype=np.uint8)
    n = A.shape[0]
    cap = max(int(max_out), 0)
    masks = np.zeros(max(cap, 1), dtype=np.uint32)
    prio = np.zeros(max(cap, 1) * n, dtype=np.int32)
    K = C.c_int64(0)
    args = [n, abi.u8p(A), cap, C.byref(K), abi.u32p(masks), abi.i32p(prio)]
    if handle is not None:
        rc = L.pdmpc_unique_priorities(handle.h, *args)
        what = "pdmpc_unique_priorities"
    else:
        rc = L.pdmpc_unique_priorities_host(*args)
        what = "pdmpc_unique_priorities_host"
    if rc == ERR_CAPACITY:
        raise CapacityError("%s: capacity (%d unique prioritizations, max_out %d)" % (what, K.value, cap), K.value)
    _check(L, rc, what, last_error="pdmpc_last_error" if handle is not None else None)
    k = K.value
    return prio[: k * n].reshape(k, n).T.astype(np.int64), masks[:k].astype(np.int64)


def unique_priorities_grouped_call(graphs, max_out, handle=None, masks_out=None, priorities_out=None):
    """pdmpc_unique_priorities_grouped on `handle`'s device, or pdmpc_unique_priorities_grouped_host without one: every graph of
    `graphs` in ONE call -> [(priorities n_g x K_g, masks [K_g])] per graph, as unique_priorities_call returns a graph's.  max_out: one
    bound for all graphs or one per graph.  Raises CapacityError for PDMPC_ERR_CAPACITY: `counts` holds every graph's count (-1 outside
    the limits), `count` the first that does not fit.  masks_out / priorities_out (tests): the arrays the call writes into."""
    L = load_library()
    As = [np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8) for a in graphs]
    M = len(As)
    sizes = np.array([a.shape[0] for a in As], dtype=np.int32)
    caps = np.full(M, max_out, dtype=np.int64) if np.isscalar(max_out) else np.ascontiguousarray(max_out, dtype=np.int64)
    if caps.shape != (M,):
        raise ValueError("max_out: one bound, or one per graph")
    room = np.maximum(caps, 0)
    masks = np.zeros(max(int(room.sum()), 1), dtype=np.uint32) if masks_out is None else masks_out
    prio = np.zeros(max(int((room * sizes).sum()), 1), dtype=np.int32) if priorities_out is None else priorities_out
    counts = np.zeros(max(M, 1), dtype=np.int64)
    ptrs = (abi.c_uint8_p * max(M, 1))(*[abi.u8p(a) for a in As])
    args = [M, abi.i32p(sizes), ptrs, caps.ctypes.data_as(C.POINTER(C.c_int64)), counts.ctypes.data_as(C.POINTER(C.c_int64)), abi.u32p(masks), abi.i32p(prio)]
    if handle is not None:
        rc = L.pdmpc_unique_priorities_grouped(handle.h, *args)
        what = "pdmpc_unique_priorities_grouped"
    else:
        rc = L.pdmpc_unique_priorities_grouped_host(*args)
        what = "pdmpc_unique_priorities_grouped_host"
    if rc == ERR_CAPACITY:
        got = [int(k) for k in counts[:M]]
        bad = [k for k, cap in zip(got, caps) if k < 0 or k > cap]
        raise CapacityError("%s: capacity (unique prioritizations %s, max_out %s)" % (what, got, caps.tolist()), bad[0] if bad else -1, got)
    _check(L, rc, what, last_error="pdmpc_last_error" if handle is not None else "pdmpc_controller_last_error")
    out, at, row = [], 0, 0
    for n, k in zip(sizes.tolist(), counts[:M].tolist()):
        out.append((prio[row : row + k * n].reshape(k, n).T.astype(np.int64), masks[at : at + k].astype(np.int64)))
        at += k
        row += k * n
    return out


def local_reachable_sets_native(mpa):
    """pdmpc_local_reachable_sets (csrc/reachable_sets.cpp), the C++ twin of MotionPrimitiveAutomaton.local_reachable_sets_conv
    -> [trim][k] (2, m) arrays."""
    L = load_library()
    s, keep = abi.pack_mpa(mpa)
    n, Hp = mpa.n_trims, mpa.Hp
    off = np.zeros(n * Hp + 1, dtype=np.int32)
    rc = L.pdmpc_local_reachable_sets(C.byref(s), 0, abi.i32p(off), None, None)
    if rc != ERR_CAPACITY:
        _check(L, rc, "pdmpc_local_reachable_sets", last_error=None)
    tot = int(off[-1])
    x = np.zeros(max(tot, 1))
    y = np.zeros(max(tot, 1))
    rc = L.pdmpc_local_reachable_sets(C.byref(s), tot, abi.i32p(off), abi.dp(x), abi.dp(y))
    _check(L, rc, "pdmpc_local_reachable_sets", last_error=None)
    del keep
    return [[np.array([x[off[i * Hp + k] : off[i * Hp + k + 1]], y[off[i * Hp + k] : off[i * Hp + k + 1]]]) for k in range(Hp)] for i in range(n)]


def pack_local_sets(local_sets):
    """[trim][k] (2, m) hulls -> (pdmpc_polygon_set, keep-alive) with polygon trim * Hp + k."""
    keep = abi._Keep()
    return abi.pack_polygon_set([h for row in local_sets for h in row], keep), keep


def _coupling_args(x, y, yaw, trim):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    yaw = np.asarray(yaw, dtype=np.float64)
    c = np.array([math.cos(float(a)) for a in yaw], dtype=np.float64)  # the host's libm, as the Python twin moves the sets
    s = np.array([math.sin(float(a)) for a in yaw], dtype=np.float64)
    t = np.ascontiguousarray(trim, dtype=np.int32)
    return x, y, c, s, t


def _coupling_out(n):
    """The outputs of a coupler, never empty -> (adjacency, areas, a call that returns them as (n, n) arrays)."""
    adj = np.zeros(max(n * n, 1), dtype=np.uint8)
    area = np.zeros(max(n * n, 1), dtype=np.float64)
    return adj, area, lambda: (adj[: n * n].reshape(n, n), area[: n * n].reshape(n, n))


def reachable_set_coupling_call(local_sets, x, y, yaw, trim, handle=None):
    """ReachableSetCoupler.couple natively: on `handle`'s device (pdmpc_reachable_set_coupling; the handle must hold the table, see
    Handle.upload_reachable_sets) or, without one, on the host twin (pdmpc_reachable_set_coupling_host).  trim is 1-based.
    -> (adjacency (n, n) uint8, areas (n, n))."""
    L = load_library()
    x, y, c, s, t = _coupling_args(x, y, yaw, trim)
    n = x.size
    adj, area, shaped = _coupling_out(n)
    ptrs = [abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), abi.i32p(t), abi.u8p(adj), abi.dp(area)]
    if handle is not None:
        _check(L, L.pdmpc_reachable_set_coupling(handle.h, n, *ptrs), "pdmpc_reachable_set_coupling")
    else:
        ps, keep = pack_local_sets(local_sets)
        rc = L.pdmpc_reachable_set_coupling_host(len(local_sets), len(local_sets[0]), C.byref(ps), n, *ptrs)
        del keep
        _check(L, rc, "pdmpc_reachable_set_coupling_host", last_error=None)
    return shaped()


def _group_offsets(group_sizes):
    off = np.zeros(len(group_sizes) + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.asarray(group_sizes, dtype=np.int64))
    return off


def _grouped_out(group_sizes):
    """The outputs of a grouped coupler, never empty -> (adjacency, areas, a call that decodes the blocks into [(adjacency (n_g, n_g),
    areas (n_g, n_g)) per group])."""
    total = int(sum(int(g) * int(g) for g in group_sizes))
    adj = np.zeros(max(total, 1), dtype=np.uint8)
    area = np.zeros(max(total, 1), dtype=np.float64)

    def blocks():
        out, at = [], 0
        for g in group_sizes:
            g = int(g)
            out.append((adj[at : at + g * g].reshape(g, g).copy(), area[at : at + g * g].reshape(g, g).copy()))
            at += g * g
        return out

    return adj, area, blocks


def reachable_set_coupling_grouped_call(local_sets, group_sizes, x, y, yaw, trim, handle=None):
    """The reachable-set coupler for several independent sets of vehicles at once: the vehicles are consecutive groups of
    `group_sizes` vehicles, pairs are formed inside a group only.  On `handle`'s device (pdmpc_reachable_set_coupling_grouped) or,
    without one, on the host twin.  -> [(adjacency (n_g, n_g) uint8, areas (n_g, n_g)) per group]."""
    L = load_library()
    x, y, c, s, t = _coupling_args(x, y, yaw, trim)
    off = _group_offsets(group_sizes)
    if int(off[-1]) != x.size:
        raise ValueError("the groups cover %d vehicles, %d were handed over" % (int(off[-1]), x.size))
    adj, area, blocks = _grouped_out(group_sizes)
    ptrs = [abi.i32p(off), abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), abi.i32p(t), abi.u8p(adj), abi.dp(area)]
    if handle is not None:
        _check(L, L.pdmpc_reachable_set_coupling_grouped(handle.h, len(group_sizes), *ptrs), "pdmpc_reachable_set_coupling_grouped")
    else:
        ps, keep = pack_local_sets(local_sets)
        rc = L.pdmpc_reachable_set_coupling_grouped_host(len(local_sets), len(local_sets[0]), C.byref(ps), len(group_sizes), *ptrs)
        del keep
        _check(L, rc, "pdmpc_reachable_set_coupling_grouped_host", last_error=None)
    return blocks()


def polygon_set_coupling_grouped_call(sets, group_sizes):
    """pdmpc_polygon_set_coupling_grouped_host: polygon_set_coupling_call on consecutive groups of the polygons
    -> [(adjacency, areas) per group]."""
    L = load_library()
    keep = abi._Keep()
    off = _group_offsets(group_sizes)
    if int(off[-1]) != len(sets):
        raise ValueError("the groups cover %d polygons, %d were handed over" % (int(off[-1]), len(sets)))
    ps = abi.pack_polygon_set([np.asarray(p, dtype=np.float64) for p in sets], keep)
    adj, area, blocks = _grouped_out(group_sizes)
    rc = L.pdmpc_polygon_set_coupling_grouped_host(C.byref(ps), len(group_sizes), abi.i32p(off), abi.u8p(adj), abi.dp(area))
    del keep
    _check(L, rc, "pdmpc_polygon_set_coupling_grouped_host", last_error=None)
    return blocks()


def fca_pairs(adjacency):
    """The coupled pairs a < b of an adjacency matrix in the order pdmpc_fca_collisions takes them: (P, 2) int32, ascending by (a, b)."""
    A = np.asarray(adjacency) != 0
    a, b = np.nonzero(np.triu(A, 1))
    return np.ascontiguousarray(np.stack([a, b], axis=1), dtype=np.int32).reshape(-1, 2)


def fca_pack(reference_points, pairs, length, width, offset, obstacles=(), dynamic_obstacle_area=(), headings=None):
    """The arguments of pdmpc_fca_collisions(_host) after the handle -> (args, (collisions, priorities) output arrays, keep-alive).
    The headings are prioritizer.calculate_yaw's and their cos / sin the host's libm, as prioritizer.fca_priorities builds them;
    `headings` = (cos, sin), two (n, Hp) arrays, is passed to the C ABI as it is instead (an exact quarter turn has no yaw angle)."""
    from .prioritizer import calculate_yaw

    ref = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in reference_points]
    n = len(ref)
    Hp = ref[0].shape[0] if n else 0
    if any(r.shape[0] != Hp for r in ref):
        raise ValueError("every vehicle needs Hp reference points")
    x = np.ascontiguousarray(np.concatenate([r[:, 0] for r in ref]) if n else np.zeros(1), dtype=np.float64)
    y = np.ascontiguousarray(np.concatenate([r[:, 1] for r in ref]) if n else np.zeros(1), dtype=np.float64)
    if headings is None:
        yaw = [a for r in ref for a in (calculate_yaw(r) if Hp >= 2 else np.zeros(Hp))]
        c = np.array([math.cos(float(a)) for a in yaw] or [0.0], dtype=np.float64)
        s = np.array([math.sin(float(a)) for a in yaw] or [0.0], dtype=np.float64)
    else:
        c, s = (np.ascontiguousarray(np.asarray(h, dtype=np.float64).reshape(-1)) for h in headings)
        if c.size != n * Hp or s.size != n * Hp:
            raise ValueError("headings: a cosine and a sine per vehicle and step")
        if not n * Hp:
            c, s = np.zeros(1), np.zeros(1)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    keep = abi._Keep()
    keep.refs += [x, y, c, s, pr]
    obst = abi.pack_polygon_set([np.asarray(o, dtype=np.float64) for o in obstacles], keep)
    dyn = abi.pack_polygon_set([np.asarray(p, dtype=np.float64) for row in dynamic_obstacle_area for p in row], keep) if len(dynamic_obstacle_area) else None
    keep.refs += [obst, dyn]
    coll = np.zeros(max(n, 1), dtype=np.int32)
    prio = np.zeros(max(n, 1), dtype=np.int32)
    args = [n, Hp, abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), len(pr), abi.i32p(pr) if len(pr) else None, C.byref(obst),
            C.byref(dyn) if dyn is not None else None, float(length), float(width), float(offset), abi.i32p(coll), abi.i32p(prio)]
    return args, (coll[:n], prio[:n]), keep


def fca_collisions_host(reference_points, pairs, length, width, offset, obstacles=(), dynamic_obstacle_area=(), handle=None, headings=None):
    """FcaPrioritizer natively (pdmpc_fca_collisions_host; on `handle`'s device, pdmpc_fca_collisions, if one is given).
    reference_points: per vehicle an (Hp, 2) array; pairs: (P, 2) coupled pairs a < b, ascending (fca_pairs); obstacles: (2, V) arrays;
    dynamic_obstacle_area: rows of Hp (2, V) arrays.  -> (collisions (n,) int32, priorities (n,) int32: the 1-based index vector of the
    stable descending sort, as the reference passes it on).  headings: (cos, sin) per vehicle and step in place of calculate_yaw's."""
    L = load_library()
    args, out, keep = fca_pack(reference_points, pairs, length, width, offset, obstacles, dynamic_obstacle_area, headings)
    if handle is not None:
        _check(L, L.pdmpc_fca_collisions(handle.h, *args), "pdmpc_fca_collisions")
    else:
        _check(L, L.pdmpc_fca_collisions_host(*args), "pdmpc_fca_collisions_host", last_error=None)
    del keep
    return out


def fca_grouped_pack(groups, Hp=None):
    """The arguments of pdmpc_fca_collisions_grouped(_host) after the handle -> (args, a call that decodes the outputs into
    [(collisions (n_g,), priorities (n_g,)) per group], keep-alive).  groups: per group a dict of fca_collisions_host's arguments
    (reference_points, pairs, length, width, offset and, optionally, obstacles, dynamic_obstacle_area, headings); a group without
    vehicles is legal.  Hp: the horizon, where no group has a vehicle to tell it.  An empty obstacle list is handed over as NULL."""
    keeps, arr, parts, sizes = [], (FcaGroup * max(len(groups), 1))(), [[], [], [], []], []
    for g, G in enumerate(groups):
        G = dict(G)
        refs = G.pop("reference_points")
        obst, dyn = G.pop("obstacles", ()), G.pop("dynamic_obstacle_area", ())
        args, _, keep = fca_pack(refs, G.pop("pairs"), G.pop("length"), G.pop("width"), G.pop("offset"), obst, dyn, G.pop("headings", None))
        if G:
            raise TypeError("unknown entries of group %d: %s" % (g, sorted(G)))
        n, hp = args[0], args[1]
        if n:
            if Hp is not None and hp != Hp:
                raise ValueError("group %d has Hp %d, the call %d" % (g, hp, Hp))
            Hp = hp
            for part, a in zip(parts, keep.refs[:4]):  # x, y, cos, sin of its reference points
                part.append(a)
        keeps.append(keep)
        sizes.append(n)
        arr[g].n, arr[g].n_pairs, arr[g].pairs = n, args[6], args[7] if args[6] else None
        arr[g].obstacles = C.pointer(keep.refs[-2]) if len(obst) else None
        arr[g].dynamic_rows = C.pointer(keep.refs[-1]) if keep.refs[-1] is not None else None
        arr[g].length, arr[g].width, arr[g].offset = args[10], args[11], args[12]
    x, y, c, s = (np.ascontiguousarray(np.concatenate(part + [np.zeros(1)])) for part in parts)
    N = int(sum(sizes))
    coll = np.zeros(max(N, 1), dtype=np.int32)
    prio = np.zeros(max(N, 1), dtype=np.int32)
    keeps += [arr, x, y, c, s]
    args = [len(groups), arr, Hp if Hp is not None else 0] + [abi.dp(a) for a in (x, y, c, s)] + [abi.i32p(coll), abi.i32p(prio)]
    at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)

    def per_group():
        return [(coll[at[g] : at[g + 1]].copy(), prio[at[g] : at[g + 1]].copy()) for g in range(len(groups))]

    return args, per_group, keeps


def fca_collisions_grouped_call(groups, Hp=None, handle=None):
    """FcaPrioritizer for several independent sets of vehicles at once (pdmpc_fca_collisions_grouped_host; on `handle`'s device,
    pdmpc_fca_collisions_grouped, if one is given); groups, Hp: see fca_grouped_pack.  -> [(collisions (n_g,), priorities (n_g,)) per
    group]: what fca_collisions_host returns for each group alone."""
    L = load_library()
    args, per_group, keep = fca_grouped_pack(groups, Hp)
    if handle is not None:
        _check(L, L.pdmpc_fca_collisions_grouped(handle.h, *args), "pdmpc_fca_collisions_grouped")
    else:
        _check(L, L.pdmpc_fca_collisions_grouped_host(*args), "pdmpc_fca_collisions_grouped_host", last_error=None)
    del keep
    return per_group()


def _pack_lanelet_polygons(lanelet_polys):
    """[vehicle] raw lanelet polygon (2, P) or None (not bounded) -> (pdmpc_polygon_set, keep-alive)."""
    keep = abi._Keep()
    polys = [np.zeros((2, 0)) if p is None else np.asarray(p, dtype=np.float64).reshape(2, -1) for p in lanelet_polys]
    return abi.pack_polygon_set(polys, keep), keep


def bound_reachable_sets_call(local_sets, x, y, yaw, trim, lanelet_polys, all_steps=True, handle=None):
    """bound_reachable_sets natively: on `handle`'s device (pdmpc_bound_reachable_sets; the handle must hold the table, see
    Handle.upload_reachable_sets) or, without one, on the host twin.  trim is 1-based; lanelet_polys[v] is vehicle v's raw lanelet
    polygon (reachability.lanelet_polygon) or None.  -> (sets: [vehicle][step] closed (2, c) arrays (one step, Hp, unless
    all_steps), flags (n, steps) uint8)."""
    L = load_library()
    x, y, c, s, t = _coupling_args(x, y, yaw, trim)
    n = x.size
    lp, lkeep = _pack_lanelet_polygons(lanelet_polys)
    S = (handle.options.Hp if handle is not None else len(local_sets[0])) if all_steps else 1
    off = np.zeros(n * S + 1, dtype=np.int32)
    flags = np.zeros(max(n * S, 1), dtype=np.uint8)
    head = [abi.dp(x), abi.dp(y), abi.dp(c), abi.dp(s), abi.i32p(t), C.byref(lp), int(bool(all_steps))]
    if handle is None:
        ps, keep = pack_local_sets(local_sets)
        fn = lambda *tail: L.pdmpc_bound_reachable_sets_host(len(local_sets), len(local_sets[0]), C.byref(ps), n, *head, *tail)  # noqa: E731
    else:
        fn = lambda *tail: L.pdmpc_bound_reachable_sets(handle.h, n, *head, *tail)  # noqa: E731
    rc = fn(0, abi.i32p(off), None, None, None)
    if rc != ERR_CAPACITY or (n and int(off[-1]) == 0):
        _check(L, rc, "pdmpc_bound_reachable_sets")
    tot = int(off[-1])
    bx = np.zeros(max(tot, 1))
    by = np.zeros(max(tot, 1))
    rc = fn(tot, abi.i32p(off), abi.dp(bx), abi.dp(by), abi.u8p(flags))
    del lkeep
    _check(L, rc, "pdmpc_bound_reachable_sets")
    sets = [[np.array([bx[off[v * S + q] : off[v * S + q + 1]], by[off[v * S + q] : off[v * S + q + 1]]]) for q in range(S)] for v in range(n)]
    return sets, flags[: n * S].reshape(n, S)


def polygon_set_coupling_call(sets):
    """pdmpc_polygon_set_coupling_host: ReachableSetCoupler.couple on any simple clockwise polygons -> (adjacency (n, n) uint8, areas)."""
    L = load_library()
    keep = abi._Keep()
    n = len(sets)
    ps = abi.pack_polygon_set([np.asarray(p, dtype=np.float64) for p in sets], keep)
    adj, area, shaped = _coupling_out(n)
    rc = L.pdmpc_polygon_set_coupling_host(C.byref(ps), n, abi.u8p(adj), abi.dp(area))
    del keep
    _check(L, rc, "pdmpc_polygon_set_coupling_host", last_error=None)
    return shaped()


class Choice:
    """A choice among the plans of a batch as data (pdmpc_choice), packed for the C ABI.

    cells: per cell the list of slots whose final costs are added, in this order; graphs: per graph its number of candidates (the
    cells are the graphs' candidates one graph after the other, cells beyond the last graph belong to none) or an explicit offset
    array; picks: per pick (graph, slots) -- a slot per candidate of the graph, or (-1, [slot])."""

    def __init__(self, cells, graphs=(), picks=(), graph_offset=None):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        self.cell_offset = i32(np.concatenate([[0], np.cumsum([len(c) for c in cells])]))
        self.cell_slot = i32([s for c in cells for s in c] + [0])
        self.graph_offset = i32(graph_offset if graph_offset is not None else np.concatenate([[0], np.cumsum(list(graphs))]))
        self.pick_graph = i32([g for g, _ in picks] + [0])
        self.pick_offset = i32(np.concatenate([[0], np.cumsum([len(sl) for _, sl in picks])]))
        self.pick_slot = i32([s for _, sl in picks for s in sl] + [0])
        self.n_cells, self.n_graphs, self.n_picks = len(cells), len(self.graph_offset) - 1, len(picks)

    def struct(self):
        p = abi.i32p
        return ChoiceStruct(self.n_cells, self.n_graphs, self.n_picks, 0, p(self.cell_offset), p(self.cell_slot), p(self.graph_offset), p(self.pick_graph),
                            p(self.pick_offset), p(self.pick_slot))

    def outputs(self):
        return np.zeros(max(self.n_graphs, 1), dtype=np.int32), np.zeros(max(self.n_cells, 1)), abi.out_array(max(self.n_picks, 1))

    def shaped(self, chosen, cost, picks=None):
        out = (chosen[: self.n_graphs], cost[: self.n_cells])
        return out if picks is None else out + (picks[: self.n_picks],)


def choose_host_call(status, final_cost, choice):
    """pdmpc_choose_host: the choice on the host twin (no GPU) -> (chosen per graph, rounded cost per cell)."""
    L = load_library()
    st = np.ascontiguousarray(status, dtype=np.int32)
    fc = np.ascontiguousarray(final_cost, dtype=np.float64)
    chosen, cost, _ = choice.outputs()
    ch = choice.struct()
    _check(L, L.pdmpc_choose_host(len(st), abi.i32p(st), abi.dp(fc), C.byref(ch), abi.i32p(chosen), abi.dp(cost)), "pdmpc_choose_host")
    return choice.shaped(chosen, cost)


def load_library(path=None):
    """dlopen the HIP backend and declare every prototype of include/pdmpc.h."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64; if this library pulled in the system
    # copy first, torch.cuda would later find "no HIP GPUs".  Importing torch first makes both share torch's copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise BackendError(
            "HIP backend %s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % p
        )
    L = declare(C.CDLL(p))
    if path is None:
        _LIB = L
    return L


def _check(L, rc, what, last_error="pdmpc_last_error"):
    """A failing status of `what` -> BackendError with .status, and with the message of the error string that belongs to the call:
    pdmpc_last_error, "pdmpc_controller_last_error", or None for a host twin, which leaves none."""
    if rc != 0:
        msg = ": " + (getattr(L, last_error)() or b"").decode() if last_error else ""
        err = BackendError("%s failed with status %d%s" % (what, rc, msg))
        err.status = rc
        raise err


def _flat_columns(lst):
    """A list of (2, n_i) arrays -> (offsets[len + 1], x, y) of their columns one behind the other (one spare element, so no array is empty)."""
    off = np.zeros(len(lst) + 1, dtype=np.int32)
    for i, p in enumerate(lst):
        off[i + 1] = off[i] + np.asarray(p).reshape(2, -1).shape[1]
    x = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(2, -1)[0] for p in lst] + [np.zeros(1)]))
    y = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(2, -1)[1] for p in lst] + [np.zeros(1)]))
    return off, x, y


def _step_args(Hp, iters, predecessors, fallback_shapes):
    """The arguments of a step call after the vehicle count -> (vehicle array, pred_offset, pred_index, fallback sets, keep-alive)."""
    n = len(iters)
    arr, keep = abi.pack_vehicles(iters, Hp)
    off = np.zeros(n + 1, dtype=np.int32)
    for i, p in enumerate(predecessors):
        off[i + 1] = off[i] + len(p)
    idx = np.array([j for p in predecessors for j in p] + [0], dtype=np.int32)
    fb = None
    if fallback_shapes is not None:
        fb = (abi.PolygonSet * n)()
        for i, shapes in enumerate(fallback_shapes):
            fb[i] = abi.pack_polygon_set(list(shapes), keep)
    return arr, off, idx, fb, keep


SHARD_AUTO, SHARD_COMPONENTS, SHARD_LEVELS = 0, 1, 2
COLLECTIVE_AUTO, COLLECTIVE_RCCL, COLLECTIVE_COPY = 0, 1, 2  # include/pdmpc.h: how the ranks of a group exchange their records


def group_partition(preds, world, mode=SHARD_AUTO, weights=None):
    """pdmpc_group_partition (no GPU needed): per vehicle the device of its whole component (-1: planned by levels over all
    devices), its level (1-based, 0 for whole components) and the device of its block within that level (-1)."""
    L = load_library()
    n = len(preds)
    off = np.zeros(n + 1, dtype=np.int32)
    for i, p in enumerate(preds):
        off[i + 1] = off[i] + len(p)
    idx = np.array([j for p in preds for j in p] + [0], dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    rank_of, level_of, block = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
    rc = L.pdmpc_group_partition(n, abi.i32p(off), abi.i32p(idx), None if w is None else abi.dp(w), world, mode, abi.i32p(rank_of), abi.i32p(level_of), abi.i32p(block))
    _check(L, rc, "pdmpc_group_partition")
    return rank_of[:n], level_of[:n], block[:n]


def group_route(preds, world, mode=SHARD_AUTO, weights=None):
    """pdmpc_group_route_host (no GPU needed): per vehicle the rank that holds its record after the launches of the step so
    partitioned, and its position among the records that rank holds."""
    L = load_library()
    n = len(preds)
    off = np.zeros(n + 1, dtype=np.int32)
    for i, p in enumerate(preds):
        off[i + 1] = off[i] + len(p)
    idx = np.array([j for p in preds for j in p] + [0], dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    rank, pos = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(2))
    rc = L.pdmpc_group_route_host(n, abi.i32p(off), abi.i32p(idx), None if w is None else abi.dp(w), world, mode, abi.i32p(rank), abi.i32p(pos))
    _check(L, rc, "pdmpc_group_route_host")
    return rank[:n], pos[:n]


class Group:
    """One pdmpc_group: a handle per GPU of this process, bound by an RCCL communicator; plan_step plans a time step over them
    (include/pdmpc.h: pdmpc_group_*)."""

    def __init__(self, options, n_devices=1, devices=None, checker=None, collective=COLLECTIVE_AUTO):
        """devices: HIP ordinals of the ranks (None: 0 .. n_devices - 1).  A device listed more than once makes LOGICAL ranks that share
        a GPU (collective = peer copies instead of RCCL): how the multi-rank protocol is exercised on a 1-GPU box."""
        self.L = load_library()
        self.options = options
        self.Hp = options.Hp
        if checker is None:
            checker = abi.CHECK_INTERX if options.are_any_obstacles_non_convex else abi.CHECK_SAT
        self.cfg = abi.Config(Hp=options.Hp, checker=checker, dt_seconds=options.dt_seconds, device=0, max_nodes=options.max_nodes, max_vehicles=options.max_vehicles,
                              trace_pops=0)
        self.g = C.c_void_p()
        devs = None if devices is None else (C.c_int32 * n_devices)(*devices)
        _check(self.L, self.L.pdmpc_group_create_ex(C.byref(self.cfg), n_devices, devs, collective, C.byref(self.g)), "pdmpc_group_create_ex")
        self.n_devices = n_devices
        c = C.c_int32(0)
        _check(self.L, self.L.pdmpc_group_collective(self.g, C.byref(c)), "pdmpc_group_collective")
        self.collective = {COLLECTIVE_RCCL: "rccl", COLLECTIVE_COPY: "copy"}[c.value]
        self._mpa_keep = None
        budget = int(getattr(options, "n_expansions_max", SAMPLED_BUDGET_DEFAULT))
        if budget != SAMPLED_BUDGET_DEFAULT:
            self.set_sampled_budget(budget)
        if int(getattr(options, "n_members", 1)) != 1:
            self.set_sampled_ensemble(options.n_members)

    def close(self):
        if self.g:
            self.L.pdmpc_group_destroy(self.g)
            self.g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_mpa(self, mpa):
        s, keep = abi.pack_mpa(mpa)
        _check(self.L, self.L.pdmpc_group_upload_mpa(self.g, C.byref(s)), "pdmpc_group_upload_mpa")
        self._mpa_keep = keep

    def plan_step(self, iters, predecessors, fallback_shapes=None, weights=None, mode=SHARD_AUTO):
        n = len(iters)
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        out = abi.out_array(n)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        rc = self.L.pdmpc_group_plan_step(self.g, n, arr, abi.i32p(off), abi.i32p(idx), fb, None if w is None else abi.dp(w), mode, abi.out_ptr(out))
        _check(self.L, rc, "pdmpc_group_plan_step")
        del keep
        return out[:n]

    def pack_step(self, bank, iters, predecessors, fallback_shapes=None, weights=None, mode=SHARD_AUTO):
        """Make a step resident on the devices (group bank `bank`); launch(bank) plans it, fetch(bank, n) reads the records."""
        n = len(iters)
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        rc = self.L.pdmpc_group_pack_step(self.g, bank, n, arr, abi.i32p(off), abi.i32p(idx), fb, None if w is None else abi.dp(w), mode)
        _check(self.L, rc, "pdmpc_group_pack_step")
        del keep

    def grow_arena(self, max_nodes):
        """Arenas of at least max_nodes nodes per vehicle on every device (the resident path does not grow them by itself)."""
        _check(self.L, self.L.pdmpc_group_grow_arena(self.g, int(max_nodes)), "pdmpc_group_grow_arena")

    def launch(self, bank):
        _check(self.L, self.L.pdmpc_group_launch(self.g, bank), "pdmpc_group_launch")

    def fetch(self, bank, n):
        out = abi.out_array(n)
        _check(self.L, self.L.pdmpc_group_fetch(self.g, bank, n, abi.out_ptr(out)), "pdmpc_group_fetch")
        return out[:n]

    def timing(self):
        t = (C.c_double * 6)()
        _check(self.L, self.L.pdmpc_group_last_timing(self.g, t), "pdmpc_group_last_timing")
        return dict(zip(("total", "partition", "pack", "enqueue", "wait", "read_back"), t))

    def rank0(self):
        """The handle of rank 0 (pdmpc_group_handle) as the object NativeController and NativeSweep take for `handle`: what a
        controller that is to step on the group (set_group) is created on.  The group owns it."""
        h = C.c_void_p()
        _check(self.L, self.L.pdmpc_group_handle(self.g, 0, C.byref(h)), "pdmpc_group_handle")
        return GroupHandle(self, h)

    def set_step_seeds(self, seeds):
        """pdmpc_group_set_step_seeds: the next pack makes sampled banks on the ranks (the sampled optimizer), seeds in the caller's order."""
        s = np.ascontiguousarray(seeds, dtype=np.uint32)
        _check(self.L, self.L.pdmpc_group_set_step_seeds(self.g, len(s), abi.u32p(s)), "pdmpc_group_set_step_seeds")

    def set_sampled_budget(self, n_expansions_max):
        """pdmpc_group_set_sampled_budget: the sampled optimizer's expansion budget on every rank."""
        _check(self.L, self.L.pdmpc_group_set_sampled_budget(self.g, int(n_expansions_max)), "pdmpc_group_set_sampled_budget")

    def set_sampled_ensemble(self, n_members):
        """pdmpc_group_set_sampled_ensemble: the sampled optimizer's ensemble size on every rank."""
        _check(self.L, self.L.pdmpc_group_set_sampled_ensemble(self.g, int(n_members)), "pdmpc_group_set_sampled_ensemble")

    def _group_step_args(self, iters, predecessors, fallback_shapes, weights, mode):
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        return (self.g, len(iters), arr, abi.i32p(off), abi.i32p(idx), fb, None if w is None else abi.dp(w), mode), (keep, off, idx, w)

    def plan_step_lean(self, iters, predecessors, fallback_shapes=None, weights=None, mode=SHARD_AUTO):
        """pdmpc_group_plan_step_lean -> (status, final cost) per vehicle; the records stay on the ranks for fetch_records_at."""
        n = len(iters)
        args, keep = self._group_step_args(iters, predecessors, fallback_shapes, weights, mode)
        status, cost = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1))
        _check(self.L, self.L.pdmpc_group_plan_step_lean(*args, abi.i32p(status), abi.dp(cost)), "pdmpc_group_plan_step_lean")
        del keep
        return status[:n], cost[:n]

    def fetch_records_at(self, vehicles):
        """pdmpc_group_fetch_records_at: the records of these vehicles of the step launched last, each from the rank that holds it."""
        v = np.ascontiguousarray(vehicles, dtype=np.int32)
        out = abi.out_array(max(len(v), 1))
        _check(self.L, self.L.pdmpc_group_fetch_records_at(self.g, len(v), abi.i32p(v), abi.out_ptr(out)), "pdmpc_group_fetch_records_at")
        return out[: len(v)]

    def _choice_call(self, what, call, choice):
        chosen, cost, picks = choice.outputs()
        ch = choice.struct()
        _check(self.L, call(C.byref(ch), abi.i32p(chosen), abi.dp(cost), abi.out_ptr(picks)), what)
        return choice.shaped(chosen, cost, picks)

    def plan_step_chosen(self, iters, predecessors, fallback_shapes, choice, weights=None, mode=SHARD_AUTO):
        """pdmpc_group_plan_step_chosen: the step over the ranks and the choice on them -> (chosen, cell costs, picked records)."""
        args, keep = self._group_step_args(iters, predecessors, fallback_shapes, weights, mode)
        out = self._choice_call("pdmpc_group_plan_step_chosen", lambda *tail: self.L.pdmpc_group_plan_step_chosen(*args, *tail), choice)
        del keep
        return out

    def choose_resident(self, bank, n, choice):
        """pdmpc_group_choose_resident: the choice on the records the ranks hold of group bank `bank` (the one launched last)."""
        return self._choice_call("pdmpc_group_choose_resident", lambda *tail: self.L.pdmpc_group_choose_resident(self.g, bank, n, *tail), choice)

    def debug_choose(self, records, rank_of, choice):
        """pdmpc_group_debug_choose: the choice over the ranks on records placed by hand (rank_of[v]; -1: on every rank)."""
        rec = np.ascontiguousarray(records)
        ro = np.ascontiguousarray(rank_of, dtype=np.int32)
        return self._choice_call("pdmpc_group_debug_choose", lambda *tail: self.L.pdmpc_group_debug_choose(self.g, len(rec), abi.out_ptr(rec), abi.i32p(ro), *tail), choice)

    def last_exchange(self):
        """pdmpc_group_last_exchange: the last call's bytes per rank into collectives, bytes to the host, host waits, re-plans."""
        x = (C.c_int64 * 4)()
        _check(self.L, self.L.pdmpc_group_last_exchange(self.g, x), "pdmpc_group_last_exchange")
        return dict(zip(("collective_bytes", "host_bytes", "host_waits", "replans"), (int(v) for v in x)))

    def reset_stats(self):
        for r in range(self.n_devices):
            h = C.c_void_p()
            _check(self.L, self.L.pdmpc_group_handle(self.g, r, C.byref(h)), "pdmpc_group_handle")
            _check(self.L, self.L.pdmpc_reset_stats(h), "pdmpc_reset_stats")

    def stats_all(self):
        """Statistics over the whole group: counts summed over the ranks, kernel_ms / n_launches of the rank whose kernels ran longest
        (the ranks' launches run side by side), per-rank values under "per_rank"."""
        per = [self.stats(r) for r in range(self.n_devices)]
        tot = dict(per[max(range(len(per)), key=lambda r: per[r]["kernel_ms"])])
        for k in ("edge_checks", "segment_pair_tests", "nodes_processed", "rounds", "shared_rounds", "helper_checked", "bad_status_plans", "queue_fallbacks",
                  "speculation_arrivals", "safe_replans"):
            if k in tot:
                tot[k] = sum(p[k] for p in per)
        tot["per_rank"] = per
        return tot

    def stats(self, rank=0):
        h = C.c_void_p()
        _check(self.L, self.L.pdmpc_group_handle(self.g, rank, C.byref(h)), "pdmpc_group_handle")
        st = abi.Stats()
        _check(self.L, self.L.pdmpc_get_last_stats(h, C.byref(st)), "pdmpc_get_last_stats")
        return {k: getattr(st, k) for k, _ in abi.Stats._fields_}


class GroupHandle:
    """A handle that belongs to a Group (Group.rank0): .h for the calls that take a pdmpc_handle; it keeps its group alive."""

    def __init__(self, group, h):
        self.group, self.h = group, h


class Handle:
    """One pdmpc_handle: bound to one GPU, owns the uploaded MPA and all device buffers."""

    def __init__(self, options, checker=None):
        self.L = load_library()
        self.options = options
        self.Hp = options.Hp
        if checker is None:
            checker = abi.CHECK_INTERX if options.are_any_obstacles_non_convex else abi.CHECK_SAT
        self.cfg = abi.Config(
            Hp=options.Hp,
            checker=checker,
            dt_seconds=options.dt_seconds,
            device=options.device,
            max_nodes=options.max_nodes,
            max_vehicles=options.max_vehicles,
            trace_pops=options.trace_pops,
        )
        self.allow_overflow = False  # tests of the overflow status itself switch this on
        self.h = C.c_void_p()
        _check(self.L, self.L.pdmpc_create(C.byref(self.cfg), C.byref(self.h)), "pdmpc_create")
        self._mpa_keep = None
        budget = int(getattr(options, "n_expansions_max", SAMPLED_BUDGET_DEFAULT))
        if budget != SAMPLED_BUDGET_DEFAULT:
            self.set_sampled_budget(budget)
        if int(getattr(options, "n_members", 1)) != 1:
            self.set_sampled_ensemble(options.n_members)

    def set_sampled_ensemble(self, n_members):
        """pdmpc_set_sampled_ensemble: members per vehicle of the sampled banks packed from now on (1: the reference's one stream)."""
        _check(self.L, self.L.pdmpc_set_sampled_ensemble(self.h, int(n_members)), "pdmpc_set_sampled_ensemble")

    def get_sampled_ensemble(self):
        """pdmpc_get_sampled_ensemble."""
        n = C.c_int32(0)
        _check(self.L, self.L.pdmpc_get_sampled_ensemble(self.h, C.byref(n)), "pdmpc_get_sampled_ensemble")
        return int(n.value)

    def sampled_ensemble_result(self, n_vehicles, n_members=None):
        """pdmpc_sampled_ensemble_result of the current bank's last launch, in the caller's vehicle order ->
        (winner (n,), member_status (n, E), member_cost (n, E); +inf where a member is not OK).  n_members: the size the bank was
        packed with, if the handle's has been changed since."""
        E = self.get_sampled_ensemble() if n_members is None else int(n_members)
        winner = np.zeros(max(n_vehicles, 1), dtype=np.int32)
        status = np.zeros(max(n_vehicles * E, 1), dtype=np.int32)
        cost = np.zeros(max(n_vehicles * E, 1))
        _check(self.L, self.L.pdmpc_sampled_ensemble_result(self.h, int(n_vehicles), abi.i32p(winner), abi.i32p(status), abi.dp(cost)), "pdmpc_sampled_ensemble_result")
        return winner[:n_vehicles], status[: n_vehicles * E].reshape(n_vehicles, E), cost[: n_vehicles * E].reshape(n_vehicles, E)

    def set_sampled_budget(self, n_expansions_max):
        """pdmpc_set_sampled_budget: the sampled optimizer's expansion budget (MonteCarloTreeSearch.m:8) of the banks packed from now on."""
        _check(self.L, self.L.pdmpc_set_sampled_budget(self.h, int(n_expansions_max)), "pdmpc_set_sampled_budget")

    def sampled_budget(self):
        """pdmpc_get_sampled_budget."""
        n = C.c_int32(0)
        _check(self.L, self.L.pdmpc_get_sampled_budget(self.h, C.byref(n)), "pdmpc_get_sampled_budget")
        return int(n.value)

    def last_sampled_kernel(self):
        """pdmpc_last_sampled_kernel: the kernel the last sampled launch ran ("" before the first one)."""
        return self.L.pdmpc_last_sampled_kernel(self.h).decode()

    def sampled_plan_bank(self, n_expansions_max):
        """pdmpc_sampled_plan_bank: the plan of the current (sampled) bank at a budget -> ({field: value} incl. kernel, extra dict)."""
        p = abi.LaunchPlan()
        x = (C.c_int64 * 4)()
        _check(self.L, self.L.pdmpc_sampled_plan_bank(self.h, int(n_expansions_max), C.byref(p), x), "pdmpc_sampled_plan_bank")
        plan = {f: getattr(p, f) for f, _ in abi.LaunchPlan._fields_}
        plan["kernel"] = plan["kernel"].decode() if plan["kernel"] else ""
        return plan, dict(zip(("node_cap", "tree_in_lds", "tree_hbm_bytes", "rand_chunk"), (int(v) for v in x)))

    def debug_random_stream(self, seeds, n):
        """The chunked generator of pdmpc_sampled_budget_kernel on its own (pdmpc_debug_random_stream) -> (len(seeds), n) doubles."""
        sd = (C.c_uint32 * max(len(seeds), 1))(*[int(s) for s in seeds])
        out = np.zeros(max(len(seeds) * n, 1))
        _check(self.L, self.L.pdmpc_debug_random_stream(self.h, len(seeds), sd, int(n), abi.dp(out)), "pdmpc_debug_random_stream")
        return out[: len(seeds) * n].reshape(len(seeds), n)

    def close(self):
        if self.h:
            self.L.pdmpc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_mpa(self, mpa):
        s, keep = abi.pack_mpa(mpa)
        _check(self.L, self.L.pdmpc_upload_mpa(self.h, C.byref(s)), "pdmpc_upload_mpa")
        self._mpa_keep = keep

    def plan_batch(self, iters):
        """list[VehicleIter] -> numpy records (abi.VEHICLE_OUT_DTYPE)."""
        n = len(iters)
        arr, keep = abi.pack_vehicles(iters, self.Hp)
        out = abi.out_array(n)
        _check(self.L, self.L.pdmpc_plan_batch(self.h, n, arr, abi.out_ptr(out)), "pdmpc_plan_batch")
        del keep
        return self._checked(out[:n])

    def plan_batch_sampled(self, iters, seeds):
        """The sampled optimizer for one computation level; seeds[i] = time_step + vehicle_index (MonteCarloTreeSearch.m:32)."""
        n = len(iters)
        arr, keep = abi.pack_vehicles(iters, self.Hp)
        out = abi.out_array(n)
        sd = (C.c_uint32 * max(n, 1))(*[int(s) for s in seeds])
        _check(self.L, self.L.pdmpc_plan_batch_sampled(self.h, n, arr, sd, abi.out_ptr(out)), "pdmpc_plan_batch_sampled")
        del keep
        return out[:n]

    def plan_step_sampled(self, iters, predecessors, fallback_shapes, seeds):
        """A whole time step of the sampled optimizer in one call (pdmpc_plan_step_sampled): arguments as for plan_step, seeds[i] =
        time_step + vehicle_index of vehicle i (MonteCarloTreeSearch.m:32)."""
        n = len(iters)
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        out = abi.out_array(n)
        sd = (C.c_uint32 * max(n, 1))(*[int(s) for s in seeds])
        _check(self.L, self.L.pdmpc_plan_step_sampled(self.h, n, arr, abi.i32p(off), abi.i32p(idx), fb, sd, abi.out_ptr(out)), "pdmpc_plan_step_sampled")
        del keep
        return self._checked(out[:n])

    def set_step_seeds(self, seeds):
        """Seeds of the next packed step (pdmpc_set_step_seeds): that pack makes a sampled bank, whose launches run the sampled optimizer."""
        sd = (C.c_uint32 * max(len(seeds), 1))(*[int(s) for s in seeds])
        _check(self.L, self.L.pdmpc_set_step_seeds(self.h, len(seeds), sd), "pdmpc_set_step_seeds")

    def debug_random_numbers(self, seeds, n):
        """The sampled kernel's device generator on its own (pdmpc_debug_random_numbers) -> (len(seeds), n) doubles."""
        sd = (C.c_uint32 * max(len(seeds), 1))(*[int(s) for s in seeds])
        out = np.zeros(max(len(seeds) * n, 1))
        _check(self.L, self.L.pdmpc_debug_random_numbers(self.h, len(seeds), sd, int(n), abi.dp(out)), "pdmpc_debug_random_numbers")
        return out[: len(seeds) * n].reshape(len(seeds), n)

    def plan_joint(self, problems):
        """Centralized control: list of problems, each a list of 1 to JOINT_MAX VehicleIter, one joint search per problem ->
        numpy records (abi.VEHICLE_OUT_DTYPE), one per vehicle in input order (pdmpc_plan_joint)."""
        off = np.zeros(len(problems) + 1, dtype=np.int32)
        for p, prob in enumerate(problems):
            off[p + 1] = off[p] + len(prob)
        iters = [it for prob in problems for it in prob]
        n = len(iters)
        arr, keep = abi.pack_vehicles(iters, self.Hp)
        out = abi.out_array(n)
        _check(self.L, self.L.pdmpc_plan_joint(self.h, len(problems), abi.i32p(off), arr, abi.out_ptr(out)), "pdmpc_plan_joint")
        del keep
        return self._checked(out[:n])

    def packed_offsets(self, vehicle):
        """Where the last pack put `vehicle` in the point pool (pdmpc_debug_packed_offsets) -> (lit_off, hdv_off, (ll_off, ll_len))."""
        lit, hdv = (np.zeros(abi.HP_MAX + 1, dtype=np.int32) for _ in range(2))
        ll = np.zeros(2, dtype=np.int32)
        _check(self.L, self.L.pdmpc_debug_packed_offsets(self.h, int(vehicle), abi.i32p(lit), abi.i32p(hdv), abi.i32p(ll)), "pdmpc_debug_packed_offsets")
        return lit[: self.Hp + 1].tolist(), hdv[: self.Hp + 1].tolist(), (int(ll[0]), int(ll[1]))

    def upload_reachable_sets(self, local_sets):
        """pdmpc_upload_reachable_sets: the automaton's local hulls ([trim][k] (2, m), e.g. mpa.local_reachable_sets_conv)."""
        ps, keep = pack_local_sets(local_sets)
        _check(self.L, self.L.pdmpc_upload_reachable_sets(self.h, len(local_sets), len(local_sets[0]), C.byref(ps)), "pdmpc_upload_reachable_sets")
        del keep

    def reachable_set_coupling(self, x, y, yaw, trim):
        """ReachableSetCoupler.couple on this handle's device (pdmpc_reachable_set_coupling) -> (adjacency (n, n) uint8, areas (n, n))."""
        return reachable_set_coupling_call(None, x, y, yaw, trim, handle=self)

    def bound_reachable_sets(self, x, y, yaw, trim, lanelet_polys, all_steps=True):
        """pdmpc_bound_reachable_sets on this handle's device -> (sets [vehicle][step], flags (n, steps)); the sets stay on the device
        for bounded_set_coupling."""
        out = bound_reachable_sets_call(None, x, y, yaw, trim, lanelet_polys, all_steps, handle=self)
        self._bound_n = len(out[0])
        return out

    def bounded_set_coupling(self):
        """pdmpc_bounded_set_coupling on the step-Hp sets of the last bound_reachable_sets -> (adjacency (n, n) uint8, areas (n, n))."""
        n = getattr(self, "_bound_n", 0)
        adj = np.zeros(max(n * n, 1), dtype=np.uint8)
        area = np.zeros(max(n * n, 1), dtype=np.float64)
        _check(self.L, self.L.pdmpc_bounded_set_coupling(self.h, abi.u8p(adj), abi.dp(area)), "pdmpc_bounded_set_coupling")
        return adj[: n * n].reshape(n, n), area[: n * n].reshape(n, n)

    def reachable_set_coupling_grouped(self, group_sizes, x, y, yaw, trim):
        """pdmpc_reachable_set_coupling_grouped on this handle's device: consecutive groups of `group_sizes` vehicles, pairs inside a
        group only -> [(adjacency (n_g, n_g) uint8, areas (n_g, n_g)) per group]."""
        return reachable_set_coupling_grouped_call(None, group_sizes, x, y, yaw, trim, handle=self)

    def bounded_set_coupling_grouped(self, group_sizes):
        """pdmpc_bounded_set_coupling_grouped on the step-Hp sets of the last bound_reachable_sets, as consecutive groups of
        `group_sizes` vehicles -> [(adjacency, areas) per group]."""
        off = _group_offsets(group_sizes)
        adj, area, blocks = _grouped_out(group_sizes)
        rc = self.L.pdmpc_bounded_set_coupling_grouped(self.h, len(group_sizes), abi.i32p(off), abi.u8p(adj), abi.dp(area))
        _check(self.L, rc, "pdmpc_bounded_set_coupling_grouped")
        return blocks()

    def bounded_reachable_kernel_ms(self):
        """kernel times (ms) of the last bound_reachable_sets and bounded_set_coupling"""
        ms = np.zeros(2)
        _check(self.L, self.L.pdmpc_bounded_reachable_kernel_ms(self.h, abi.dp(ms)), "pdmpc_bounded_reachable_kernel_ms")
        return float(ms[0]), float(ms[1])

    def fca_collisions(self, reference_points, pairs, length, width, offset, obstacles=(), dynamic_obstacle_area=(), headings=None):
        """FcaPrioritizer on this handle's device (pdmpc_fca_collisions) -> (collisions, priorities); see fca_collisions_host."""
        return fca_collisions_host(reference_points, pairs, length, width, offset, obstacles, dynamic_obstacle_area, handle=self, headings=headings)

    def fca_collisions_grouped(self, groups, Hp=None):
        """pdmpc_fca_collisions_grouped on this handle's device -> [(collisions, priorities) per group]; see fca_collisions_grouped_call."""
        return fca_collisions_grouped_call(groups, Hp, handle=self)

    def fca_kernel_ms(self):
        """kernel time (ms) of the last fca_collisions or fca_collisions_grouped"""
        ms = C.c_double(0.0)
        _check(self.L, self.L.pdmpc_fca_kernel_ms(self.h, C.byref(ms)), "pdmpc_fca_kernel_ms")
        return ms.value

    def upload_hdv_map(self, hmap, local_sets, slot=0):
        """pdmpc_upload_hdv_map_slot: the map (hdv.HdvMap) and the HDV automaton's local sets into one of the handle's map slots; slot 0
        is what hdv_traffic reads, a group of hdv_traffic_grouped names its slot."""
        from . import hdv

        hdv.upload_hdv_map(self, hmap, local_sets, slot=slot)

    def hdv_map_slot_state(self, slot=0):
        """(the slot's generation: 0 before its first upload, a larger number after every upload; uploads into all slots so far)"""
        from . import hdv

        return hdv.hdv_map_slot_state(self, slot)

    def hdv_map_slot_holds(self, slot, hmap, local_sets):
        """pdmpc_hdv_map_slot_holds: the slot holds exactly this map and these local sets (compared byte for byte, no hash)"""
        from . import hdv

        return hdv.hdv_map_slot_holds(self, slot, hmap, local_sets)

    def hdv_traffic_grouped(self, groups, capacity=None, call_ms=None, raw=None, guard=0):
        """pdmpc_hdv_traffic_grouped on this handle's device -> per group the dict of hdv_traffic; see hdv.hdv_traffic_grouped_native."""
        from . import hdv

        return hdv.hdv_traffic_grouped_native(self, groups, capacity=capacity, call_ms=call_ms, raw=raw, guard=guard)

    def hdv_traffic(self, hdv_x, hdv_y, hdv_yaw, hdv_trim, hdv_tile, cav_x, cav_y, cav_lanelet, cav_tile, capacity=None, call_ms=None, cos_sin=None):
        """pdmpc_hdv_traffic on this handle's device; see hdv.hdv_traffic_native."""
        from . import hdv

        return hdv.hdv_traffic_native(None, None, hdv_x, hdv_y, hdv_yaw, hdv_trim, hdv_tile, cav_x, cav_y, cav_lanelet, cav_tile, handle=self, capacity=capacity,
                                      call_ms=call_ms, cos_sin=cos_sin)

    def hdv_kernel_ms(self):
        """kernel time (ms) of the last hdv_traffic"""
        from . import hdv

        return hdv.hdv_kernel_ms(self)

    def reachable_set_coupling_kernel_ms(self):
        ms = C.c_double(0.0)
        _check(self.L, self.L.pdmpc_reachable_set_coupling_kernel_ms(self.h, C.byref(ms)), "pdmpc_reachable_set_coupling_kernel_ms")
        return ms.value

    def unique_priorities(self, adjacency, max_out):
        """Prioritizer.unique_priorities on this handle's device (pdmpc_unique_priorities) -> (priorities n x K, masks [K])."""
        return unique_priorities_call(adjacency, max_out, handle=self)

    def unique_priorities_grouped(self, graphs, max_out, **out):
        """... of several graphs in ONE call (pdmpc_unique_priorities_grouped) -> [(priorities n_g x K_g, masks [K_g])]."""
        return unique_priorities_grouped_call(graphs, max_out, handle=self, **out)

    # ---- device-resident path ----
    def pack_batch(self, iters):
        arr, keep = abi.pack_vehicles(iters, self.Hp)
        _check(self.L, self.L.pdmpc_pack_batch(self.h, len(iters), arr), "pdmpc_pack_batch")
        del keep

    def set_step_weights(self, weights):
        """Expected work per vehicle of the next packed step (pdmpc_set_step_weights): its searches go out by priority, not slot order."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        _check(self.L, self.L.pdmpc_set_step_weights(self.h, len(w), abi.dp(w)), "pdmpc_set_step_weights")

    def pack_step(self, iters, predecessors, fallback_shapes=None, weights=None):
        """predecessors: list (per vehicle) of lists of 0-based vehicle indices in this batch."""
        n = len(iters)
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        if weights is not None:
            self.set_step_weights(weights)
        _check(self.L, self.L.pdmpc_pack_step(self.h, n, arr, abi.i32p(off), abi.i32p(idx), fb), "pdmpc_pack_step")
        del keep

    def plan_step(self, iters, predecessors, fallback_shapes=None, weights=None):
        """A whole time step in one call (pdmpc_plan_step): pack + launch + fetch, arenas grow if a search needs it."""
        n = len(iters)
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        out = abi.out_array(n)
        if weights is not None:
            self.set_step_weights(weights)
        _check(self.L, self.L.pdmpc_plan_step(self.h, n, arr, abi.i32p(off), abi.i32p(idx), fb, abi.out_ptr(out)), "pdmpc_plan_step")
        del keep
        return self._checked(out[:n])

    def _choice_call(self, what, call, choice):
        chosen, cost, picks = choice.outputs()
        ch = choice.struct()
        _check(self.L, call(C.byref(ch), abi.i32p(chosen), abi.dp(cost), abi.out_ptr(picks)), what)
        return choice.shaped(chosen, cost, picks)

    def choose_resident(self, n, choice):
        """pdmpc_choose_resident: the choice on the device on the n records resident in the current bank -> (chosen, cell costs, picked records)."""
        return self._choice_call("pdmpc_choose_resident", lambda *tail: self.L.pdmpc_choose_resident(self.h, n, *tail), choice)

    def plan_step_chosen(self, iters, predecessors, fallback_shapes, choice, weights=None):
        """pdmpc_plan_step_chosen: pack, ONE launch of the searches, the choice on the device, one read-back -> (chosen, cell costs, picked records)."""
        n = len(iters)
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        if weights is not None:
            self.set_step_weights(weights)
        out = self._choice_call("pdmpc_plan_step_chosen", lambda *tail: self.L.pdmpc_plan_step_chosen(self.h, n, arr, abi.i32p(off), abi.i32p(idx), fb, *tail), choice)
        del keep
        return out

    def choice_kernel_ms(self):
        """Kernel milliseconds (HIP events) of the two launches of the last choice on the device."""
        ms = C.c_double()
        _check(self.L, self.L.pdmpc_choice_kernel_ms(self.h, C.byref(ms)), "pdmpc_choice_kernel_ms")
        return ms.value

    def step_args(self, iters, predecessors, fallback_shapes=None):
        """The marshalled arguments of pdmpc_plan_step / pdmpc_plan_step_literal, reusable across calls (bench.py times the calls,
        not the Python marshalling): (n, vehicle array, pred_offset, pred_index, fallback sets, keep-alive)."""
        arr, off, idx, fb, keep = _step_args(self.Hp, iters, predecessors, fallback_shapes)
        return len(iters), arr, off, idx, fb, keep

    def plan_step_literal(self, args):
        """One pdmpc_plan_batch(h, 1, ...) per vehicle in slot (= kahn) order with the hand-over on the host: what GraphSearchHip.m
        gives an unmodified controller (pdmpc_plan_step_literal).  args = step_args(...)."""
        n, arr, off, idx, fb, _ = args
        out = abi.out_array(n)
        _check(self.L, self.L.pdmpc_plan_step_literal(self.h, n, arr, abi.i32p(off), abi.i32p(idx), fb, abi.out_ptr(out)), "pdmpc_plan_step_literal")
        return self._checked(out[:n])

    def _checked(self, recs):
        """Only PDMPC_EXHAUSTED is a planning result (info.is_exhausted); anything else is an error of this backend."""
        st = np.asarray(recs["status"])
        if ((st != abi.OK) & (st != abi.EXHAUSTED)).any() and not self.allow_overflow:
            bad = int(st[(st != abi.OK) & (st != abi.EXHAUSTED)][0])
            if bad == abi.ARENA_OVERFLOW:
                raise BackendError("a search outgrew its arena (%d nodes per vehicle) and the arena limit forbids growing it" % self.arena_nodes()[0])
            raise BackendError("device-side error status %d in a result record (predecessor wait timed out?)" % bad)
        return recs

    def set_arena_limit(self, max_nodes_limit):
        _check(self.L, self.L.pdmpc_set_arena_limit(self.h, int(max_nodes_limit)), "pdmpc_set_arena_limit")

    def grow_arena(self, max_nodes):
        _check(self.L, self.L.pdmpc_grow_arena(self.h, int(max_nodes)), "pdmpc_grow_arena")

    def arena_nodes(self):
        n, r = C.c_int32(), C.c_int64()
        _check(self.L, self.L.pdmpc_arena_nodes(self.h, C.byref(n), C.byref(r)), "pdmpc_arena_nodes")
        return n.value, r.value

    def launch(self):
        _check(self.L, self.L.pdmpc_launch_packed(self.h), "pdmpc_launch_packed")

    def launch_range(self, first, count):
        _check(self.L, self.L.pdmpc_launch_range(self.h, first, count), "pdmpc_launch_range")

    def begin_step(self):
        _check(self.L, self.L.pdmpc_begin_step(self.h), "pdmpc_begin_step")

    def select_bank(self, bank):
        _check(self.L, self.L.pdmpc_select_bank(self.h, bank), "pdmpc_select_bank")

    def reset_stats(self):
        _check(self.L, self.L.pdmpc_reset_stats(self.h), "pdmpc_reset_stats")

    def synchronize(self):
        _check(self.L, self.L.pdmpc_synchronize(self.h), "pdmpc_synchronize")

    def set_safe_launch(self, on):
        """Every launch in slices that are resident as a whole (forward progress without any assumption on the dispatch order)."""
        _check(self.L, self.L.pdmpc_set_safe_launch(self.h, 1 if on else 0), "pdmpc_set_safe_launch")

    def fetch(self, n):
        out = abi.out_array(n)
        _check(self.L, self.L.pdmpc_fetch_results(self.h, n, abi.out_ptr(out)), "pdmpc_fetch_results")
        return self._checked(out[:n])

    def result_device_buffer(self):
        p = C.c_void_p()
        nb = C.c_size_t()
        _check(self.L, self.L.pdmpc_result_device_buffer(self.h, C.byref(p), C.byref(nb)), "pdmpc_result_device_buffer")
        return p.value, nb.value

    def import_results(self, first, n, dev_ptr):
        _check(self.L, self.L.pdmpc_import_results(self.h, first, n, C.c_void_p(dev_ptr)), "pdmpc_import_results")

    def export_results(self, first, n, dev_ptr):
        _check(self.L, self.L.pdmpc_export_results(self.h, first, n, C.c_void_p(dev_ptr)), "pdmpc_export_results")

    def export_results_async(self, first, n, dev_ptr):
        _check(self.L, self.L.pdmpc_export_results_async(self.h, first, n, C.c_void_p(dev_ptr)), "pdmpc_export_results_async")

    def stream_ptr(self):
        p = C.c_void_p()
        _check(self.L, self.L.pdmpc_stream(self.h, C.byref(p)), "pdmpc_stream")
        return p.value or 0

    def stats(self):
        s = abi.Stats()
        _check(self.L, self.L.pdmpc_get_last_stats(self.h, C.byref(s)), "pdmpc_get_last_stats")
        return {name: getattr(s, name) for name, _ in abi.Stats._fields_}

    def heap_script(self, ops, ids, keys, lds_entries=4096):
        """Run a push/pop script on the device open list -> (popped ids, cycles per pop, cycles per push)."""
        ops = np.ascontiguousarray(ops, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        keys = np.ascontiguousarray(keys, dtype=np.float64)
        out = np.zeros(max(len(ops), 1), dtype=np.int32)
        n = C.c_int32()
        cp, cq = C.c_double(), C.c_double()
        rc = self.L.pdmpc_debug_heap_script(self.h, len(ops), abi.i32p(ops), abi.i32p(ids), abi.dp(keys), lds_entries, abi.i32p(out), C.byref(n), C.byref(cp), C.byref(cq))
        _check(self.L, rc, "pdmpc_debug_heap_script")
        return out[: n.value].copy(), cp.value, cq.value

    def pop_trace(self, vehicle, capacity=1 << 16):
        ids = np.zeros(capacity, dtype=np.int32)
        n = C.c_int32()
        _check(self.L, self.L.pdmpc_debug_pop_trace(self.h, vehicle, capacity, abi.i32p(ids), C.byref(n)), "pdmpc_debug_pop_trace")
        return ids[: min(n.value, capacity)].copy()

    def raw_tree(self, vehicle, capacity=1 << 20):
        """The arena as the kernel left it: node arrays + key + validity (see pdmpc_debug_raw_tree)."""
        f = {k: np.zeros(capacity) for k in ("x", "y", "yaw", "g", "h", "key")}
        i = {k: np.zeros(capacity, dtype=np.int32) for k in ("trim", "k", "parent")}
        val = np.zeros(capacity, dtype=np.uint8)
        n = C.c_int32()
        args = [abi.dp(f[k]) for k in ("x", "y", "yaw", "g", "h")] + [abi.i32p(i[k]) for k in ("trim", "k", "parent")]
        args += [abi.dp(f["key"]), abi.u8p(val)]
        _check(self.L, self.L.pdmpc_debug_raw_tree(self.h, vehicle, capacity, *args, C.byref(n)), "pdmpc_debug_raw_tree")
        nn = min(n.value, capacity)
        d = {k: v[:nn].copy() for k, v in f.items()}
        d.update({k: v[:nn].copy() for k, v in i.items()})
        d["validity"] = val[:nn].copy()
        return d

    def edge_check(self, mode, a_list, b_list):
        """Run a collision primitive on the device for len(a_list) cases: mode 0 InterX, 1 intersect_sat, 2 intersect_lanelet_boundary
        (b = [left, NaN, right, NaN]), 3 intersect_sat against every polygon of a NaN-separated soup.  a_list / b_list: lists of (2, n)
        arrays.  Returns a bool array."""
        return self.edge_check_raw(mode, a_list, b_list) != 0

    def edge_check_raw(self, mode, a_list, b_list):
        """edge_check with the call's own codes: 0 / 1, or
        2 + the per-lane answer where the wave-wide and the per-lane form of a check disagree.  Returns an int32 array."""
        n = len(a_list)
        ao, ax, ay = _flat_columns(a_list)
        bo, bx, by = _flat_columns(b_list)
        hit = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.L.pdmpc_debug_edge_check(self.h, mode, n, abi.i32p(ao), abi.dp(ax), abi.dp(ay), abi.i32p(bo), abi.dp(bx), abi.dp(by), abi.i32p(hit))
        _check(self.L, rc, "pdmpc_debug_edge_check")
        return hit[:n].copy()

    def interx_soups(self, a_list, b_list, soups):
        """The InterX check of an edge on its three soups (pdmpc_debug_interx_soups): a_list / b_list = shapes A and B of every case
        (equal column counts), soups = one (vehicle soup, HDV soup, boundary) triple of (2, n) arrays per case.  Codes as edge_check_raw."""
        n = len(a_list)
        assert len(b_list) == n and len(soups) == n and all(len(t) == 3 for t in soups)
        assert all(np.asarray(a).shape == np.asarray(b).shape for a, b in zip(a_list, b_list))
        ao, ax, ay = _flat_columns(a_list)
        _, bx, by = _flat_columns(b_list)
        so, sx, sy = _flat_columns([s for t in soups for s in t])
        hit = np.zeros(max(n, 1), dtype=np.int32)
        rc = self.L.pdmpc_debug_interx_soups(self.h, n, abi.i32p(ao), abi.dp(ax), abi.dp(ay), abi.dp(bx), abi.dp(by), abi.i32p(so), abi.dp(sx), abi.dp(sy), abi.i32p(hit))
        _check(self.L, rc, "pdmpc_debug_interx_soups")
        return hit[:n].copy()

    def debug_sincos(self, x):
        """include/pdmpc_math.h's pdmpc_sincos on the device (pdmpc_debug_sincos) -> (sin, cos) of every element of x."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        s, c = np.zeros_like(x), np.zeros_like(x)
        _check(self.L, self.L.pdmpc_debug_sincos(self.h, x.size, abi.dp(x), abi.dp(s), abi.dp(c)), "pdmpc_debug_sincos")
        return s, c

    def debug_counters(self):
        out = (C.c_uint64 * 16)()
        _check(self.L, self.L.pdmpc_debug_counters(self.h, out), "pdmpc_debug_counters")
        return list(out)

    def progress(self, vehicle):
        w = (C.c_uint32 * 32)()
        _check(self.L, self.L.pdmpc_debug_progress(self.h, vehicle, w), "pdmpc_debug_progress")
        return list(w)

    def tree(self, vehicle, capacity=1 << 16):
        f = {k: np.zeros(capacity) for k in ("x", "y", "yaw", "g", "h")}
        i = {k: np.zeros(capacity, dtype=np.int32) for k in ("trim", "k", "parent")}
        n = C.c_int32()
        args = [abi.dp(f[k]) for k in ("x", "y", "yaw", "g", "h")] + [abi.i32p(i[k]) for k in ("trim", "k", "parent")]
        _check(self.L, self.L.pdmpc_debug_tree(self.h, vehicle, capacity, *args, C.byref(n)), "pdmpc_debug_tree")
        nn = min(n.value, capacity)
        d = {k: v[:nn].copy() for k, v in f.items()}
        d.update({k: v[:nn].copy() for k, v in i.items()})
        return d
