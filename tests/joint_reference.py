"""CPU restatement of the joint graph search of centralized control.  TEST INFRASTRUCTURE ONLY.

GraphSearch.do_graph_search (hlc/optimizer/graph_search/GraphSearch.m:23-107) with iter.amount = N and the separating-axis
checker: eval_edge_exact (:111-196) with are_constraints_satisfied_sat.m, expand_node.m with cartprod.m / ind2subVect.m, and the
reference's priority queue (priority_queue_interface_mex.cpp:19-31, a std::priority_queue) restated from libstdc++'s
push_heap / pop_heap below.  The collision tests and sin / cos are the oracle's exported primitives, so with N = 1 this is the
oracle's single-vehicle search (tests/test_joint_reference.py pins that).  Python floats are IEEE doubles evaluated operation by
operation, the arithmetic of the oracle and of the kernels (-ffp-contract=off).

Records come out in abi.VEHICLE_OUT_DTYPE, one per vehicle, in the layout pdmpc_plan_joint documents (include/pdmpc.h).
"""
import math

import numpy as np

from pdmpc import abi

from oracle import oracle

OK, EXHAUSTED, ARENA_OVERFLOW = abi.OK, abi.EXHAUSTED, abi.ARENA_OVERFLOW


# ---- std::priority_queue<tuple<size_t, double>, vector, comp> with comp(a, b) = a.key > b.key (libstdc++ stl_heap.h)
def _comp(a, b):
    return a[1] > b[1]


def _push_heap_hole(h, hole, top, value):  # std::__push_heap
    parent = (hole - 1) // 2
    while hole > top and _comp(h[parent], value):
        h[hole] = h[parent]
        hole = parent
        parent = (hole - 1) // 2
    h[hole] = value


def heap_push(h, entry):  # priority_queue::push = push_back + push_heap
    h.append(entry)
    _push_heap_hole(h, len(h) - 1, 0, entry)


def heap_pop(h):  # priority_queue::pop = pop_heap + pop_back; returns the former top
    top = h[0]
    last = len(h) - 1
    value = h[last]
    h[last] = h[0]
    # std::__adjust_heap(first, 0, len = last, value)
    length = last
    hole = 0
    second = 0
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if _comp(h[second], h[second - 1]):
            second -= 1
        h[hole] = h[second]
        hole = second
    if (length & 1) == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        h[hole] = h[second - 1]
        hole = second - 1
    _push_heap_hole(h, hole, 0, value)
    h.pop()
    return top


def pq_script(ops, ids, keys):
    """The same command script as oracle.pq_script: op 0 pushes (id, key), op 1 pops (-1 on an empty queue)."""
    h, out = [], []
    for o, i, k in zip(ops, ids, keys):
        if o == 0:
            heap_push(h, (int(i), float(k)))
        else:
            out.append(heap_pop(h)[0] if h else -1)
    return np.array(out, dtype=np.int32)


# ---- the MPA in the form the search reads it
class JointMpa:
    def __init__(self, mpa):
        self.n = mpa.n_trims
        self.trans = np.asarray(mpa.transition_matrix_single) != 0  # (n, n, Hp)
        self.man = mpa.maneuvers

    def successors(self, trim, k_exp):
        """find(mpa.transition_matrix_single(trim, :, k_exp)), 1-based, ascending (expand_node.m:18)."""
        return [j + 1 for j in np.flatnonzero(self.trans[trim - 1, :, k_exp - 1])]

    def maneuver(self, t1, t2):
        return self.man[t1 - 1][t2 - 1]


def child_tuples(per_vehicle):
    """The children of a node in expand_node.m's order: cartprod over the vehicles' successor lists, vehicle 1 varying fastest."""
    out = []
    total = 1
    for s in per_vehicle:
        total *= len(s)
    for t in range(total):
        rest, tup = t, []
        for s in per_vehicle:
            tup.append(s[rest % len(s)])
            rest //= len(s)
        out.append(tuple(tup))
    return out


def _place(area, c, s, px, py):
    # c * area(1, :) - s * area(2, :) + pX; s * area(1, :) + c * area(2, :) + pY              GraphSearch.m:158-159
    a = np.asarray(area, dtype=np.float64)
    return np.vstack([c * a[0] - s * a[1] + px, s * a[0] + c * a[1] + py])


def _boundary(it):
    left, right = it.predicted_lanelet_boundary
    left = np.zeros((2, 0)) if left is None else np.asarray(left, dtype=np.float64)
    right = np.zeros((2, 0)) if right is None else np.asarray(right, dtype=np.float64)
    return left, right


def search(options, jm, iters, max_nodes):
    """One joint problem -> (list of N records, dict with the tree and the pop sequence)."""
    Hp = options.Hp
    N = len(iters)
    recs = np.zeros(N, dtype=abi.VEHICLE_OUT_DTYPE)
    recs["y_predicted"][:] = np.nan
    recs["n_hp"] = Hp
    ref = [np.asarray(it.reference_trajectory_points, dtype=np.float64) for it in iters]
    vref = [np.asarray(it.v_ref, dtype=np.float64) for it in iters]
    bounds = [_boundary(it) for it in iters]
    # tree: per node (parent, k, g, h, [(x, y, yaw, trim) per vehicle])                                  Tree.m:3-13
    parent = [0]
    kk = [0]
    gg = [0.0]
    hh = [0.0]
    pose = [[(float(it.x0[0]), float(it.x0[1]), float(it.x0[2]), int(it.trim_index)) for it in iters]]
    pq = []
    heap_push(pq, (1, 0.0))
    pops = []
    status = EXHAUSTED
    goal = 0
    while True:
        if not pq:
            break
        cur = heap_pop(pq)[0]
        pops.append(cur)
        par = parent[cur - 1]
        cK = kk[cur - 1]
        if par:
            # ---- eval_edge_exact: every vehicle's areas from the parent's pose, then its constraints           :130-193
            ppose = pose[par - 1]
            s_arr, c_arr = oracle.sincos(np.array([p[2] for p in ppose]))
            shapes, shapes_bc = [], []
            valid = True
            for v in range(N):
                px, py, _, t1 = ppose[v]
                t2 = pose[cur - 1][v][3]
                m = jm.maneuver(t1, t2)
                c, s = float(c_arr[v]), float(s_arr[v])
                shapes.append(_place(m.area, c, s, px, py))
                shapes_bc.append(_place(m.area_large_offset if cK == Hp else m.area_without_offset, c, s, px, py))
            for v in range(N):  # are_constraints_satisfied_sat.m:15-53 (the hdv loop :55-66 is unreachable)
                it = iters[v]
                for o in it.obstacles:
                    if oracle.intersect_sat(shapes[v], o):
                        valid = False
                        break
                if valid:
                    for row in it.dynamic_obstacle_area:
                        if oracle.intersect_sat(shapes[v], row[cK - 1]):
                            valid = False
                            break
                if valid:
                    for u in range(v - 1, -1, -1):
                        if oracle.intersect_sat(shapes[u], shapes[v]):
                            valid = False
                            break
                if valid:
                    left, right = bounds[v]
                    if oracle.intersect_lanelet_boundary(shapes_bc[v], left, right):
                        valid = False
                if not valid:
                    break
            if not valid:
                continue
        if cK == Hp:
            status = OK
            goal = cur
            break
        # ---- expand_node.m
        k_exp = cK + 1
        cur_pose = pose[cur - 1]
        succ = [jm.successors(p[3], k_exp) for p in cur_pose]
        children = child_tuples(succ)
        if len(parent) + len(children) > max_nodes:
            status = ARENA_OVERFLOW
            break
        s_arr, c_arr = oracle.sincos(np.array([p[2] for p in cur_pose]))
        steps_to_go = Hp - k_exp
        new_open = []
        for tup in children:
            g = gg[cur - 1]
            h = 0.0
            node = []
            for v in range(N):
                x, y, yaw, t1 = cur_pose[v]
                t2 = tup[v]
                m = jm.maneuver(t1, t2)
                c, s = float(c_arr[v]), float(s_arr[v])
                ex = c * m.dx - s * m.dy + x
                ey = s * m.dx + c * m.dy + y
                eyaw = yaw + m.dyaw
                ddx = ex - ref[v][k_exp - 1, 0]
                ddy = ey - ref[v][k_exp - 1, 1]
                nrm = math.sqrt(ddx * ddx + ddy * ddy)
                g = g + nrm * nrm
                dmax = 0.0
                for i_t in range(1, steps_to_go + 1):
                    dmax = dmax + options.dt_seconds * vref[v][k_exp + i_t - 1]
                    ddx = ex - ref[v][k_exp + i_t - 1, 0]
                    ddy = ey - ref[v][k_exp + i_t - 1, 1]
                    nrm = math.sqrt(ddx * ddx + ddy * ddy)
                    diff = nrm - dmax
                    m0 = diff if diff > 0 else 0.0
                    h = h + m0 * m0
                node.append((float(ex), float(ey), float(eyaw), int(t2)))
            parent.append(cur)
            kk.append(k_exp)
            gg.append(float(g))
            hh.append(float(h))
            pose.append(node)
            new_open.append((len(parent), float(g) * 1 + float(h) * 1))
        for e in new_open:
            heap_push(pq, e)
    recs["status"] = status
    recs["n_expanded"] = len(parent)
    recs["n_popped"] = len(pops)
    if status == OK:
        path = [goal]
        while path[-1] != 1:
            path.append(parent[path[-1] - 1])
        path = path[::-1]
        for v in range(N):
            r = recs[v]
            for i, nd in enumerate(path):
                x, y, yaw, trim = pose[nd - 1][v]
                r["tree_path"][i] = nd
                r["path_nodes"][i] = [x, y, yaw, trim, gg[nd - 1], hh[nd - 1], kk[nd - 1], 1.0]
                if i >= 1:
                    r["y_predicted"][i - 1] = [x, y, yaw]
                    r["predicted_trims"][i - 1] = trim
                    px, py, pyaw, t1 = pose[path[i - 1] - 1][v]
                    m = jm.maneuver(t1, trim)
                    s_, c_ = oracle.sincos(np.array([pyaw]))
                    sh = _place(m.area, float(c_[0]), float(s_[0]), px, py)
                    r["shape_cols"][i - 1] = sh.shape[1]
                    r["shapes"][i - 1][:, : sh.shape[1]] = sh
    tree = {"parent": np.array(parent), "k": np.array(kk), "g": np.array(gg), "h": np.array(hh), "pose": pose}
    return recs, {"pops": pops, "tree": tree}


def arena_nodes(options):
    """The arena of a handle created with options.max_nodes (0: 32768), rounded up to even as the backend does."""
    m = options.max_nodes if options.max_nodes > 0 else 32768
    return (m + 1) & ~1


def plan_joint(options, mpa, problems, max_nodes=None):
    """The records pdmpc_plan_joint returns for `problems` (lists of VehicleIter), in input order.  max_nodes=None: an
    unbounded tree, as the reference's."""
    jm = JointMpa(mpa)
    cap = max_nodes if max_nodes is not None else (1 << 62)
    out = [search(options, jm, prob, cap)[0] for prob in problems]
    return np.concatenate(out) if out else np.zeros(0, dtype=abi.VEHICLE_OUT_DTYPE)
