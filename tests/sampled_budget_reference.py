"""CPU restatement of the sampled optimizer with its expansion budget as a parameter.  TEST INFRASTRUCTURE ONLY.

MonteCarloTreeSearch.do_graph_search (hlc/optimizer/graph_search/MonteCarloTreeSearch.m:40-249) with n_expansions_max (:8, which the
constructor, :16-26, overrides from config/mcts.json) as an argument, vectorize_all_obstacles.m:1-66 restated here, and
are_constraints_satisfied_sat.m / _interx.m on the oracle's exported primitives (oracle.interx, intersect_sat,
intersect_lanelet_boundary, sincos, mt19937_doubles), as tests/joint_reference.py builds the joint search.  At budget 250 it is the
oracle's own restatement (oracle.plan_batch_sampled), byte for byte: tests/test_sampled_budget_reference.py pins that.  Python floats
and numpy's element-wise products and sums are IEEE doubles evaluated operation by operation, the arithmetic of the oracle and of the
kernels (-ffp-contract=off).

Two rules of the kernels that the reference does not have, because it would have failed instead: a random number beyond the
Hp * budget drawn ones is the last one, and Seed = 0 is the generator's default seed 5489.

Records come out in abi.VEHICLE_OUT_DTYPE.  plan_step_sampled is the level-by-level step of tests/sampled_step_reference.py with the
planner as an argument."""
import copy
import math

import numpy as np

from pdmpc import abi

from oracle import oracle

OK, EXHAUSTED = abi.OK, abi.EXHAUSTED
DEFAULT_BUDGET = 250

_NAN_COL = np.array([[np.nan], [np.nan]])


class SampledMpa:
    """The automaton in the form the descents read it: successor_trims{trim, step} and the maneuvers."""

    def __init__(self, mpa):
        self.n = mpa.n_trims
        trans = np.asarray(mpa.transition_matrix_single) != 0  # (n, n, Hp)
        self.succ = [[[j + 1 for j in np.flatnonzero(trans[i, :, k])] for k in range(trans.shape[2])] for i in range(self.n)]
        self.man = mpa.maneuvers

    def successors(self, trim, step):
        """find(mpa.transition_matrix_single(trim, :, step)), 1-based, ascending."""
        return self.succ[trim - 1][step - 1]

    def maneuver(self, t1, t2):
        return self.man[t1 - 1][t2 - 1]


def _poly(a):
    return np.zeros((2, 0)) if a is None else np.asarray(a, dtype=np.float64).reshape(2, -1)


def _with_nan(polys):
    # cellfun(@(c)[c, [nan; nan]], ...) and horzcat                                          vectorize_all_obstacles.m
    parts = []
    for p in polys:
        parts += [_poly(p), _NAN_COL]
    return np.ascontiguousarray(np.hstack(parts)) if parts else np.zeros((2, 0))


def vectorize_all_obstacles(it, Hp):
    """vectorize_all_obstacles.m:1-66 -> (vehicle_obstacles {1 x Hp}, hdv_obstacles {1 x Hp}, lanelet_boundary)."""
    left, right = it.predicted_lanelet_boundary
    boundary = _with_nan([left, right])  # [left, NaN, right, NaN]                                :27-30
    vehicle, hdv = [], []
    for k in range(Hp):  # :36-62
        vehicle.append(_with_nan(list(it.obstacles) + [row[k] for row in it.dynamic_obstacle_area]))
        hdv.append(_with_nan([row[k] for row in it.hdv_reachable_sets]))
    return vehicle, hdv, boundary


def _place(area, ncols, c, s, px, py):
    # transform(1:2,1:2) * area + start_pose(1:2)                                               MonteCarloTreeSearch.m:159-166
    a = np.asarray(area, dtype=np.float64)[:, :ncols]
    return np.ascontiguousarray(np.vstack([(c * a[0] + (-s) * a[1]) + px, (s * a[0] + c * a[1]) + py]))


class _Checker:
    """are_constraints_satisfied_sat.m:13-66 / are_constraints_satisfied_interx.m:13-37 for one vehicle."""

    def __init__(self, checker, it, Hp):
        self.sat = checker == abi.CHECK_SAT
        self.it = it
        left, right = it.predicted_lanelet_boundary
        self.left, self.right = _poly(left), _poly(right)
        if not self.sat:
            self.vehicle, self.hdv, self.boundary = vectorize_all_obstacles(it, Hp)
            self.hdv_all_nan = [bool(np.all(np.isnan(h))) for h in self.hdv]

    def satisfied(self, shape, shape_bc, i_step):
        if self.sat:
            for o in self.it.obstacles:
                if oracle.intersect_sat(shape, o):
                    return False
            for row in self.it.dynamic_obstacle_area:
                if oracle.intersect_sat(shape, row[i_step - 1]):
                    return False
            return not oracle.intersect_lanelet_boundary(shape_bc, self.left, self.right)
        if oracle.interx(shape, self.vehicle[i_step - 1]):
            return False
        if not self.hdv_all_nan[i_step - 1] and oracle.interx(shape, self.hdv[i_step - 1]):
            return False
        return not oracle.interx(shape_bc, self.boundary)


def _apply(pose, m, c, s):
    # node_pose + transform * maneuver.dpose: a 3x3 product, each row accumulated left to right, zeros included    :131-138
    t0 = c * m.dx + (-s) * m.dy + 0.0 * m.dyaw
    t1 = s * m.dx + c * m.dy + 0.0 * m.dyaw
    t2 = 0.0 * m.dx + 0.0 * m.dy + 1.0 * m.dyaw
    return (pose[0] + t0, pose[1] + t1, pose[2] + t2)


def search(options, sm, it, seed, budget, checker=None, tree_sizes=None):
    """One vehicle -> its record.  budget = n_expansions_max.  tree_sizes: a list that receives the tree's nodes, the root included."""
    Hp = options.Hp
    if checker is None:
        checker = abi.CHECK_INTERX if options.are_any_obstacles_non_convex else abi.CHECK_SAT
    rec = np.zeros((), dtype=abi.VEHICLE_OUT_DTYPE)
    rec["n_hp"] = Hp
    rec["y_predicted"][:] = np.nan
    n_random = Hp * budget
    random_numbers = oracle.mt19937_doubles(int(seed) if int(seed) else 5489, n_random)  # :53
    sincos = {}

    def sc(yaw):
        v = sincos.get(yaw)
        if v is None:
            s_, c_ = oracle.sincos(np.array([yaw]))
            v = sincos[yaw] = (float(s_[0]), float(c_[0]))
        return v

    ref = np.asarray(it.reference_trajectory_points, dtype=np.float64)
    root_pose = (float(it.x0[0]), float(it.x0[1]), float(it.x0[2]))
    # :60-74 (node ids are 1-based; the arrays grow with the tree: the reference has no capacity)
    trims = [0, int(it.trim_index)]
    parents = [0, 0]
    children = [None, {q: 1 for q in range(len(sm.successors(int(it.trim_index), 1)))}]  # children(position, node) != 0
    shapes = [None, None]
    check = _Checker(checker, it, Hp)
    best = None  # valid_nodes_at_hp: only its top is ever read (:197); the first of the cheapest stays on top
    n_expansions = n_traversals = 0
    is_finished = False
    while n_expansions < budget and not is_finished:  # :89
        node_id = 1
        solution_cost = 0.0
        pose = root_pose
        is_valid = False
        child_position = node_parent = 0
        for i_step in range(1, Hp + 1):  # :95
            is_valid = False
            n_traversals += 1
            trim_positions = sorted(children[node_id])  # find(children(:, node_id))                          :100
            n_trims = len(trim_positions)
            if n_trims != 0:
                r = random_numbers[min(n_traversals, n_random) - 1]
                child_position = trim_positions[max(int(math.ceil(r * float(n_trims))) - 1, 0)]  # :105
            else:
                if node_id != 1:  # remove edge to node without children                                   :108-112
                    ch = children[parents[node_id]]
                    for q in [q for q, v in ch.items() if v == node_id]:
                        del ch[q]
                    break
                is_finished = True  # :114-115
                break
            parent_trim = trims[node_id]
            goal_trim = sm.successors(parent_trim, i_step)[child_position]
            m = sm.maneuver(parent_trim, goal_trim)
            s, c = sc(pose[2])
            start = pose
            pose = _apply(pose, m, c, s)
            ddx, ddy = pose[0] - ref[i_step - 1, 0], pose[1] - ref[i_step - 1, 1]
            nrm = math.sqrt(ddx * ddx + ddy * ddy)
            solution_cost = solution_cost + nrm * nrm  # :143
            if children[node_id][child_position] != 1:  # is_expanded                                      :145-150
                node_id = children[node_id][child_position]
                continue
            n_expansions += 1  # :152
            node_parent = node_id
            ncols = np.asarray(m.area).shape[1]
            shape = _place(m.area, ncols, c, s, start[0], start[1])
            shape_bc = _place(m.area_large_offset if i_step == Hp else m.area_without_offset, ncols, c, s, start[0], start[1])
            is_valid = check.satisfied(shape, shape_bc, i_step)  # :170-179
            if not is_valid:
                del children[node_parent][child_position]  # :183
                break
            trims.append(goal_trim)  # :186-193
            parents.append(node_parent)
            children.append({q: 1 for q in range(len(sm.successors(goal_trim, i_step + 1)))} if i_step != Hp else {})
            shapes.append(shape)
            node_id = len(trims) - 1
            children[node_parent][child_position] = node_id
        if is_valid:  # :199-203
            if best is None or solution_cost < best[0]:
                best = (solution_cost, node_id)
            del children[node_parent][child_position]  # avoid double exploration
    if tree_sizes is not None:
        tree_sizes.append(len(trims) - 1)
    rec["n_expanded"] = n_expansions  # :209
    rec["n_popped"] = n_traversals
    if best is None:  # :212-215
        rec["status"] = EXHAUSTED
        return rec
    best_cost, best_node = best
    path = [best_node]
    while path[-1] != 1:
        path.append(parents[path[-1]])
    path = path[::-1]
    pose = root_pose
    for i, nd in enumerate(path):  # :217-248
        if i >= 1:
            m = sm.maneuver(trims[path[i - 1]], trims[nd])
            s, c = sc(pose[2])
            pose = _apply(pose, m, c, s)
        rec["tree_path"][i] = nd
        rec["path_nodes"][i] = [pose[0], pose[1], pose[2], trims[nd], best_cost if nd == best_node else -1.0, -1.0, i + 1, 1.0]
        if i >= 1:
            rec["y_predicted"][i - 1] = pose
            rec["predicted_trims"][i - 1] = trims[nd]
            sh = shapes[nd]
            rec["shape_cols"][i - 1] = sh.shape[1]
            rec["shapes"][i - 1][:, : sh.shape[1]] = sh
    rec["status"] = OK
    return rec


def plan_batch_sampled(options, mpa, iters, seeds, budget=DEFAULT_BUDGET, checker=None, tree_sizes=None):
    """The records pdmpc_plan_batch_sampled returns for `iters` on a handle with pdmpc_set_sampled_budget(budget); tree_sizes: as in
    search, one entry per vehicle."""
    sm = mpa if isinstance(mpa, SampledMpa) else SampledMpa(mpa)
    out = np.zeros(len(iters), dtype=abi.VEHICLE_OUT_DTYPE)
    for i, (it, seed) in enumerate(zip(iters, seeds)):
        out[i] = search(options, sm, it, seed, budget, checker, tree_sizes)
    return out


def plan_step_sampled(options, mpa, problem, seeds, planner):
    """A whole step level by level with the hand-over rules of tests/sampled_step_reference.py: an OK predecessor contributes its
    solved areas, an exhausted one its fallback areas if it has any, and an exhausted slot's record carries its fallback areas.
    planner(iters, seeds) -> records of one level (e.g. lambda i, s: plan_batch_sampled(options, sm, i, s, budget))."""
    Hp = options.Hp
    n = len(problem["iters"])
    recs = np.zeros(n, dtype=abi.VEHICLE_OUT_DTYPE)
    first = 0
    for size in problem["level_sizes"]:
        slots = list(range(first, first + size))
        iters = []
        for s in slots:
            it = copy.copy(problem["iters"][s])
            dyn = list(it.dynamic_obstacle_area)
            for p in problem["preds"][s]:
                assert p < first, "slots are not in level order"
                if int(recs[p]["status"]) == 0:
                    dyn.append([np.array(recs[p]["shapes"][k][:, : int(recs[p]["shape_cols"][k])]) for k in range(Hp)])
                else:
                    fb = problem["fallback"][p]
                    if fb is not None and len(fb):
                        dyn.append([np.asarray(a, dtype=np.float64) for a in fb])
            it.dynamic_obstacle_area = dyn
            iters.append(it)
        out = planner(iters, [seeds[s] for s in slots])
        for q, s in enumerate(slots):
            recs[s] = out[q]
            if int(out[q]["status"]) != 0:
                fb = problem["fallback"][s]
                if fb is not None and len(fb):
                    for k in range(Hp):
                        a = np.asarray(fb[k], dtype=np.float64)
                        recs[s]["shape_cols"][k] = a.shape[1]
                        recs[s]["shapes"][k][:, : a.shape[1]] = a
        first += size
    return recs
