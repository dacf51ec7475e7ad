"""The joint search (csrc/joint_kernel.hip) at its horizon, vehicle, automaton and layout limits: the cases, built once for the CPU
half (tests/test_joint_limit_cases.py, which proves each case reaches what it names) and the GPU half
(tests/test_gpu_joint_limits.py, which compares the kernel with tests/joint_reference.py byte for byte).

What keeps Hp 16 affordable for the Python reference: ON-PATH problems.  Every vehicle's reference trajectory is laid on a maneuver
path of the automaton -- from the start trim, the same trim at every step where transition_matrix_single allows it, otherwise the
first allowed successor --, advanced with the search's own arithmetic (oracle.sincos, c * dx - s * dy + x, ...), with the visited
trims' speeds as v_ref.  Along that path g stays at rounding level and h is 0, so the search runs depth first; an obstacle on the
path, a varied path or a standing vehicle beside moving ones makes it back up by a controlled amount.

Every case and every reference search is computed once per session (functools.lru_cache) and shared; callers must not write into one.
"""
import dataclasses
import functools
import math

import numpy as np

from pdmpc import abi
from pdmpc.centralized import centralized_mpa, centralized_options
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.iteration_data import VehicleIter

import centralized_cases as cc
import joint_reference as jr

NODE_CAP = 60000  # nodes of a case's reference search: about 2 s of tests/joint_reference.py
SS, TS, RE = MpaType.single_speed, MpaType.triple_speed, MpaType.realistic


def options_for(mpa_type, N, Hp, **kw):
    return centralized_options(Config(scenario_type=ScenarioType.circle, amount=N, Hp=Hp, mpa_type=mpa_type, max_vehicles=16, **kw))


def first_straight_moving_trim(mpa):
    return [i + 1 for i, t in enumerate(mpa.trims) if t.steering == 0 and t.speed > 0][0]


def standstill_trim(mpa):
    return mpa.trims_stop[0]


def maneuver_path(options, mpa, x0, trim, varied=None):
    """Hp steps from (x0 = (x, y, yaw), trim): [(x, y, yaw, trim)] of steps 1 .. Hp.  The same trim where the transition matrix allows
    it, else the first allowed successor; varied = q: successor number (q + k) % count of step k instead (a path that changes its
    trims).  The pose arithmetic is the search's (joint_reference.search, expand_node.m:50-55)."""
    from oracle import oracle

    jm = jr.JointMpa(mpa)
    x, y, yaw = (float(q) for q in x0)
    out = []
    for k in range(1, options.Hp + 1):
        succ = jm.successors(trim, k)
        assert succ, "trim %d has no successor at step %d" % (trim, k)
        nxt = succ[(varied + k) % len(succ)] if varied is not None else (trim if trim in succ else succ[0])
        m = jm.maneuver(trim, nxt)
        s_, c_ = oracle.sincos(np.array([yaw]))
        c, s = float(c_[0]), float(s_[0])
        x, y, yaw, trim = c * m.dx - s * m.dy + x, s * m.dx + c * m.dy + y, yaw + m.dyaw, int(nxt)
        out.append((x, y, yaw, trim))
    return out


def on_path_problem(options, mpa, start_trims, spacing=3.0, yaw_step=0.3, varied=False, origin=(0.0, 0.0)):
    """(iters, paths): one vehicle per start trim, vehicle v at (origin x, origin y + spacing * v) with yaw yaw_step * v, its
    reference trajectory on its maneuver path (paths[v], see maneuver_path) and v_ref the speeds of the path's trims."""
    N = len(start_trims)
    iters, paths = [], []
    for v, trim in enumerate(start_trims):
        x0 = (origin[0], origin[1] + spacing * v, yaw_step * v)
        path = maneuver_path(options, mpa, x0, int(trim), varied=v if varied else None)
        paths.append(path)
        iters.append(
            VehicleIter(
                x0=np.array([x0[0], x0[1], x0[2], mpa.trims[trim - 1].speed]),
                trim_index=int(trim),
                reference_trajectory_points=np.array([[p[0], p[1]] for p in path]),
                v_ref=np.array([mpa.trims[p[3] - 1].speed for p in path]),
                amount=N,
            )
        )
    return iters, paths


def with_step_rectangle(iters, paths, u, k, into=None, at_step=None):
    """Copies of `iters` in which every vehicle has a dynamic_obstacle_area of its own: one row of Hp rectangles far from every path,
    and in vehicle `into`'s row (default u) at step `at_step` (default k) a rectangle of 6 cm beside vehicle u's on-path pose of
    step k, where the on-path maneuver of step k meets it and another one does not (a maneuver's area reaches from 0.12 m behind its
    start pose to 0.28 m ahead of it, 0.2 m for one that brakes to standstill, and 0.06 m to either side): at step 1, 0.1 m ahead
    of the pose the step ends at -- full speed hits it, braking does not --, at a later step 0.08 m to the left of it.
    k = None: the far rectangles alone."""
    Hp = len(paths[0])
    out = []
    for v, it in enumerate(iters):
        row = [cc.rectangle(60.0 + 2.0 * v, 60.0 + 0.5 * s, 0.2, 0.1) for s in range(Hp)]
        out.append(dataclasses.replace(it, dynamic_obstacle_area=[row]))
    if k is not None:
        x, y, yaw = paths[u][k - 1][:3]
        ahead, side = (0.1, 0.0) if k == 1 else (0.0, 0.08)
        x, y = x + ahead * math.cos(yaw) - side * math.sin(yaw), y + ahead * math.sin(yaw) + side * math.cos(yaw)
        out[u if into is None else into].dynamic_obstacle_area[0][(k if at_step is None else at_step) - 1] = cc.rectangle(x, y, 0.03, 0.03)
    return out


# ---- what a launch stages of a problem, and where layout_joint puts it


def soup_columns(problem, Hp):
    """pdmpc_joint_soup_columns of a problem as Handle.plan_joint hands it over: every polygon with a separator column, the static
    ones and each row's polygon of the step once per step; a vehicle whose obstacle lists hold the same array objects as an earlier
    one's takes over that one's soup (abi._Keep.polygon_set, pack.cpp's obstacle_key); a boundary is its points and two separators
    (the arrays of two vehicles are never the same: abi.pack_vehicle copies the rows)."""
    seen, need = set(), 0
    for it in problem:
        key = (tuple(id(o) for o in it.obstacles), tuple(id(o) for row in it.dynamic_obstacle_area for o in row), tuple(id(o) for row in it.hdv_reachable_sets for o in row))
        if key not in seen:
            seen.add(key)
            need += Hp * sum(o.shape[1] + 1 for o in it.obstacles) + sum(o.shape[1] + 1 for row in it.dynamic_obstacle_area for o in row)
        left, right = it.predicted_lanelet_boundary
        need += sum(0 if side is None else np.shape(side)[1] for side in (left, right)) + 2
    return need


def launch_soup_cap(problems, Hp):
    """dims.soup_cap of pdmpc_plan_joint for a launch of `problems`"""
    return max(soup_columns(p, Hp) for p in problems) + 2


def n_maneuvers(mpa):
    return sum(1 for row in mpa.maneuvers for m in row if m is not None)


def joint_plan(options, mpa, soup_cap):
    """(rc, plan) of pdmpc_launch_plan_host for a joint launch with this soup_cap, and the pass of layout_joint the plan is from"""
    from test_sampled_budget_reference import launch_plan

    rc, p = launch_plan(dict(checker=abi.CHECK_SAT, Hp=options.Hp, n_trims=mpa.n_trims, n_man=n_maneuvers(mpa), n_cu=256, device_share=1, max_nodes=1 << 15, kind=2, count=1,
                             n_chained=0, soup_cap=soup_cap, ll_cap=0, cand_cap=0, safe=0))
    if rc == 0:
        p["pass"] = (0 if p["areas_in_lds"] else 1) + (2 if p["total"] > 64 * 1024 else 0)
    return rc, p


def pass_capacity(mpa, Hp, p):
    budget, areas = cc.JOINT_PASSES[p]
    return cc.joint_soup_capacity(mpa, Hp, budget, areas)


# ---- the cases


@dataclasses.dataclass
class Case:
    name: str
    options: object
    mpa: object
    problem: list  # of VehicleIter
    paths: list
    claims: dict  # what the case is for: tests/test_joint_limit_cases.py asserts each key


def _case(name, mpa_type, Hp, start, claims=None, **kw):
    options = options_for(mpa_type, len(start), Hp)
    mpa = centralized_mpa(options)
    trims = [first_straight_moving_trim(mpa) if s == "m" else (standstill_trim(mpa) if s == "s" else int(s)) for s in start]
    iters, paths = on_path_problem(options, mpa, trims, **kw)
    return Case(name, options, mpa, iters, paths, dict(claims or {}))


# name, vehicles, Hp, the steps k.  (Three vehicles at Hp 4: at Hp 5 the rectangle of step 3 already costs the reference 18 434 nodes.)
SOUP_SETS = (("soup2", 2, 16, (1, 8, 16)), ("soup3", 3, 4, (1, 2, 4)))
SOUP_VEHICLE = 1  # the vehicle u whose path the rectangle lies on
OPEN_LIST_HP = 3


def shifted_step(k, Hp):
    """a step three away from k (the areas of that step's maneuvers are half a metre from the rectangle of step k); None: Hp has none"""
    return k + 3 if k + 3 <= Hp else (k - 3 if k - 3 >= 1 else None)


def adjacent_step(k, Hp):
    return k + 1 if k + 1 <= Hp else k - 1


def open_list_rectangles(mpa, p, last):
    """R for the small-open-list case of pass p: the last R whose soup_cap (15 columns a rectangle at Hp 3, two [NaN, NaN]
    boundaries, layout_joint's two) pass p still takes -- fewer than 15 columns of 16 bytes are left over, so the open list gets
    256 entries of LDS --, or the first one of pass p (one more than pass p - 1's last)."""
    per, other = 5 * OPEN_LIST_HP, 2 * 2 + 2
    return (pass_capacity(mpa, OPEN_LIST_HP, p) - other) // per if last else (pass_capacity(mpa, OPEN_LIST_HP, p - 1) - other) // per + 1


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}, in the order of the issue's list"""
    out = []
    # -- the horizon: N * (Hp + 1) items of the read-back, 68 (a second stride of the wavefront) and 64 (exactly one)
    out.append(_case("ss_4_16", SS, 16, "mmmm", {"items": 68, "children": {1, 256}}))
    out.append(_case("ss_4_15", SS, 15, "mmmm", {"items": 64, "children": {1, 256}}))
    out.append(_case("ss_3_16", SS, 16, "mmm", {"items": 51, "children": {1, 64}}))
    out.append(_case("ss_1_16", SS, 16, "m", {"items": 17}))
    out.append(_case("ss_2_16_varied", SS, 16, "mm", {"items": 34, "backs_up": 1000}, varied=True))
    # -- the automata.  triple_speed (34 trims) with three vehicles and realistic (71 trims, two mask words) with four overflow 2^18
    # nodes on their on-path problems; realistic with three fits.  The realistic automaton's first straight moving trim is 20 and its
    # path stays below 64; trim 67 is the straight one at full speed (0.768 m/s), and its path brakes through 66, 58, 48, ...: the
    # winning path and the expanded nodes' successor lists hold trims above 64, read from the second mask word.  One vehicle from
    # trim 67 is cheap at Hp 16 (493 nodes); two have 67 051 nodes there, above the cap, and 30 403 at Hp 14, so the two-vehicle case
    # with trims above 64 runs at Hp 14.
    out.append(_case("ts_2_16", TS, 16, "mm", {"n_words": 1, "n_trims": 34}))
    out.append(_case("ts_1_16", TS, 16, "m", {"n_words": 1, "n_trims": 34}))
    out.append(_case("re_3_16", RE, 16, "mmm", {"n_words": 2, "n_trims": 71}))
    out.append(_case("re_1_16_from_67", RE, 16, (67,), {"n_words": 2, "trim_above_64": True, "crosses_words": True}))
    out.append(_case("re_2_14_from_67", RE, 14, (67, 67), {"n_words": 2, "trim_above_64": True, "crosses_words": True}))
    # -- per-step soups: see with_step_rectangle
    for name, N, Hp, ks in SOUP_SETS:
        base = _case(name + "_free", SS, Hp, "m" * N)
        u = SOUP_VEHICLE

        def variant(tag, claims, *a, **kw):
            return Case("%s_%s" % (name, tag), base.options, base.mpa, with_step_rectangle(base.problem, base.paths, *a, **kw), base.paths, claims)

        out.append(variant("free", {}, u, None))
        for k in ks:
            out.append(variant("k%d_at" % k, {"differs_from": name + "_free"}, u, k))
            out.append(variant("k%d_other" % k, {"equals": name + "_free"}, u, k, into=0))
            if shifted_step(k, Hp) is not None:
                out.append(variant("k%d_shifted" % k, {"equals": name + "_free"}, u, k, at_step=shifted_step(k, Hp)))
            # one step off: a kernel that read step k - 1's or k + 1's soup would return this variant's records for the k_at one.  (Two
            # vehicles only: with three, the rectangle of step 1 in step 2's soup costs the reference more than the cap)
            if N == 2:
                out.append(variant("k%d_adjacent" % k, {"other_records_than": "%s_k%d_at" % (name, k)}, u, k, at_step=adjacent_step(k, Hp)))
    # -- the boundary-check area of step Hp (the large offset: 0.05 m longer at both ends than the one without offset, which the
    # earlier steps check): vehicle 1's left boundary is a bar of 6 cm across its path, 0.22 m ahead of the pose its last step starts
    # from and 0.07 m to the left -- the last maneuver's area without offset ends at 0.19 m, with the large offset at 0.24 m
    base = _case("bound2_16_large_offset", SS, 16, "mm", {"large_offset_only": True})
    x, y, yaw = base.paths[1][-2][:3]
    cx, cy = x + 0.22 * math.cos(yaw) - 0.07 * math.sin(yaw), y + 0.22 * math.sin(yaw) + 0.07 * math.cos(yaw)
    bar = np.array([[cx + 0.03 * math.sin(yaw), cx - 0.03 * math.sin(yaw)], [cy - 0.03 * math.cos(yaw), cy + 0.03 * math.cos(yaw)]])
    base.problem[1] = dataclasses.replace(base.problem[1], predicted_lanelet_boundary=(bar, np.array([[-40.0, -30.0], [-40.0, -40.0]])))
    out.append(base)
    # -- child chunks: 63, 64, 72 (65 to 71 are not products of any automaton's successor counts: single_speed 3, 4, 12;
    # triple_speed 3, 4, 5, 12; realistic 4, 6, 7, 8, 9) in one realistic problem, 144 = two chunks and 16, 192 = three chunks
    out.append(_case("chunks_re_8", RE, 8, (16, 17), {"n_words": 2, "children": {63, 64, 72}}))
    out.append(_case("chunks_ss_144", SS, 16, "ss", {"children": {1, 144}}))
    out.append(_case("chunks_ss_192", SS, 16, "mms", {"children": {1, 192}}))
    # -- the smallest open list, and the pass edges of layout_joint: two vehicles from standstill on a varied path at Hp 3 (the root
    # has 144 children, the search backs up 60 times) that share R far rectangles
    base = _case("open_list", SS, OPEN_LIST_HP, "ss", varied=True)
    for p in range(4):
        for last in (True, False):
            if p == 0 and not last:
                continue
            R = open_list_rectangles(base.mpa, p, last)
            rects = cc.far_rectangles(R)
            prob = [dataclasses.replace(it, obstacles=rects) for it in base.problem]
            out.append(Case("open_list_p%d_%s" % (p, "last" if last else "first"), base.options, base.mpa, prob, base.paths,
                            {"layout": (p, 256 if last else None), "peak_above": 256, "rectangles": R}))
    return {c.name: c for c in out}


HORIZON = {"single_speed": ("ss_4_16", "ss_3_16", "ss_1_16", "ss_2_16_varied"), "triple_speed": ("ts_2_16", "ts_1_16"), "realistic": ("re_3_16", "re_1_16_from_67")}
# the arena edge.  The backend rounds an arena up to an even number of nodes, so of "fits exactly" and "one node short" a case
# reaches the side its tree size n allows: an even n (ss_4_16: 3 842) fits an arena of n exactly, and the next smaller arena is
# n - 2; an odd n (ss_2_16_varied: 31 511) overflows an arena of n - 1, one node short, and the next larger arena is n + 1.
ARENA_EDGE = ("ss_4_16", "ss_2_16_varied")


def arena_edge_sizes(n):
    """(the smallest arena that holds a tree of n nodes, the largest that does not), both even"""
    fits = (n + 1) & ~1
    return fits, fits - 2


def small_problem():
    """one vehicle on its path at Hp 3: the small problem in front of an open_list case in one launch"""
    base = cases()["open_list_p0_last"]
    iters, _ = on_path_problem(base.options, base.mpa, [first_straight_moving_trim(base.mpa)], origin=(0.0, -6.0))
    return iters


def peak_open_list(pops, parent):
    """The longest open list of a search, from its trace: the root, then per pop minus one plus the popped node's children (ids and
    parents 1-based).  Children beyond a cut trace are not counted: a lower bound then."""
    n_children = np.bincount(np.asarray(parent), minlength=len(parent) + 1)
    n, peak = 1, 1
    for nd in pops:
        n += int(n_children[nd]) - 1 if nd < len(n_children) else -1
        peak = max(peak, n)
    return peak


@functools.lru_cache(maxsize=None)
def reference(name, max_nodes=NODE_CAP):
    """(records, facts) of the reference search of a case in an arena of max_nodes nodes: facts = pops, the child counts of the
    expanded nodes, the open list's high-water mark, the expanded nodes' (k, trims)."""
    c = cases()[name]
    recs, info = jr.search(c.options, jr.JointMpa(c.mpa), c.problem, max_nodes)
    parent = info["tree"]["parent"]
    n_children = np.bincount(parent, minlength=len(parent) + 1)
    facts = {
        "n_popped": len(info["pops"]),
        "children": {int(n_children[nd]) for nd in info["pops"] if n_children[nd] > 0},
        "peak": peak_open_list(info["pops"], parent),
        "expanded": {(int(info["tree"]["k"][nd - 1]),) + tuple(int(p[3]) for p in info["tree"]["pose"][nd - 1]) for nd in info["pops"] if n_children[nd] > 0},  # (k, trims)
    }
    recs.setflags(write=False)
    return recs, facts
