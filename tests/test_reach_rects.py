"""The oriented reach rule of the graph search (include/pdmpc_reach.h) on the host, no GPU: the automaton's reach
rectangles (pdmpc_mpa_reach_rects_host) against a brute-force enumeration of every area the automaton can place, the host twin of the
lists (pdmpc_reach_lists_oriented_host) against the rule written out in Python on crafted segments, and the soundness condition on the
oracle's own searches: for every edge the oracle evaluated, InterX over all segments of its step and over the listed ones agree, and
every crossing segment is listed."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from oracle import oracle
from pdmpc import abi, backend
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa
from pdmpc.road_network import boundary_provider, commonroad_scenario

HP_MAX = 16
NAN = float("nan")
INF = float("inf")
DP, IP = abi.c_double_p, abi.c_int32_p
MARGIN, ROTATION, FINITE = 2.0 ** -20, 2.0 ** -48, 2.0 ** 64
AUTOMATA = [MpaType.single_speed, MpaType.triple_speed, MpaType.realistic]


def make_mpa(mpa_type, Hp):
    return get_mpa(Config(scenario_type=ScenarioType.commonroad, amount=2, Hp=Hp, mpa_type=mpa_type, max_vehicles=4, max_nodes=1 << 12))


def native_rects(mpa, Hp):
    s, keep = abi.pack_mpa(mpa)
    out = np.full((mpa.n_trims, Hp, 4), -7.0)
    assert backend.load_library().pdmpc_mpa_reach_rects_host(C.byref(s), Hp, out.ctypes.data_as(DP)) == 0
    del keep
    return out


# ---- (a) the rectangles against an enumeration of all paths -----------------------------------------------------------------
ENUM_LIMIT = 10 ** 5


def path_counts(mpa, Hp):
    """Nodes of the full tree below each root trim (all steps together), from the transition masks alone."""
    T = mpa.transition_matrix_single.astype(np.int64)
    v = np.eye(mpa.n_trims, dtype=np.int64)
    total = np.zeros(mpa.n_trims, dtype=np.int64)
    for k in range(Hp):
        v = v @ T[:, :, k]
        total += v.sum(axis=1)
    return total


def enumerated_rects(mpa, Hp):
    """Per (root trim, step): the bounding box of every point of every area (three variants) of every maneuver the masks allow, the
    poses accumulated as the search accumulates them (expand_node.m:44-51)."""
    n = mpa.n_trims
    T = mpa.transition_matrix_single
    out = np.full((n, Hp, 4), NAN)
    for r in range(n):
        trim, x, y, yaw = np.array([r]), np.zeros(1), np.zeros(1), np.zeros(1)
        for k in range(Hp):
            nt, nx, ny, nyaw = [], [], [], []
            lo = np.array([INF, INF])
            hi = -lo
            for i in np.unique(trim):
                sel = trim == i
                px, py, pyaw = x[sel], y[sel], yaw[sel]
                c, s = np.cos(pyaw), np.sin(pyaw)
                for j in np.nonzero(T[i, :, k])[0]:
                    m = mpa.maneuvers[i][j]
                    pts = np.hstack([m.area, m.area_without_offset, m.area_large_offset])
                    gx = c[:, None] * pts[0][None, :] - s[:, None] * pts[1][None, :] + px[:, None]
                    gy = s[:, None] * pts[0][None, :] + c[:, None] * pts[1][None, :] + py[:, None]
                    lo = np.minimum(lo, [gx.min(), gy.min()])
                    hi = np.maximum(hi, [gx.max(), gy.max()])
                    nt.append(np.full(len(px), j))
                    nx.append(c * m.dx - s * m.dy + px)
                    ny.append(s * m.dx + c * m.dy + py)
                    nyaw.append(pyaw + m.dyaw)
            if not nt:
                break
            out[r, k] = lo[0], hi[0], lo[1], hi[1]
            trim, x, y, yaw = np.concatenate(nt), np.concatenate(nx), np.concatenate(ny), np.concatenate(nyaw)
    return out


@pytest.mark.parametrize("mpa_type", AUTOMATA)
def test_rectangles_hold_the_enumerated_areas_and_are_tight(mpa_type):
    """At the largest horizon whose full tree stays under 10^5 nodes for every root trim.  The native rectangle contains the
    enumerated bounding box and exceeds it by less than 1e-9 m on each side.  "Contains" is up to the rounding of two operation orders
    (hull composition from the leaves, pose accumulation from the root): at most Hp <= 8 compositions of coordinates below 4 m, each
    within a few 2^-52 of its value, 1e-13 m and less; 1e-12 m is allowed."""
    Hp = max(h for h in range(1, 9) if path_counts(make_mpa(mpa_type, h), h).max() < ENUM_LIMIT)
    mpa = make_mpa(mpa_type, Hp)
    got, want = native_rects(mpa, Hp), enumerated_rects(mpa, Hp)
    print("%s: Hp %d, at most %d nodes per root" % (mpa_type, Hp, path_counts(mpa, Hp).max()))
    assert Hp >= 3
    assert np.array_equal(np.isnan(got), np.isnan(want))
    seen = ~np.isnan(want[:, :, 0])
    assert seen[:, 0].all() and seen.sum() > mpa.n_trims
    sign = np.array([-1.0, 1.0, -1.0, 1.0])  # (outwards: x_lo, x_hi, y_lo, y_hi)
    excess = ((got - want) * sign)[seen]
    print("excess of the native rectangle over the enumeration: %.3g .. %.3g m" % (excess.min(), excess.max()))
    assert excess.min() >= -1e-12 and excess.max() < 1e-9
    # shorter horizons of the same automaton are the first steps of the table (the masks of steps 1 .. k decide step k)
    assert np.array_equal(native_rects(mpa, Hp - 1), got[:, : Hp - 1], equal_nan=True)


def test_first_trim_of_the_single_speed_automaton_at_hp_8():
    r = native_rects(make_mpa(MpaType.single_speed, 8), 8)[0, 7]
    assert np.allclose(r, [-0.160, 1.283, -0.862, 0.862], atol=5e-4), r


def test_rects_arguments():
    mpa = make_mpa(MpaType.single_speed, 4)
    s, keep = abi.pack_mpa(mpa)
    out = np.zeros((mpa.n_trims, HP_MAX + 1, 4))
    L = backend.load_library()
    for Hp in (0, 5, HP_MAX + 1):  # (beyond the automaton's masks, beyond the kernel's horizon)
        assert L.pdmpc_mpa_reach_rects_host(C.byref(s), Hp, out.ctypes.data_as(DP)) != 0
    assert L.pdmpc_mpa_reach_rects_host(C.byref(s), 4, None) != 0
    del keep


# ---- (b) the rule, written out (pdmpc_reach.h says the same in C) -----------------------------------------------------------
def widened(rect, rx, ry):
    e = max(max(abs(rect[0]), abs(rect[1])), max(abs(rect[2]), abs(rect[3])))
    m = MARGIN * (1.0 + abs(rx) + abs(ry) + e)
    return rect[0] - m, rect[1] + m, rect[2] - m, rect[3] + m


def root_frame(px, py, rx, ry, cs, sn):
    dx, dy = px - rx, py - ry
    return cs * dx + sn * dy, cs * dy - sn * dx


def in_reach(seg, rect, rx, ry, yaw):
    x0, y0, x1, y1 = seg
    if any(math.isnan(c) for c in seg):
        return False
    if not all(abs(c) <= FINITE for c in seg):
        return True
    s, c = oracle.sincos(np.array([yaw]))
    cs, sn = float(c[0]), float(s[0])
    x_lo, x_hi, y_lo, y_hi = widened(rect, rx, ry)
    u0, v0 = root_frame(x0, y0, rx, ry, cs, sn)
    u1, v1 = root_frame(x1, y1, rx, ry, cs, sn)
    slack = ROTATION * (abs(x0 - rx) + abs(y0 - ry) + abs(x1 - rx) + abs(y1 - ry))
    return not (max(u0, u1) < x_lo - slack or min(u0, u1) > x_hi + slack or max(v0, v1) < y_lo - slack or min(v0, v1) > y_hi + slack)


def ranges(Hp, n, only=None):
    count = np.array([n if only in (None, k) else 0 for k in range(1, Hp + 1)], dtype=np.int32)
    return np.zeros(Hp, dtype=np.int32), count


def twin(Hp, rects, trim, rx, ry, yaw, x, y, rng):
    L = backend.load_library()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    rects = np.ascontiguousarray(rects, dtype=np.float64)
    first, count = (np.ascontiguousarray(a, dtype=np.int32) for a in rng)
    lo = np.zeros(Hp + 1, dtype=np.int32)
    lst = np.full(max(int(count.sum()), 1), -1, dtype=np.int32)
    rc = L.pdmpc_reach_lists_oriented_host(Hp, rects.shape[0], rects.ctypes.data_as(DP), trim, rx, ry, yaw, x.ctypes.data_as(DP), y.ctypes.data_as(DP), first.ctypes.data_as(IP),
                                           count.ctypes.data_as(IP), lo.ctypes.data_as(IP), lst.ctypes.data_as(IP))
    assert rc == 0
    return [lst[lo[k]:lo[k + 1]].tolist() for k in range(Hp)]


def brute(Hp, rects, trim, rx, ry, yaw, x, y, rng):
    out = []
    for k in range(1, Hp + 1):
        a, c = int(rng[0][k - 1]), int(rng[1][k - 1])
        out.append([j for j in range(max(c - 1, 0)) if in_reach((x[a + j], y[a + j], x[a + j + 1], y[a + j + 1]), rects[trim - 1, k - 1], rx, ry, yaw)])
    return out


ROOT = (2.25, -1.5)
YAWS = [0.0, math.pi / 4, 3 * math.pi / 4, -math.pi / 2, 2.0]


def flip_pair(seg_at, lo, hi):
    """Two neighbouring doubles t (in reach) and its successor towards hi (out of reach) of a family of segments that is in at lo and
    out at hi: bisection on the rule itself."""
    assert seg_at(lo)[1] and not seg_at(hi)[1]
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if seg_at(mid)[1]:
            lo = mid
        else:
            hi = mid
    assert hi == math.nextafter(lo, hi)
    return seg_at(lo)[0], seg_at(hi)[0]


def crafted_columns(rect, yaw):
    """One soup whose segments exercise every clause of the rule against `rect` around ROOT with the given yaw.  Returns the columns,
    and what the rule must say per segment where the construction fixes it (None: whatever the written-out rule says)."""
    rx, ry = ROOT
    h = np.array([math.cos(yaw), math.sin(yaw)])  # heading and left normal: where the construction aims (the rule decides)
    l = np.array([-h[1], h[0]])
    mid_u, mid_v = 0.5 * (rect[0] + rect[1]), 0.5 * (rect[2] + rect[3])
    world = lambda u, v: (rx + u * h[0] + v * l[0], ry + u * h[1] + v * l[1])
    segs, want = [], []
    inside = list(world(mid_u, mid_v)) + list(world(mid_u + 0.01, mid_v + 0.01))
    for i in range(4):  # NaN in each of the four coordinates
        s = list(inside)
        s[i] = NAN
        segs.append(s)
        want.append(False)
    far = list(world(mid_u + 500.0, mid_v + 500.0)) + list(world(mid_u + 501.0, mid_v + 501.0))
    for i in range(4):  # +-inf in each: never culled
        for v in (INF, -INF):
            s = list(far)
            s[i] = v
            segs.append(s)
            want.append(True)
    big_in, big_out = 2.0 ** 64, 2.0 ** 65
    segs += [[big_in, ry, big_in, ry + 1.0], [big_out, ry, big_out, ry + 1.0], [rx, -big_out, rx + 1.0, -big_out], [far[0], far[1], far[2], math.nextafter(2.0 ** 64, INF)]]
    want += [None, True, True, True]  # (2^64 itself is finite for the rule: decided by the arithmetic; beyond it: in)
    # one ulp inside and outside each widened side: a short segment beyond the side, parallel to it, moved along the side's normal
    for axis, sign, bound in ((0, 1.0, rect[1]), (0, -1.0, rect[0]), (1, 1.0, rect[3]), (1, -1.0, rect[2])):
        def seg_at(t, axis=axis, sign=sign, bound=bound):
            d = bound + sign * t
            p, q = (world(d, mid_v - 0.01), world(d, mid_v + 0.01)) if axis == 0 else (world(mid_u - 0.01, d), world(mid_u + 0.01, d))
            s = [p[0], p[1], q[0], q[1]]
            return s, in_reach(s, rect, rx, ry, yaw)
        a, b = flip_pair(seg_at, 0.0, 1e-3)
        segs += [a, b]
        want += [True, False]
    segs += [inside, list(world(mid_u - 10.0, mid_v - 10.0)) + list(world(mid_u + 10.0, mid_v + 10.0)), far, list(world(rect[0] - 0.05, mid_v)) + list(world(rect[0] - 0.04, mid_v))]
    want += [True, True, False, False]  # (the last one: directly behind the root, inside the square of the disc bound)
    xs, ys = [], []
    for s in segs:  # every segment a polyline of its own: [p0, p1, NaN]
        xs += [s[0], s[2], NAN]
        ys += [s[1], s[3], NAN]
    return np.array(xs), np.array(ys), want


@pytest.mark.parametrize("yaw", YAWS)
def test_twin_matches_the_rule_on_crafted_segments(yaw):
    mpa = make_mpa(MpaType.single_speed, 8)
    trim = 1
    for Hp in (1, 3, 8):
        rects = native_rects(mpa, Hp)
        x, y, want = crafted_columns(rects[trim - 1, Hp - 1], yaw)
        every = ranges(Hp, len(x))
        got = twin(Hp, rects, trim, ROOT[0], ROOT[1], yaw, x, y, every)
        assert got == brute(Hp, rects, trim, ROOT[0], ROOT[1], yaw, x, y, every)
        last = set(twin(Hp, rects, trim, ROOT[0], ROOT[1], yaw, x, y, ranges(Hp, len(x), only=Hp))[Hp - 1])
        for i, w in enumerate(want):
            if w is not None:
                assert (3 * i in last) == w, (Hp, i, w)
        assert all(j % 3 != 1 for j in last)  # a segment into a NaN separator is never listed
    # every root trim reads its own row of the table
    rects = native_rects(mpa, 8)
    x, y, _ = crafted_columns(rects[0, 7], yaw)
    for trim in range(1, mpa.n_trims + 1):
        every = ranges(8, len(x))
        assert twin(8, rects, trim, ROOT[0], ROOT[1], yaw, x, y, every) == brute(8, rects, trim, ROOT[0], ROOT[1], yaw, x, y, every)


def test_lists_twin_arguments():
    L = backend.load_library()
    rects = np.zeros((2, 1, 4))
    x = np.zeros(2)
    first, count, lo, lst = np.zeros(1, np.int32), np.full(1, 2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    call = lambda Hp, n, trim: L.pdmpc_reach_lists_oriented_host(Hp, n, rects.ctypes.data_as(DP), trim, 0.0, 0.0, 0.0, x.ctypes.data_as(DP), x.ctypes.data_as(DP), first.ctypes.data_as(IP),
                                                                 count.ctypes.data_as(IP), lo.ctypes.data_as(IP), lst.ctypes.data_as(IP))
    assert call(1, 2, 1) == 0 and call(1, 2, 2) == 0
    assert call(1, 2, 0) != 0 and call(1, 2, 3) != 0 and call(0, 2, 1) != 0 and call(HP_MAX + 1, 2, 1) != 0
    # a table of NaN (a trim without successors) culls nothing but NaN segments
    rects[:] = NAN
    assert call(1, 2, 1) == 0 and lo[1] == 1


# ---- (c) soundness on the oracle's own searches ------------------------------------------------------------------------------
def soup(polys):
    xs, ys = [], []
    for p in polys:
        p = np.asarray(p, dtype=np.float64)
        xs += p[0].tolist() + [NAN]
        ys += p[1].tolist() + [NAN]
    return np.array(xs), np.array(ys)


def listed(x, y, lst):
    out = np.full((2, 3 * len(lst) + 1), NAN)
    for i, j in enumerate(lst):
        out[0, 3 * i:3 * i + 2] = x[j:j + 2]
        out[1, 3 * i:3 * i + 2] = y[j:j + 2]
    return out


def check_step_problem(options, mpa, prob, rects):
    """The level loop of oracle.plan_step with traces; every edge of every tree against its step's soups, whole and listed."""
    Hp = options.Hp
    recs = {}
    first = 0
    edges = crossing = walked = in_list = 0
    for size in prob["level_sizes"]:
        slots = list(range(first, first + size))
        iters = []
        for s in slots:
            it = copy.copy(prob["iters"][s])
            dyn = list(it.dynamic_obstacle_area)
            for p in prob["preds"][s]:
                if int(recs[p]["status"]) == 0:
                    dyn.append([np.array(recs[p]["shapes"][k][:, : int(recs[p]["shape_cols"][k])]) for k in range(Hp)])
                elif prob["fallback"][p] is not None and len(prob["fallback"][p]):
                    dyn.append([np.asarray(a, dtype=np.float64) for a in prob["fallback"][p]])
            it.dynamic_obstacle_area = dyn
            iters.append(it)
        _, out, traces = oracle.plan_batch(options, mpa, iters, trace=True)
        for q, s in enumerate(slots):
            recs[s] = out[q]
        for it, tr in zip(iters, traces):
            rx, ry, ryaw, rtrim = float(it.x0[0]), float(it.x0[1]), float(it.x0[2]), int(it.trim_index)
            lists = lambda x, y, only=None: twin(Hp, rects, rtrim, rx, ry, ryaw, x, y, ranges(Hp, len(x), only=only))
            left, right = it.predicted_lanelet_boundary
            bx, by = soup([b for b in (left, right) if b is not None and np.size(b)])
            bl = lists(bx, by) if len(bx) else [[]] * Hp
            vs = [soup(list(it.obstacles) + [d[k] for d in it.dynamic_obstacle_area] + [h[k] for h in it.hdv_reachable_sets]) for k in range(Hp)]
            vl = [lists(vs[k][0], vs[k][1], only=k + 1)[k] if len(vs[k][0]) else [] for k in range(Hp)]
            walked += sum(max(len(vs[k][0]) - 1, 0) + max(len(bx) - 1, 0) for k in range(Hp))
            in_list += sum(len(vl[k]) + len(bl[k]) for k in range(Hp))
            t = tr.tree
            assert float(t["yaw"][0]) == ryaw and int(t["trim"][0]) == rtrim
            sn, cs = oracle.sincos(t["yaw"])
            for i in range(len(t["x"])):
                par = int(t["parent"][i])
                if par <= 0:
                    continue
                k = int(t["k"][i])
                assert 1 <= k <= Hp
                man = mpa.maneuvers[int(t["trim"][par - 1]) - 1][int(t["trim"][i]) - 1]
                c, s_, px, py = cs[par - 1], sn[par - 1], t["x"][par - 1], t["y"][par - 1]
                move = lambda a: np.vstack([c * a[0] - s_ * a[1] + px, s_ * a[0] + c * a[1] + py])
                box = widened(rects[rtrim - 1, k - 1], rx, ry)
                for area, (x, y), lst in ((move(man.area), vs[k - 1], vl[k - 1]),
                                          (move(man.area_large_offset if k == Hp else man.area_without_offset), (bx, by), bl[k - 1])):
                    if len(x) < 2:
                        continue
                    u, v = root_frame(area[0], area[1], rx, ry, cs[0], sn[0])  # the bound the lists rest on: the area lies in its step's rectangle
                    assert u.min() >= box[0] and u.max() <= box[1] and v.min() >= box[2] and v.max() <= box[3], (i, k)
                    whole = oracle.interx(area, np.vstack([x, y]))
                    part = oracle.interx(area, listed(x, y, lst)) if lst else False
                    assert whole == part, (i, k, whole, part)
                    if whole:  # every single crossing segment is a listed one
                        crossing += 1
                        for j in range(len(x) - 1):
                            if j not in lst and not (math.isnan(x[j]) or math.isnan(x[j + 1])):
                                assert not oracle.interx(area, np.array([[x[j], x[j + 1]], [y[j], y[j + 1]]])), (i, k, j)
                    edges += 1
        first += size
    return edges, crossing, walked, in_list


@pytest.mark.parametrize("amount,Hp,steps", [(20, 8, range(21, 27)), (12, 5, range(1, 7))])
def test_lists_are_sound_on_the_oracles_searches(amount, Hp, steps):
    options = Config(scenario_type=ScenarioType.commonroad, amount=amount, Hp=Hp, mpa_type=MpaType.single_speed, max_vehicles=32, max_nodes=1 << 30)
    mpa = get_mpa(options)
    rects = native_rects(mpa, Hp)
    sc = commonroad_scenario(options, seed=1, tiles=1)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc), priority_strategy="constant")
    step = [0]
    totals = [0, 0, 0, 0]

    def plan_step(prob):
        recs, _, _ = oracle.plan_step_native(options, mpa, prob, n_threads=8)
        step[0] += 1
        if step[0] in steps:
            for q, v in enumerate(check_step_problem(options, mpa, prob, rects)):
                totals[q] += v
        return [info_from_record(recs[i], Hp) for i in range(len(recs))]

    for _ in range(max(steps)):
        ctl.step(plan_step=plan_step)
    print("edges %d, crossing %d, segments walked %d, listed %d" % tuple(totals))
    assert totals[0] > 1000 and totals[1] > 0, totals
    assert totals[3] < totals[2]
