"""The reach lists of the graph search (include/pdmpc_reach.h) on the host, no GPU: the host twin
pdmpc_reach_lists_host against the rule written out in Python on crafted soups, the automaton's reach against pdmpc.mpa, and the
soundness condition on the oracle's own searches: for every edge the oracle evaluated, InterX over all segments of its step and over
the listed ones agree, and every crossing segment is listed."""
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


# ---- the rule, written out (pdmpc_reach.h says the same in C) ---------------------------------------------------------------
def radius(dmax, amax, k):
    r = np.float64(k - 1) * np.float64(dmax) + np.float64(amax)
    return float(r + r * np.float64(2.0 ** -50))


def box(dmax, amax, k, rx, ry):
    R = np.float64(radius(dmax, amax, k))
    rho = R + np.float64(2.0 ** -20) * (np.float64(1.0) + abs(np.float64(rx)) + abs(np.float64(ry)) + R)
    return float(rx - rho), float(rx + rho), float(ry - rho), float(ry + rho)


def in_reach(seg, b):
    x0, y0, x1, y1 = seg
    if any(math.isnan(c) for c in seg):
        return False
    if not all(abs(c) <= 2.0 ** 64 for c in seg):
        return True
    x_lo, x_hi, y_lo, y_hi = b
    return not (max(x0, x1) < x_lo or min(x0, x1) > x_hi or max(y0, y1) < y_lo or min(y0, y1) > y_hi)


def ranges(Hp, n, only=None):
    """(first, count) per step: all n columns for every step (the lanelet boundary), or for step `only` alone (1-based)."""
    count = np.array([n if only in (None, k) else 0 for k in range(1, Hp + 1)], dtype=np.int32)
    return np.zeros(Hp, dtype=np.int32), count


def brute(Hp, dmax, amax, rx, ry, x, y, rng):
    out = []
    for k in range(1, Hp + 1):
        b = box(dmax, amax, k, rx, ry)
        a, c = int(rng[0][k - 1]), int(rng[1][k - 1])
        out.append([j for j in range(max(c - 1, 0)) if in_reach((x[a + j], y[a + j], x[a + j + 1], y[a + j + 1]), b)])
    return out


def twin(Hp, dmax, amax, rx, ry, x, y, rng):
    L = backend.load_library()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    first, count = (np.ascontiguousarray(a, dtype=np.int32) for a in rng)
    lo = np.zeros(Hp + 1, dtype=np.int32)
    lst = np.full(max(int(count.sum()), 1), -1, dtype=np.int32)
    rc = L.pdmpc_reach_lists_host(Hp, dmax, amax, rx, ry, x.ctypes.data_as(DP), y.ctypes.data_as(DP), first.ctypes.data_as(IP), count.ctypes.data_as(IP), lo.ctypes.data_as(IP),
                                  lst.ctypes.data_as(IP))
    assert rc == 0
    return [lst[lo[k]:lo[k + 1]].tolist() for k in range(Hp)]


DMAX, AMAX = 0.16, 0.324
ROOT = (2.25, -1.5)


def ulp_steps(v, n):
    for _ in range(abs(n)):
        v = math.nextafter(v, INF if n > 0 else -INF)
    return v


def crafted_columns():
    """One soup whose segments exercise every clause of the rule against the square of step 3 around ROOT."""
    x_lo, x_hi, y_lo, y_hi = box(DMAX, AMAX, 3, *ROOT)
    cx, cy = ROOT
    segs = []
    for i in range(4):  # NaN in each of the four coordinates
        s = [cx, cy, cx + 0.1, cy + 0.1]
        s[i] = NAN
        segs.append(s)
    for i in range(4):  # +-inf in each: never culled
        for v in (INF, -INF):
            s = [cx + 50.0, cy + 50.0, cx + 51.0, cy + 51.0]
            s[i] = v
            segs.append(s)
    big_in, big_out = 2.0 ** 64, math.nextafter(2.0 ** 64, INF)
    segs += [[big_in, cy, big_in, cy + 1.0], [big_out, cy, big_out, cy + 1.0], [-big_in, cy, -big_in, cy], [-big_out, cy, -big_out, cy],
             [cx, math.nextafter(2.0 ** 64, 0.0), cx + 100.0, 2.0 ** 64], [cx + 100.0, big_out, cx + 101.0, big_out]]
    for d in (-1, 0, 1):  # a box touching the square from each side: one ulp inside, on it, one ulp outside
        segs.append([ulp_steps(x_lo, -d) - 1.0, cy, ulp_steps(x_lo, -d), cy])        # from the left: max x against x_lo
        segs.append([ulp_steps(x_hi, d), cy, ulp_steps(x_hi, d) + 1.0, cy])          # from the right
        segs.append([cx, ulp_steps(y_lo, -d) - 1.0, cx, ulp_steps(y_lo, -d)])        # from below
        segs.append([cx, ulp_steps(y_hi, d), cx, ulp_steps(y_hi, d) + 1.0])          # from above
    segs += [[cx - 10.0, cy - 10.0, cx + 10.0, cy + 10.0], [cx, cy, cx, cy], [cx + 5.0, cy, cx + 6.0, cy], [x_hi + 1.0, y_hi + 1.0, x_hi + 2.0, y_lo - 5.0]]
    xs, ys = [], []
    for s in segs:  # every segment a polyline of its own: [p0, p1, NaN]
        xs += [s[0], s[2], NAN]
        ys += [s[1], s[3], NAN]
    return np.array(xs), np.array(ys), len(segs)


def test_twin_matches_the_rule_on_crafted_segments():
    x, y, n = crafted_columns()
    for Hp in (1, 2, 3, HP_MAX):
        every = ranges(Hp, len(x))  # (every step sees the whole soup, as with the lanelet boundary)
        got = twin(Hp, DMAX, AMAX, ROOT[0], ROOT[1], x, y, every)
        assert got == brute(Hp, DMAX, AMAX, ROOT[0], ROOT[1], x, y, every)
        assert all(set(a) <= set(b) for a, b in zip(got, got[1:]))
    # step 3 of Hp 3, clause by clause: segment i is columns 3 i, 3 i + 1
    lst = set(twin(3, DMAX, AMAX, ROOT[0], ROOT[1], x, y, ranges(3, len(x), only=3))[2])
    seg = lambda i: 3 * i in lst
    assert not any(seg(i) for i in range(4))                      # NaN: out
    assert all(seg(i) for i in range(4, 12))                      # infinities: in
    assert [seg(i) for i in range(12, 18)] == [False, True, False, True, False, True]  # |c| <= 2^64 far away: out; beyond: in
    touch = [seg(i) for i in range(18, 30)]
    assert touch == [True] * 8 + [False] * 4                      # one ulp inside and exactly on the square: in; one ulp outside: out
    assert [seg(i) for i in range(30, 34)] == [True, True, False, False]
    assert all(j % 3 != 1 for j in lst)                           # a segment into a NaN separator is never listed
    assert n == 34


def test_empty_steps_and_trip_boundaries():
    cx, cy = ROOT
    for n_in in (0, 1, 63, 64, 65, 130):
        # a polyline of n_in segments inside the square, then as many far outside it (one joining segment crosses the square's edge: in)
        xs = [cx + 1e-3 * i for i in range(n_in + 1)] + [cx + 100.0 + i for i in range(n_in + 1)]
        ys = [cy] * len(xs)
        if n_in == 0:
            xs, ys = [cx + 100.0, cx + 101.0], [cy, cy]
        Hp = 2
        so = ranges(Hp, len(xs), only=2)  # step 1 is empty
        got = twin(Hp, DMAX, AMAX, cx, cy, xs, ys, so)
        assert got == brute(Hp, DMAX, AMAX, cx, cy, xs, ys, so)
        assert got[0] == []
        assert len(got[1]) == (0 if n_in == 0 else n_in + 1) and got[1] == sorted(got[1])
    # no columns at all, and a single column (no segment)
    assert twin(1, DMAX, AMAX, 0.0, 0.0, [0.0], [0.0], ranges(1, 0)) == [[]]
    assert twin(1, DMAX, AMAX, 0.0, 0.0, [0.0], [0.0], ranges(1, 1)) == [[]]


def test_reach_grows_with_the_step():
    xs = np.linspace(ROOT[0], ROOT[0] + 3.0, 400)
    ys = np.full_like(xs, ROOT[1])
    Hp = HP_MAX
    lists = twin(Hp, DMAX, AMAX, ROOT[0], ROOT[1], xs, ys, ranges(Hp, len(xs)))
    for a, b in zip(lists, lists[1:]):
        assert set(a) < set(b)
    for k, l in enumerate(lists, start=1):
        want = [j for j in range(len(xs) - 1) if xs[j] <= box(DMAX, AMAX, k, *ROOT)[1]]
        assert l == want


# ---- the automaton's reach -------------------------------------------------------------------------------------------------
def python_reach(mpa):
    dmax = amax = 0.0
    for row in mpa.maneuvers:
        for m in row:
            if m is None:
                continue
            dmax = max(dmax, math.hypot(m.dx, m.dy))
            for a in (m.area, m.area_without_offset, m.area_large_offset):
                amax = max(amax, max(math.hypot(float(a[0, v]), float(a[1, v])) for v in range(a.shape[1])))
    return dmax, amax


def native_reach(mpa):
    s, keep = abi.pack_mpa(mpa)
    d, a = C.c_double(-1.0), C.c_double(-1.0)
    rc = backend.load_library().pdmpc_mpa_reach_host(C.byref(s), C.byref(d), C.byref(a))
    assert rc == 0
    del keep
    return d.value, a.value


@pytest.mark.parametrize("mpa_type", [MpaType.single_speed, MpaType.triple_speed, MpaType.realistic])
def test_automaton_reach(mpa_type):
    options = Config(scenario_type=ScenarioType.commonroad, amount=2, Hp=6, mpa_type=mpa_type, max_vehicles=4, max_nodes=1 << 12)
    mpa = get_mpa(options)
    assert native_reach(mpa) == python_reach(mpa)
    if mpa_type == MpaType.single_speed:
        d, a = native_reach(mpa)
        assert abs(d - 0.16) < 5e-3 and abs(a - 0.324) < 5e-3


def test_automaton_reach_counts_used_columns_only():
    """Columns beyond n_cols of an area are padding (whatever they hold): an 8-column area counts all eight, a 5-column one five."""
    options = Config(scenario_type=ScenarioType.commonroad, amount=2, Hp=6, mpa_type=MpaType.single_speed, max_vehicles=4, max_nodes=1 << 12)
    mpa = get_mpa(options)
    s, keep = abi.pack_mpa(mpa)
    d0, a0 = native_reach(mpa)
    m = s.maneuvers[0]
    n_cols = m.n_cols
    assert n_cols < abi.VMAX
    m.area[0][abi.VMAX - 1] = 1000.0  # padding: not counted
    d, a = C.c_double(), C.c_double()
    L = backend.load_library()
    assert L.pdmpc_mpa_reach_host(C.byref(s), C.byref(d), C.byref(a)) == 0 and (d.value, a.value) == (d0, a0)
    m.n_cols = abi.VMAX  # an 8-column area: counted
    assert L.pdmpc_mpa_reach_host(C.byref(s), C.byref(d), C.byref(a)) == 0 and a.value == math.hypot(1000.0, m.area[1][abi.VMAX - 1])
    m.n_cols = n_cols
    m.area[0][abi.VMAX - 1] = 0.0
    del keep


# ---- soundness on the oracle's own searches --------------------------------------------------------------------------------
def soup(polys):
    """[polygon, NaN] ... as two coordinate arrays."""
    xs, ys = [], []
    for p in polys:
        p = np.asarray(p, dtype=np.float64)
        xs += p[0].tolist() + [NAN]
        ys += p[1].tolist() + [NAN]
    return np.array(xs), np.array(ys)


def listed(x, y, lst):
    """The listed segments as a soup of their own: [q0, q1, NaN] ..."""
    out = np.full((2, 3 * len(lst) + 1), NAN)
    for i, j in enumerate(lst):
        out[0, 3 * i:3 * i + 2] = x[j:j + 2]
        out[1, 3 * i:3 * i + 2] = y[j:j + 2]
    return out


def check_step_problem(options, mpa, prob, dmax, amax):
    """The level loop of oracle.plan_step with traces; every edge of every tree against its step's soups, whole and listed."""
    Hp = options.Hp
    recs = {}
    first = 0
    edges = crossing = 0
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
            rx, ry = float(it.x0[0]), float(it.x0[1])
            left, right = it.predicted_lanelet_boundary
            bx, by = soup([b for b in (left, right) if b is not None and np.size(b)])
            bl = twin(Hp, dmax, amax, rx, ry, bx, by, ranges(Hp, len(bx))) if len(bx) else [[]] * Hp
            vs = [soup(list(it.obstacles) + [d[k] for d in it.dynamic_obstacle_area] + [h[k] for h in it.hdv_reachable_sets]) for k in range(Hp)]
            vl = [[] for _ in range(Hp)]
            for k in range(Hp):
                vl[k] = twin(Hp, dmax, amax, rx, ry, vs[k][0], vs[k][1], ranges(Hp, len(vs[k][0]), only=k + 1))[k] if len(vs[k][0]) else []
            t = tr.tree
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
                for area, (x, y), lst in ((move(man.area), vs[k - 1], vl[k - 1]),
                                          (move(man.area_large_offset if k == Hp else man.area_without_offset), (bx, by), bl[k - 1])):
                    if len(x) < 2:
                        continue
                    assert np.max(np.hypot(area[0] - rx, area[1] - ry)) <= radius(dmax, amax, k) + 1e-9  # the bound the lists rest on
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
    return edges, crossing


@pytest.mark.parametrize("amount,Hp,steps", [(20, 8, range(21, 27)), (12, 5, range(1, 7))])
def test_lists_are_sound_on_the_oracles_searches(amount, Hp, steps):
    options = Config(scenario_type=ScenarioType.commonroad, amount=amount, Hp=Hp, mpa_type=MpaType.single_speed, max_vehicles=32, max_nodes=1 << 30)
    mpa = get_mpa(options)
    dmax, amax = native_reach(mpa)
    sc = commonroad_scenario(options, seed=1, tiles=1)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc), priority_strategy="constant")
    step = [0]
    totals = [0, 0]

    def plan_step(prob):
        recs, _, _ = oracle.plan_step_native(options, mpa, prob, n_threads=8)
        step[0] += 1
        if step[0] in steps:
            e, c = check_step_problem(options, mpa, prob, dmax, amax)
            totals[0] += e
            totals[1] += c
        return [info_from_record(recs[i], Hp) for i in range(len(recs))]

    for _ in range(max(steps)):
        ctl.step(plan_step=plan_step)
    assert totals[0] > 1000 and totals[1] > 0, totals
