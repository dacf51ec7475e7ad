"""Human-driven vehicles on the CPU: the host twin (csrc/hdv.cpp, include/pdmpc_hdv.h) against the Python twin
(pdmpc/hdv.py) bit for bit, and both against exact arithmetic — the closest-lanelet decisions against rational squared distances, the
reachable lanes against exact clipping of the chain polygon by the set's half-planes (tests/exact_geometry.py, with the tolerance of
the exact bounding test: it is the same rule), the adjacency against cases worked out by hand."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

import exact_geometry as X
import hdv_cases as H
from pdmpc import backend, hdv
from pdmpc import reachability as R
from pdmpc.road_network import lab_map, lanelet_relationship_types
from reachable_geometry_checks import check_bounded_set

ERRORS = X.Errors()


@pytest.fixture(scope="module")
def lab():
    return hdv.lab_hdv_map()


# ---- the relationship table


def test_relationship_table_of_the_lab_map():
    m = lab_map()
    T = lanelet_relationship_types(m)
    assert T.shape == (104, 104) and not np.tril(T).any()
    # 1 -> 3 (longitudinal), 1 and 15 both lead into 3 (merging), 3 -> 5 and 3 -> 23 (forking), 1 | 2 are not in the same direction
    assert T[0, 2] == hdv.LONGITUDINAL and T[0, 14] == hdv.MERGING and T[4, 22] == hdv.FORKING and T[2, 4] == hdv.LONGITUDINAL
    assert T[2, 63] == 0
    for i in range(104):
        for s in m.succ[i]:
            if s:
                assert T[min(i, s - 1), max(i, s - 1)] == hdv.LONGITUDINAL
    assert sorted(np.unique(T).tolist()) == [0, 1, 2, 3, 4]  # (no crossing: left out)


# ---- (a) closest lanelets


def _exact_points(hmap):
    """every centre point as exact integers on a common grid -> (scale, per lanelet object arrays x, y)"""
    D = math.lcm(1, *{Fraction(float(v)).denominator for c in hmap.centre for v in c.ravel()})
    return D, [(np.array([int(Fraction(float(v)) * D) for v in c[:, 0]], dtype=object), np.array([int(Fraction(float(v)) * D) for v in c[:, 1]], dtype=object)) for c in hmap.centre]


def test_closest_lanelets_on_every_centre_point_against_exact_arithmetic(lab):
    """1 176 points.  d_i: host twin = Python twin bit for bit.  Every `<` of the scan against the exact squared distances; every band
    decision `<= best + 0.1` against 50-digit arithmetic where |d_i - (best + 0.1)| > 1e-9 (at most 1 % may be left out)."""
    getcontext().prec = 50
    D, pts = _exact_points(lab)
    band = Decimal(hdv.CLOSEST_BAND)
    n_points = decisions = skipped = 0
    most = 0
    for c in lab.centre:
        for q in range(c.shape[0]):
            px, py = float(c[q, 0]), float(c[q, 1])
            d = hdv.lanelet_distances(lab, px, py)
            assert d.tobytes() == hdv.lanelet_distances_native(lab, px, py).tobytes()
            ipx, ipy = int(Fraction(px) * D), int(Fraction(py) * D)
            d2 = [min((x - ipx) * (x - ipx) + (y - ipy) * (y - ipy)) for x, y in pts]  # exact, times D^2
            best, best2, lst = math.inf, None, []
            for i, di in enumerate(d.tolist()):
                less = best2 is None or d2[i] < best2
                assert (di < best) == less, (px, py, i)
                if less:
                    best, best2, lst = di, d2[i], [i + 1]
                    continue
                decisions += 1
                if abs(di - (best + hdv.CLOSEST_BAND)) <= 1e-9:
                    skipped += 1
                else:
                    exact = (Decimal(d2[i]).sqrt() - Decimal(best2).sqrt()) / Decimal(D) <= band
                    assert (di <= best + hdv.CLOSEST_BAND) == exact, (px, py, i)
                if di <= best + hdv.CLOSEST_BAND:
                    lst.append(i + 1)
            assert lst == hdv.closest_scan(d)
            assert len(hdv.chains(lab, lst)) <= 8  # (PDMPC_HDV_MAX_CHAINS is 16)
            most = max(most, len(lst))
            n_points += 1
    print("points", n_points, "band decisions", decisions, "left out", skipped)
    assert n_points == 1176 and most == 8
    assert skipped <= 0.01 * decisions


def test_closest_lanelets_named_cases(lab):
    x, y, _ = H.along(lab, 3, 0)
    d = hdv.lanelet_distances(lab, x, y)
    assert hdv.closest_lanelets(lab, x, y) == [3, 15]
    # the rule is order-dependent: lanelet 1 is within 0.1 of the final minimum, but was dropped when lanelet 3 took the lead
    assert (np.flatnonzero(d <= d.min() + 0.1) + 1).tolist() == [1, 3, 15]
    x, y, _ = H.along(lab, 17, 10)
    assert hdv.closest_lanelets(lab, x, y) == [17, 20, 21, 24, 43, 46, 47, 50]
    x, y, _ = H.along(lab, 3, 3)
    assert hdv.closest_lanelets(lab, x, y) == [3] and hdv.chains(lab, [3]) == [(3, 5), (3, 23)]
    assert hdv.chains(H.hand_map(), [1, 2, 3]) == [(1, 2), (2, 0), (3, 2)]
    # ... and a tile offset is taken off the position first
    assert hdv.closest_lanelets(lab, x + 12.0, y - 24.0, 12.0, -24.0) == [3]


def test_more_chains_than_the_limit_is_a_capacity_error(lab):
    """17 lanelets on one spot: 17 closest lanelets, one chain each"""
    sq = [(0.0, 0.5), (1.0, 0.5)], [(0.0, -0.5), (1.0, -0.5)]
    many = hdv.HdvMap([sq[0]] * 17, [sq[1]] * 17, [[]] * 17, np.zeros((17, 17), dtype=np.uint8))
    args = ([0.5], [0.0], [0.0], [1], [(0.0, 0.0)], [], [], [], [])
    with pytest.raises(backend.BackendError) as e:
        hdv.hdv_traffic_native(many, H.local_sets(1), *args)
    assert e.value.status == backend.ERR_CAPACITY
    with pytest.raises(OverflowError):
        hdv.hdv_traffic(many, H.local_sets(1), *args)
    fewer = hdv.HdvMap([sq[0]] * 16, [sq[1]] * 16, [[]] * 16, np.zeros((16, 16), dtype=np.uint8))
    assert len(hdv.hdv_traffic_native(fewer, H.local_sets(1), *args)["row_hdv"]) == 16


def test_invalid_arguments_of_the_host_twin(lab):
    sets = H.local_sets(1)
    ok = ([0.5], [0.0], [0.0], [1], [(0.0, 0.0)], [0.5], [0.0], [1], [(0.0, 0.0)])
    hm = H.hand_map()
    assert hdv.hdv_traffic_native(hm, sets, *ok)["closest"] == [[1]]
    for bad in (([0.5], [0.0], [0.0], [0], [(0.0, 0.0)], [], [], [], []), ([0.5], [0.0], [0.0], [len(sets) + 1], [(0.0, 0.0)], [], [], [], []),
                ([0.5], [0.0], [0.0], [1], [(0.0, 0.0)], [0.5], [0.0], [4], [(0.0, 0.0)]), ([0.5], [0.0], [0.0], [1], [(0.0, 0.0)], [0.5], [0.0], [0], [(0.0, 0.0)])):
        with pytest.raises(backend.BackendError) as e:
            hdv.hdv_traffic_native(hm, sets, *bad)
        assert e.value.status == -1  # PDMPC_ERR_INVALID
    with pytest.raises(backend.BackendError) as e:  # more HDVs than PDMPC_HDV_MAX_VEHICLES
        hdv.hdv_traffic_native(hm, sets, [0.5] * 65, [0.0] * 65, [0.0] * 65, [1] * 65, [(0.0, 0.0)] * 65, [], [], [], [])
    assert e.value.status == backend.ERR_CAPACITY
    with pytest.raises(backend.BackendError) as e:  # Hp beyond PDMPC_HP_MAX, as at the upload
        hdv.hdv_traffic_native(hm, H.ngon_sets(4, 17), *ok)
    assert e.value.status == -1
    broken = H.hand_map()
    broken.successors[0] = [4]
    with pytest.raises(backend.BackendError) as e:
        hdv.hdv_traffic_native(broken, sets, *ok)
    assert e.value.status == -1


# ---- (c) the reachable lane


def _lane_cases(lab):
    """(name, map, sets, HDV, the flags that must occur)"""
    wide = H.hand_map(width=4.0)
    x, y, yaw = H.along(lab, 64, 3)
    return [
        ("K inside L", wide, H.local_sets(1), (1.0, 0.0, 0.0), {0}),
        ("K across one boundary", wide, H.local_sets(1), (1.0, 1.9, 0.0), {0}),
        ("K across both boundaries", lab, H.local_sets(6), (x, y, yaw), {0}),
        ("K and L apart", lab, H.local_sets(6), (x - math.sin(yaw), y + math.cos(yaw), yaw), {0, R.BOUND_RESTORED}),
        ("two regions", H.u_map(), H.ngon_sets(12, 1, radius=1.0), (0.5, 0.0, 0.0), {R.BOUND_MULTIPLE}),
    ]


def _check_lane(name, what, r, flag, K, Ln):
    """One reachable lane r against area(K ∩ L) from exact clipping of L by K's half-planes (X.area_convex_simple: the shoelace sum of
    the clipped polygon, which is also defined where the map's chain polygon is not strictly simple — the lab map's lanelets do not
    meet their successors bit for bit), with the tolerance of the exact bounding test.  Returns the error."""
    full = X.area_convex_simple(K, Ln)
    tol = X.tolerance(full, X.area(K), X.area(Ln))
    if flag & R.BOUND_RESTORED:  # empty: a polygon of 0 columns, and the exact intersection has no area
        assert flag == R.BOUND_RESTORED and r.shape == (2, 0), (name, what)
        assert full <= tol, (name, what, float(full))
        return float(full)
    assert r.shape[1] >= 4 and r[0, 0] == r[0, -1] and r[1, 0] == r[1, -1], (name, what, "not closed")
    ar = X.area(X.poly(r))
    if flag == R.BOUND_MULTIPLE:
        assert 0 < ar < full - Fraction(tol), (name, what, float(ar), float(full))
        return 0.0
    assert flag == 0, (name, what, flag)
    assert abs(ar - full) <= tol, (name, what, float(ar), float(full), tol)
    return float(abs(ar - full))


def test_reachable_lanes_against_exact_clipping(lab):
    for name, hmap, sets, (x, y, yaw), want_flags in _lane_cases(lab):
        args = ([x], [y], [yaw], [1], [(0.0, 0.0)], [], [], [], [])
        py, host = hdv.hdv_traffic(hmap, sets, *args), hdv.hdv_traffic_native(hmap, sets, *args)
        H.assert_same(py, host, name)
        seen, worst = set(), 0.0
        lst = py["closest"][0]
        for row, (lanelet, successor) in enumerate(hdv.chains(hmap, lst)):
            Ln = X.normalized(X.poly(hdv.chain_polygon(hmap, lanelet, successor)))
            simple = X.is_simple(Ln)
            for k, K_closed in enumerate(R.reachable_sets_at_pose(sets, x, y, yaw, 1)):
                K = X.poly(K_closed)
                r, f = py["sets"][row][k], int(py["flags"][row, k])
                seen.add(f)
                worst = max(worst, _check_lane(name, (row, k), r, f, K, Ln))
                if f != R.BOUND_RESTORED and simple:  # ... and everything the exact bounding test asks of a bounded set
                    check_bounded_set(ERRORS, "reachable lane, " + name, ("python", "host"), r, f, K, Ln, False, (row, k), thorough=False)
        print(name, "worst area error", worst)
        assert seen == want_flags, (name, seen)
        if name == "K inside L":
            K = R.reachable_sets_at_pose(sets, x, y, yaw, 1)[0]
            assert py["sets"][0][0].tobytes() == np.ascontiguousarray(K).tobytes()  # K itself, closed
        if name == "K and L apart":
            assert all(py["sets"][r][0].shape[1] == 0 for r in range(len(py["sets"]))) and any(s.shape[1] > 0 for s in py["sets"][0])
    for line in ERRORS.lines():
        print(line)


def test_the_twins_agree_on_the_device_cases():
    """the cases tests/test_gpu_hdv.py runs on the device: Python twin = host twin, and the capacity protocol of the host twin"""
    for case in H.traffic_cases():
        py, host = case.python(), case.host()
        H.assert_same(py, host, case.name)
        total = int(host["set_offset"][-1])
        assert total == sum(s.shape[1] for row in py["sets"] for s in row)
        if total:
            with pytest.raises(backend.CapacityError) as e:
                case.host(capacity=total - 1)
            assert e.value.count == total
        H.assert_same(case.host(capacity=total), host, case.name)
    names = " ".join(c.name for c in H.traffic_cases())
    assert "Hp 1" in names and "256" in names and "tile" in names


def test_the_layout_is_what_a_search_receives(lab):
    """rows of the adjacent HDVs in row order, polygon row * Hp + k (pdmpc_vehicle_in.hdv_reachable_sets)"""
    case = H.traffic_cases()[2]
    r = case.host()
    assert r["row_hdv"] == sorted(r["row_hdv"]) and len(r["sets"]) == len(r["row_hdv"]) == 11 and all(len(row) == 6 for row in r["sets"])
    for v in range(len(case.cavs)):
        rows = hdv.cav_rows(r, v)
        assert len(rows) == sum(1 for h in r["row_hdv"] if r["adjacency"][v, h])


# ---- (d) adjacency


def _adjacent(hmap, hdv_pose, cav, hdv_tile=(0.0, 0.0), cav_tile=(0.0, 0.0)):
    """the adjacency bit of one CAV (x, y, lanelet) and one HDV (x, y, yaw): both twins, which must agree"""
    args = ([hdv_pose[0]], [hdv_pose[1]], [hdv_pose[2]], [1], [hdv_tile], [cav[0]], [cav[1]], [cav[2]], [cav_tile])
    a = hdv.hdv_traffic(hmap, H.local_sets(1), *args)["adjacency"]
    b = hdv.hdv_traffic_native(hmap, H.local_sets(1), *args)["adjacency"]
    assert a.shape == (1, 1) and np.array_equal(a, b)
    return int(a[0, 0])


def test_adjacency_on_the_hand_made_graph():
    hm = H.hand_map()
    merge_yaw = math.atan2(0.5, 1.0)
    assert _adjacent(hm, (0.5, 0.0, 0.0), (1.5, 0.0, 1)) == 0  # behind on the same lanelet
    assert _adjacent(hm, (1.5, 0.0, 0.0), (0.5, 0.0, 1)) == 1  # ahead on it
    assert _adjacent(hm, (0.5, 0.0, 0.0), (3.0, 0.0, 2)) == 0  # on the predecessor lanelet
    assert _adjacent(hm, (3.5, 0.0, 0.0), (0.5, 0.0, 1)) == 1  # on the successor lanelet: longitudinal, but the ends do not meet
    assert _adjacent(hm, (1.0, -0.5, merge_yaw), (1.8, 0.0, 1)) == 0  # on the merging lanelet, behind along its own heading
    assert _adjacent(hm, (1.0, -0.5, merge_yaw), (0.0, 0.0, 1)) == 1  # on the merging lanelet, ahead
    assert _adjacent(hm, (1.0, -0.5, merge_yaw), (3.0, 0.0, 2)) == 0  # the merging lanelet is a predecessor of lanelet 2
    unrelated = H.hand_map(related=False)
    assert _adjacent(unrelated, (1.0, -0.5, merge_yaw), (1.8, 0.0, 1)) == 1  # no relationship: adjacent (the dropped assert)
    assert _adjacent(unrelated, (0.5, 0.0, 0.0), (3.0, 0.0, 2)) == 1
    assert _adjacent(unrelated, (0.5, 0.0, 0.0), (1.5, 0.0, 1)) == 0  # (the same lanelet needs no table)
    assert _adjacent(hm, (1.5 + 12.0, 0.0, 0.0), (0.5, 0.0, 1), hdv_tile=(12.0, 0.0)) == 0  # another copy of the map
    assert _adjacent(hm, (1.5 + 12.0, 0.0, 0.0), (0.5 + 12.0, 0.0, 1), hdv_tile=(12.0, 0.0), cav_tile=(12.0, 0.0)) == 1


def test_adjacency_with_the_table_of_the_lab_map(lab):
    on = lambda lanelet, q: H.along(lab, lanelet, q)  # noqa: E731
    cav = lambda lanelet, q: H.along(lab, lanelet, q)[:2] + (lanelet,)  # noqa: E731
    assert hdv.closest_lanelets(lab, *on(3, 3)[:2]) == [3] and hdv.closest_lanelets(lab, *on(64, 3)[:2]) == [64]
    assert _adjacent(lab, on(3, 2), cav(3, 4)) == 0  # behind on the same lanelet
    assert _adjacent(lab, on(3, 4), cav(3, 2)) == 1  # ahead
    assert 3 in lab.successors[0] and _adjacent(lab, on(1, 5), cav(3, 4)) == 0  # lanelet 1 leads into 3: on the predecessor lanelet
    assert _adjacent(lab, on(3, 3), cav(1, 5)) == 1  # ... and seen from lanelet 1, an HDV on 3 is ahead
    # 1 and 15 merge into 3: an HDV on 15 is judged along its own heading
    assert hdv.closest_lanelets(lab, *on(15, 5)[:2]) == [15] and lab.relationship[0, 14] == hdv.MERGING
    x, y, yaw = on(15, 5)
    assert _adjacent(lab, (x, y, yaw), (x + math.cos(yaw), y + math.sin(yaw), 1)) == 0  # the CAV 1 m further along that heading
    assert _adjacent(lab, (x, y, yaw), (x - math.cos(yaw), y - math.sin(yaw), 1)) == 1
    assert lab.relationship[2, 63] == 0 and _adjacent(lab, on(64, 3), cav(3, 3)) == 1  # unrelated lanelets
    assert _adjacent(lab, on(3, 4), cav(3, 2), hdv_tile=(0.0, 12.0)) == 0  # different tile
