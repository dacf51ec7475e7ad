"""The reachable-set kernels on the MI355X at the sizes the ABI declares, against exact arithmetic.

In the closed loop the kernels of csrc/reachable_kernel.hip and csrc/bounded_kernel.hip see hulls of at most 146 vertices, lanelet
polygons of 50 to 72 and bounded sets of about 90; the limits are 256 (PDMPC_REACHABLE_MAX_COLS), 512 (PDMPC_LANELET_POLY_MAX_COLS)
and 1024 (PDMPC_BOUNDED_MAX_COLS).  Here a handle with Hp 2 is given tables of its own — polygons of 3 to 256 vertices, step-1 and
step-2 hulls of different sizes, so that a wrong trim * Hp + q shows — and lanelet polygons of up to 512 vertices (bands and gears,
tests/exact_geometry.py).  Every case asserts the device's bits against the host twin's and the device's answers against the exact
reference by the rules of tests/test_exact_reachable_geometry.py; where a batch is too large for exact arithmetic, every entry
meets the host twin and a seeded sample the reference.  With yaw 0 and offsets that are multiples of 2^-4 the device's K is the
table's hull moved exactly; at any other yaw K is taken in doubles from reachability.reachable_sets_at_pose.

Every launch is an ordinary one: sizes stay inside what the ABI accepts or are refused by the host before a launch.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_geometry as X
from pdmpc import reachability as R
from pdmpc.backend import BackendError, Handle, bound_reachable_sets_call, fca_pairs, polygon_set_coupling_call, reachable_set_coupling_call
from pdmpc.config import Config, ScenarioType

from reachable_geometry_checks import Decisions, Pinches, chains_case, check_bounded_set, count_chains, gear_case, write_report

pytestmark = pytest.mark.gpu

SIZES = [3, 8, 12, 63, 64, 65, 128, 255, 256]  # vertices of trim t's step-2 hull; 255: the 256-gon without its vertex 7
STEP1 = [12, 3, 8, 65, 63, 64, 256, 128, 255]  # ... and of its step-1 hull (radius 0.5)
PAIR_BLOCKS = 2048  # PDMPC_BOUND_PAIR_BLOCKS (csrc/pdmpc_device.h)
ERRORS = X.Errors()  # this module's record (the device's rows of profiles/exact_geometry_errors.txt)
PINCHES = Pinches()  # none of this module's cases is pinched: every bounded set is held to strict simplicity (asserted at the end)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _hull(m, radius):
    if m == 255:
        P = X.ngon(256, radius)
        P = P[:7] + P[8:]
        assert X.is_convex_clockwise(P)
        return P
    return X.ngon(m, radius)


def _table(sizes=SIZES, step1=STEP1, radius=None):
    """[trim][step] hulls as exact polygons; step 2 (the coupled one) of radius 1 unless `radius` gives one per trim"""
    return [[_hull(step1[t], 0.5), _hull(m, 1.0 if radius is None else radius[t])] for t, m in enumerate(sizes)]


def _arrays(table):
    return [[X.arr(P) for P in row] for row in table]


def _shift(P, dx, dy):
    return [(p[0] + Fraction(dx), p[1] + Fraction(dy)) for p in P]


def _sets_at(table, arrays, x, y, yaw, trim):
    """every vehicle's exact K per step: the table's hull moved exactly (yaw 0), else the doubles of reachable_sets_at_pose"""
    out = []
    for v in range(len(x)):
        if yaw[v] == 0.0:
            out.append([_shift(P, x[v], y[v]) for P in table[trim[v] - 1]])
        else:
            out.append([X.poly(s) for s in R.reachable_sets_at_pose(arrays, x[v], y[v], yaw[v], int(trim[v]))])
    return out


def _lattice(rng, n, span):
    """n offsets in [-span, span], multiples of 2^-4"""
    return rng.integers(-int(span * 16), int(span * 16) + 1, n) / 16.0


@pytest.fixture(scope="module")
def handle():
    h = Handle(Config(scenario_type=ScenarioType.commonroad, Hp=2, max_vehicles=512, max_nodes=1 << 12))
    yield h
    h.close()


def _passing_pairs(sets):
    """the pairs i < j whose boxes overlap (boxes that only touch do not), from the exact sets"""
    a = [X.arr(P) for P in sets]
    x0, x1 = np.array([p[0].min() for p in a]), np.array([p[0].max() for p in a])
    y0, y1 = np.array([p[1].min() for p in a]), np.array([p[1].max() for p in a])
    ok = ~((x0[:, None] >= x1[None, :]) | (y0[:, None] >= y1[None, :]) | (x1[:, None] <= x0[None, :]) | (y1[:, None] <= y0[None, :]))
    i, j = np.nonzero(np.triu(ok, 1))
    return list(zip(i.tolist(), j.tolist()))


def _check_pairs(family, sets, pairs, adj, area, exact_area):
    """the device's area and coupling bit of the listed pairs (i, j) against the exact reference"""
    dec = Decisions()
    for i, j in pairs:
        ref = exact_area(i, j)
        tol = X.check_area(ERRORS, family, "device", area[i, j], ref, sets[i], sets[j], False, (i, j))
        assert area[j, i] == area[i, j] and adj[j, i] == adj[i, j]
        dec.check(adj[i, j], ref, tol, (family, i, j))
    dec.assert_share()
    return dec.n


# ---- pdmpc_reach_pose_kernel / pdmpc_reach_pairs_kernel


def test_coupler_on_every_pair_of_hull_sizes(handle):
    sizes = [3, 63, 64, 65, 128, 255, 256]
    table = _table()
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    rng = np.random.default_rng(21)
    trim = np.array([SIZES.index(m) + 1 for m in sizes] * 2)
    n = len(trim)
    x, y, yaw = _lattice(rng, n, 0.75), _lattice(rng, n, 0.75), np.zeros(n)
    adj_d, area_d = handle.reachable_set_coupling(x, y, yaw, trim)
    adj_h, area_h = reachable_set_coupling_call(arrays, x, y, yaw, trim)
    assert np.array_equal(adj_d, adj_h) and np.array_equal(_bits(area_d), _bits(area_h))
    K = [s[-1] for s in _sets_at(table, arrays, x, y, yaw, trim)]
    seen = {(len(K[i]), len(K[j])) for i in range(n) for j in range(i + 1, n)}
    assert all((a, b) in seen for a in sizes for b in sizes), "not every combination of (i, j)"
    pairs = _passing_pairs(K)
    assert len(pairs) == n * (n - 1) // 2
    checked = _check_pairs("device convex, every size pair", K, pairs, adj_d, area_d, lambda i, j: X.area_convex_simple(K[i], K[j]))
    assert checked == 91 and adj_d.sum() > 0


@pytest.mark.parametrize("n", [2, 64, 65, 512])
def test_coupler_on_dense_batches(handle, n):
    """one dense cluster (every lane of a ballot is a candidate: all boxes overlap), identical poses, nested sets, boxes that touch
    exactly, and a tail of vehicles far apart"""
    sizes = [3, 4, 7, 12, 20, 33, 65]
    radius = [0.6 + 0.1 * t for t in range(len(sizes))]
    table = _table(sizes, sizes[::-1], radius)
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    rng = np.random.default_rng(n)
    dense = n if n < 128 else n - 64
    x, y = _lattice(rng, n, 0.25), _lattice(rng, n, 0.25)
    yaw = np.where(rng.integers(2, size=n) == 1, rng.uniform(-math.pi, math.pi, n), 0.0)
    trim = rng.integers(1, len(sizes) + 1, n)
    x[dense:] = 100.0 + 10.0 * np.arange(n - dense)  # far apart: fail the box test
    if n >= 64:
        x[1], y[1], yaw[1], trim[1] = x[0], y[0], yaw[0], trim[0]  # identical
        x[3], y[3], yaw[3], yaw[2], trim[3], trim[2] = x[2], y[2], 0.0, 0.0, 1, 7  # nested: radius 0.6 in radius 1.2
        box = X.arr(table[6][1])
        x[4], y[4], yaw[4], trim[4] = x[2] + (box[0].max() - box[0].min()), y[2], 0.0, 7  # boxes touch exactly
    adj_d, area_d = handle.reachable_set_coupling(x, y, yaw, trim)
    adj_h, area_h = reachable_set_coupling_call(arrays, x, y, yaw, trim)
    assert np.array_equal(adj_d, adj_h) and np.array_equal(_bits(area_d), _bits(area_h)), n
    assert not adj_d.diagonal().any() and not area_d.diagonal().any()
    K = [s[-1] for s in _sets_at(table, arrays, x, y, yaw, trim)]
    passing = _passing_pairs(K)
    if n >= 64:
        first = set(passing)
        assert all((i, j) in first for i in range(64) for j in range(i + 1, 64) if 4 not in (i, j)), "not every lane of the first ballot is a candidate"
        assert (2, 4) not in first and adj_d[2, 4] == 0 and area_d[2, 4] == 0.0
        assert adj_d[0, 1] == 1 and abs(Fraction(float(area_d[0, 1])) - X.area(K[0])) <= 1e-9 * X.area(K[0])
        assert abs(Fraction(float(area_d[2, 3])) - X.area(K[3])) <= 1e-9 * X.area(K[3])  # nested: the inner set's area
    if n > dense:
        assert not adj_d[dense:, :].any() and not area_d[dense:, :].any()
    assert len(passing) >= (1 if n == 2 else 1500)
    pick = [passing[k] for k in rng.choice(len(passing), min(500, len(passing)), replace=False)]
    checked = _check_pairs("device convex, dense batches", K, pick, adj_d, area_d, lambda i, j: X.area_convex_simple(K[i], K[j]))
    assert checked == min(500, len(passing)), "a seeded sample of %d box-passing pairs of %d" % (checked, len(passing))


def test_coupler_on_hulls_with_the_same_heading_one_behind_the_other(handle):
    """Pairs of vehicles with the same trim and heading (yaw != 0), the second displaced along an edge of the first one's hull: two hull
    edges collinear up to the rounding of cos, sin and the offsets, the orientation determinants of the kernel's clipping at +-1e-17
    (pdmpc_orient; before it, about one such pair in sixteen missed the tolerance on the host twin)."""
    sizes = [12, 20, 33, 65, 128, 256]
    table = _table(sizes, sizes[::-1])
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    rng = np.random.default_rng(61)
    pairs_n = 120
    n = 2 * pairs_n
    x, y, yaw, trim = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for k in range(pairs_n):
        a, b = 2 * k, 2 * k + 1
        trim[a] = trim[b] = 1 + k % len(sizes)
        yaw[a] = yaw[b] = rng.uniform(0.05, 3.0) * (1 if k % 2 else -1)
        x[a], y[a] = 10.0 * k + rng.uniform(-2, 2), rng.uniform(-2, 2)  # (pairs far from each other)
        h = R.reachable_sets_at_pose(arrays, x[a], y[a], yaw[a], int(trim[a]))[-1]
        e = int(rng.integers(h.shape[1] - 1))
        d = h[:, e + 1] - h[:, e]
        d = d * (rng.uniform(0.1, 1.0) / np.hypot(d[0], d[1]))  # along edge e, 0.1 to 1.0 long (the hulls' radius is 1)
        x[b], y[b] = x[a] + d[0], y[a] + d[1]
    adj_d, area_d = handle.reachable_set_coupling(x, y, yaw, trim)
    adj_h, area_h = reachable_set_coupling_call(arrays, x, y, yaw, trim)
    assert np.array_equal(adj_d, adj_h) and np.array_equal(_bits(area_d), _bits(area_h))
    K = [s[-1] for s in _sets_at(table, arrays, x, y, yaw, trim)]
    passing = set(_passing_pairs(K))
    pairs = [(2 * k, 2 * k + 1) for k in range(pairs_n)]
    assert all(p in passing for p in pairs) and len(passing) == pairs_n
    checked = _check_pairs("device convex, same heading", K, pairs, adj_d, area_d, lambda i, j: X.area_convex_simple(K[i], K[j]))
    assert checked == pairs_n and adj_d.sum() == 2 * pairs_n


# ---- pdmpc_bound_sets_kernel


def _band(p, r_in, r_out, cx=0.0, cy=0.0, a0=-2.0, a1=2.0, bits=24):
    """a lanelet-like band of 2p vertices: p points on the arc of radius r_out from the angle a0 to a1 (the left boundary, counter-
    clockwise seen from the centre), then p points back on the arc of radius r_in — a band with a bend of |a1 − a0| radians"""
    out = [(X._quantized(cx + r_out * math.cos(a0 + (a1 - a0) * k / (p - 1)), bits), X._quantized(cy + r_out * math.sin(a0 + (a1 - a0) * k / (p - 1)), bits)) for k in range(p)]
    inn = [(X._quantized(cx + r_in * math.cos(a1 - (a1 - a0) * k / (p - 1)), bits), X._quantized(cy + r_in * math.sin(a1 - (a1 - a0) * k / (p - 1)), bits)) for k in range(p)]
    P = out + inn
    P = P[::-1] if X.area(P) < 0 else P
    assert X.is_simple(P)
    return P


def _bounding_batch():
    """(trim, raw lanelet polygon or None, what) per vehicle; every vehicle at yaw 0"""
    rng = np.random.default_rng(31)
    t = {m: SIZES.index(m) + 1 for m in SIZES}
    g64 = gear_case(64)[1]
    g65 = gear_case(65)[1]
    g128 = gear_case(128)[1]
    g256 = gear_case(256)[1]
    g32_65 = X.gear(32)
    g32_65 = g32_65[:1] + [((g32_65[0][0] + g32_65[1][0]) / 2, (g32_65[0][1] + g32_65[1][1]) / 2)] + g32_65[1:]  # 65: a collinear vertex
    g256_511 = g256[:5] + g256[6:]  # 511: one valley taken out (tooth to tooth, outside K)
    tri = [(Fraction(-1), Fraction(-1)), (Fraction(0), Fraction(2)), (Fraction(2), Fraction(-1))]
    cases = [
        (t[3], tri, "3 x 3"),
        (t[256], X.raw_variant(rng, tri, 3), "256 x 3, raw counter-clockwise with repeats"),
        (t[64], X.raw_variant(rng, g64, 0), "64 x gear 64: 257"),
        (t[65], X.raw_variant(rng, g65, 1), "65 x gear 65: 261, raw counter-clockwise"),
        (t[63], X.raw_variant(rng, X.gear(63), 2), "63 x gear 63, raw with repeats"),
        (t[8], None, "not bounded"),
        (t[128], g32_65, "128 x 65 vertices"),
        (t[128], X.raw_variant(rng, g128, 3), "128 x gear 128: 513, raw counter-clockwise with repeats"),
        (t[255], g256[::-1], "255 x gear 256: 1024, raw counter-clockwise"),
        (t[12], None, "not bounded"),
        (t[256], g256_511 + [g256_511[0]], "256 x 511 vertices, raw closed: 512"),
        (t[256], _band(32, 0.7, 1.1), "256 x band 64"),
        (t[65], X.raw_variant(rng, _band(64, 0.6, 0.8, 0.5, 0.0), 1), "65 x band 128, raw counter-clockwise"),
        (t[128], _band(256, 0.8, 1.3, 0.0, 0.25, -2.5, 2.5), "128 x band 512"),
        (t[3], _band(256, 0.55, 0.8, 0.0, 0.0, -3.0, 3.0), "3 x band 512: a ring that leaves the triangle through every edge"),
        (t[12], X.raw_variant(rng, X.gear(12), 3), "12 x gear 12"),
        (t[8], [(Fraction(5), Fraction(5)), (Fraction(5), Fraction(6)), (Fraction(6), Fraction(5))], "8 x far triangle: restored"),
    ]
    return cases


def test_bounding_at_the_declared_sizes(handle):
    table = _table()
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    cases = _bounding_batch()
    n = len(cases)
    trim = np.array([c[0] for c in cases])
    raws = [c[1] for c in cases]
    lan = [None if q is None else X.arr(q) for q in raws]
    z = np.zeros(n)
    raw_sizes = [0 if q is None else len(q) for q in raws]
    norm_sizes = [0 if q is None else len(X.normalized(q)) for q in raws]
    assert sorted(set(norm_sizes)) == [0, 3, 24, 64, 65, 126, 128, 130, 256, 511, 512] and max(raw_sizes) == 512
    assert sum(a > b for a, b in zip(raw_sizes, norm_sizes)) >= 5, "no polygon of the batch shrank: the gap is never closed"
    dev, fd = handle.bound_reachable_sets(z, z, z, trim, lan, 1)
    host, fh = bound_reachable_sets_call(arrays, z, z, z, trim, lan, 1)
    assert np.array_equal(fd, fh)
    for v in range(n):
        for q in range(2):
            assert dev[v][q].shape == host[v][q].shape and np.array_equal(_bits(dev[v][q]), _bits(host[v][q])), (cases[v][2], q)
    last, fl = handle.bound_reachable_sets(z, z, z, trim, lan, 0)
    assert np.array_equal(fl[:, 0], fd[:, 1]) and all(np.array_equal(_bits(last[v][0]), _bits(dev[v][1])) for v in range(n))
    counts = [dev[v][1].shape[1] for v in range(n)]
    assert counts[2] == 257 and counts[3] == 261 and counts[7] == 513 and counts[8] == 1024, counts  # more than 64, more than 512, exactly PDMPC_BOUNDED_MAX_COLS
    flags_seen = set()
    for v in range(n):
        if raws[v] is None:
            for q in range(2):
                assert fd[v, q] == 0 and np.array_equal(_bits(dev[v][q][:, :-1]), _bits(arrays[trim[v] - 1][q])), cases[v][2]
            continue
        Ln = X.normalized(raws[v])
        for q in range(2):
            K = table[trim[v] - 1][q]
            thorough = len(K) * len(Ln) <= 65 * 130
            tris = X.triangulate(Ln) if thorough else None
            check_bounded_set(ERRORS, "device bounding at the limits", "device", dev[v][q], int(fd[v, q]), K, Ln, False, (cases[v][2], q), tris, thorough, pinches=PINCHES)
            flags_seen.add(int(fd[v, q]))
    assert flags_seen == {0, R.BOUND_RESTORED, R.BOUND_MULTIPLE}, flags_seen


def test_bounding_gears_with_a_given_number_of_chains(handle):
    chains = [1, 2, 63, 64, 65, 255]
    cases = [chains_case(c) for c in chains]
    sizes = [len(K) for K, _ in cases]
    table = [[_hull(3, 0.5), K] for K, _ in cases]
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    n = len(cases)
    z = np.zeros(n)
    trim = np.arange(1, n + 1)
    lan = [X.arr(G) for _, G in cases]
    dev, fd = handle.bound_reachable_sets(z, z, z, trim, lan, 0)
    host, fh = bound_reachable_sets_call(arrays, z, z, z, trim, lan, 0)
    assert np.array_equal(fd, fh) and not fd.any()
    for v, c in enumerate(chains):
        K, G = cases[v]
        Ln = X.normalized(G)
        assert np.array_equal(_bits(dev[v][0]), _bits(host[v][0])), c
        assert dev[v][0].shape[1] == 3 * c + sizes[v] + 1, (c, dev[v][0].shape)  # entry, valley, exit per chain, K's vertices, the closing one
        if c <= 65:
            assert count_chains(K, Ln) == c
        check_bounded_set(ERRORS, "device bounding, chains", "device", dev[v][0], 0, K, Ln, False, c, X.fan(Ln, (Fraction(0), Fraction(0))), c <= 65, pinches=PINCHES)


def test_overflow_is_refused_and_leaves_the_handle_working(handle):
    table = _table()
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    K, G = gear_case(256)
    assert K == table[SIZES.index(256)][1]
    # a set of 1025 vertices in the middle of a batch: PDMPC_ERR_CAPACITY from the device and from the host twin
    trim = np.array([SIZES.index(m) + 1 for m in (64, 256, 12, 256)])
    lan = [X.arr(gear_case(64)[1]), X.arr(G), X.arr(X.gear(12)), X.arr(X.gear(64))]
    z = np.zeros(4)
    with pytest.raises(BackendError, match="status -4"):
        bound_reachable_sets_call(arrays, z, z, z, trim, lan, 0)
    with pytest.raises(BackendError, match="status -4.*PDMPC_BOUNDED_MAX_COLS"):
        handle.bound_reachable_sets(z, z, z, trim, lan, 0)
    # ... after which the coupler refuses to run on stale sets.  (Handle.bounded_set_coupling sizes its output by the vehicle count of
    # the last successful bounding, which on this module-scoped handle is whatever the test before left; the refused call above did not
    # set it, so it is set here, to this batch's 4 — the library returns PDMPC_ERR_INVALID before it touches the buffers.)
    handle._bound_n = 4
    with pytest.raises(BackendError, match="status -1"):
        handle.bounded_set_coupling()
    # ... and the next, normal batch is served as ever: nothing was written past a slot
    lan[1] = X.arr(X.gear(64))
    dev, fd = handle.bound_reachable_sets(z, z, z, trim, lan, 0)
    host, fh = bound_reachable_sets_call(arrays, z, z, z, trim, lan, 0)
    assert np.array_equal(fd, fh)
    for v in range(4):
        assert np.array_equal(_bits(dev[v][0]), _bits(host[v][0])), v
        Ln = X.poly(lan[v])
        check_bounded_set(ERRORS, "device bounding after an overflow", "device", dev[v][0], int(fd[v, 0]), table[trim[v] - 1][1], Ln, False, v, X.fan(Ln, (Fraction(0), Fraction(0))), v != 1, pinches=PINCHES)
    adj_d, area_d = handle.bounded_set_coupling()
    adj_h, area_h = polygon_set_coupling_call([s[0] for s in host])
    assert np.array_equal(adj_d, adj_h) and np.array_equal(_bits(area_d), _bits(area_h))
    # a hull of 257 vertices is refused at upload, and the table that was there stays in use
    x = np.array([0.0, 0.25, 0.5, 0.125])
    before = handle.reachable_set_coupling(x, z, z, trim)
    bad = [list(row) for row in arrays]
    bad[0][1] = X.arr(X.ngon(257, 1.0))
    with pytest.raises(BackendError, match="status -4.*PDMPC_REACHABLE_MAX_COLS"):
        handle.upload_reachable_sets(bad)
    after = handle.reachable_set_coupling(x, z, z, trim)
    ref = reachable_set_coupling_call(arrays, x, z, z, trim)
    for got in (before, after):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(_bits(got[1]), _bits(ref[1]))
    assert ref[0].sum() > 0


# ---- pdmpc_bounded_box_kernel / pdmpc_bounded_pairs_kernel


def _one_spot_batch():
    """128 vehicles on one spot, every one bounded by a gear (or not bounded) about its own centre, so that every bounded set is star-
    shaped about that centre; three of them with sets of 257, 513 and 1024 vertices"""
    rng = np.random.default_rng(41)
    n = 128
    t = {m: SIZES.index(m) + 1 for m in SIZES}
    trim = np.array([t[int(m)] for m in rng.choice([3, 8, 12], n)])
    x, y = _lattice(rng, n, 0.25), _lattice(rng, n, 0.25)
    lan = []
    for v in range(n):
        kind = int(rng.integers(4))
        if kind == 0:
            lan.append(None)
        else:
            G = X.gear((8, 12, 8)[kind - 1], 0.9 if kind < 3 else 0.45, 1.2, 0.0, float(x[v]), float(y[v]))
            lan.append(X.raw_variant(rng, G))
    for v, (m, T) in zip((5, 70, 127), ((64, 64), (128, 128), (255, 256))):
        trim[v] = t[m]
        lan[v] = X.gear(T, 0.9, 1.2, 0.0, float(x[v]), float(y[v]))
    return x, y, trim, lan


def test_bounded_coupler_beyond_its_grid_and_on_large_non_convex_sets(handle):
    table = _table()
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    x, y, trim, raws = _one_spot_batch()
    n = len(x)
    z = np.zeros(n)
    lan = [None if q is None else X.arr(q) for q in raws]
    dev, fd = handle.bound_reachable_sets(x, y, z, trim, lan, 0)
    host, fh = bound_reachable_sets_call(arrays, x, y, z, trim, lan, 0)
    assert np.array_equal(fd, fh) and all(np.array_equal(_bits(dev[v][0]), _bits(host[v][0])) for v in range(n))
    sets = [X.poly(s[0]) for s in host]
    assert [len(sets[v]) + 1 for v in (5, 70, 127)] == [257, 513, 1024]
    passing = _passing_pairs(sets)
    assert len(passing) == n * (n - 1) // 2 == 8128 > PAIR_BLOCKS, len(passing)  # the pair pass takes four trips of its grid
    adj_d, area_d = handle.bounded_set_coupling()
    adj_h, area_h = polygon_set_coupling_call([s[0] for s in host])
    assert np.array_equal(adj_d, adj_h) and np.array_equal(_bits(area_d), _bits(area_h))
    again = handle.bounded_set_coupling()  # the pair list comes out in another order: the same bits
    assert np.array_equal(again[0], adj_d) and np.array_equal(_bits(again[1]), _bits(area_d))
    centre = [(Fraction(float(x[v])), Fraction(float(y[v]))) for v in range(n)]
    fans = {}

    def exact(i, j):
        if len(sets[i]) > len(sets[j]):
            i, j = j, i
        if i not in fans:
            fans[i] = X.fan(sets[i], centre[i])
        return X.area_simple_simple(sets[i], sets[j], fans[i])

    rng = np.random.default_rng(42)
    pick = [passing[k] for k in rng.choice(len(passing), 500, replace=False)]
    pick += [(5, 70), (70, 127), (5, 127)]  # 257 x 513, 513 x 1024, 257 x 1024 vertices: both non-convex, more than 64 and more than 512
    checked = _check_pairs("device simple x simple, one spot", sets, pick, adj_d, area_d, exact)
    assert checked == 503, "a seeded sample of 500 of 8128 box-passing pairs and the three largest"
    assert adj_d.sum() > 0


# ---- state between the calls


def test_other_calls_between_bounding_and_coupling_leave_the_coupling_unchanged(handle):
    table = _table()
    arrays = _arrays(table)
    handle.upload_reachable_sets(arrays)
    rng = np.random.default_rng(51)
    n = 12
    x, y, z = _lattice(rng, n, 0.5), _lattice(rng, n, 0.5), np.zeros(n)
    trim = rng.integers(1, 7, n)
    lan = [X.arr(X.gear(12, 0.9, 1.2, 0.0, float(x[v]), float(y[v]))) if v % 3 else None for v in range(n)]
    host, _ = bound_reachable_sets_call(arrays, x, y, z, trim, lan, 1)
    want = polygon_set_coupling_call([s[-1] for s in host])
    handle.bound_reachable_sets(x, y, z, trim, lan, 1)
    first = handle.bounded_set_coupling()
    handle.bound_reachable_sets(x, y, z, trim, lan, 1)
    adj_r, _ = handle.reachable_set_coupling(x + 0.125, y, z, trim)
    ref = [np.stack([x[v] + 0.1 * np.arange(4), y[v] + 0.05 * np.arange(4)], axis=1) for v in range(n)]
    sparse = np.triu(adj_r, 1) * (np.add.outer(np.arange(n), np.arange(n)) % 3 == 0)
    handle.fca_collisions(ref, fca_pairs(sparse + sparse.T), 0.22, 0.1, 0.01)
    A = np.zeros((n, n), dtype=np.int64)
    for v in range(n - 1):
        A[v, v + 1] = A[v + 1, v] = 1
    handle.unique_priorities(A, 1 << n)
    second = handle.bounded_set_coupling()
    for got in (first, second):
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert want[0].sum() > 0


def test_zz_no_case_is_pinched_and_write_the_error_record():
    """Every bounded set of this module met the strict check; and, not a check: writes this module's section of
    profiles/exact_geometry_errors.txt where PDMPC_EXACT_GEOMETRY_REPORT says (the suite's conftest offers no hook for it)."""
    assert PINCHES.n >= 30 and PINCHES.pinched == 0, (PINCHES.n, PINCHES.pinched)
    for line in ERRORS.lines():
        print(line)
    write_report(ERRORS, "device")
