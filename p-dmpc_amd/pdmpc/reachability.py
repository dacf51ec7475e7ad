"""Reachable sets of the motion-primitive automaton and the reachable-set coupler.

    local sets      MotionPrimitiveAutomaton.reachability_analysis_offline_DP (MotionPrimitiveAutomaton.m:394-647), convexified
    sets at a pose  MotionPrimitiveAutomaton.reachable_sets_at_pose (:649-687), closed as HighLevelController.m:258-263 does
    coupler         ReachableSetCoupler.couple (hlc/controller/common/couple/ReachableSetCoupler.m:5-56)

The reference only ever uses the convex hulls of the sets (`local_reachable_sets_conv`), so everything here is convex
geometry: the hull of a union is the hull of the union's vertices, the hull of a rigidly moved set is the moved hull, and the
overlap of two hulls is a convex-convex intersection.  csrc/reachable_sets.cpp is the C++ twin of this module and
include/pdmpc_geometry.h the arithmetic both share with the coupling kernel (csrc/reachable_kernel.hip): every operation here
is a single IEEE double operation in the same order, so the three give the same bits.
"""
import math
from typing import List

import numpy as np

# ReachableSetCoupler.m:48: overlap areas up to this are "not coupled" (tolerates inaccuracies of lanelet boundaries)
COUPLING_AREA_THRESHOLD = 1e-3
# hull pre-filter: a point more than this (m^2 of cross product) inside the octagon of extreme points cannot be a hull vertex
HULL_PREFILTER_EPS = 1e-9


def _cross(ox, oy, ax, ay, bx, by):
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox)


def convex_hull(xs, ys) -> np.ndarray:
    """Convex hull of a point set as a (2, m) array: clockwise, collinear vertices dropped, starting at the smallest x (then
    the smallest y), the first vertex not repeated (polyshape's vertex order).  Andrew's monotone chain after dropping the
    points that lie deep inside the octagon spanned by the extreme points of eight directions."""
    x = np.asarray(xs, dtype=np.float64).ravel()
    y = np.asarray(ys, dtype=np.float64).ravel()
    if x.size >= 8:
        keys = (x, x + y, y, y - x, -x, -(x + y), -y, x - y)  # outward normals in counter-clockwise order
        corners = [int(np.argmax(k)) for k in keys]
        inside = np.ones(x.size, dtype=bool)
        for c in range(8):
            a, b = corners[c], corners[(c + 1) % 8]
            inside &= _cross(x[a], y[a], x[b], y[b], x, y) > HULL_PREFILTER_EPS
        keep = ~inside
        x, y = x[keep], y[keep]
    order = np.lexsort((y, x))
    px = x[order].tolist()
    py = y[order].tolist()
    n = len(px)
    if n < 3:
        pts = sorted(set(zip(px, py)))
        return np.array(pts, dtype=np.float64).T.reshape(2, -1)
    lower = []
    for i in range(n):
        while len(lower) >= 2:
            o, a = lower[-2], lower[-1]
            if _cross(px[o], py[o], px[a], py[a], px[i], py[i]) <= 0:
                lower.pop()
            else:
                break
        lower.append(i)
    upper = []
    for i in range(n - 1, -1, -1):
        while len(upper) >= 2:
            o, a = upper[-2], upper[-1]
            if _cross(px[o], py[o], px[a], py[a], px[i], py[i]) <= 0:
                upper.pop()
            else:
                break
        upper.append(i)
    ccw = lower[:-1] + upper[:-1]
    cw = [ccw[0]] + ccw[:0:-1]
    return np.array([[px[i] for i in cw], [py[i] for i in cw]], dtype=np.float64)


def translate_global(yaw, x0, y0, xl, yl):
    """utility/translate_global.m:19-22 on arrays (the elementwise operations are the scalar ones, in the same order)."""
    c, s = math.cos(yaw), math.sin(yaw)
    xl = np.asarray(xl, dtype=np.float64)
    yl = np.asarray(yl, dtype=np.float64)
    return c * xl + (-s) * yl + x0, s * xl + c * yl + y0


def _end_pose(pose, m):
    """End pose of maneuver m started at pose (x0, y0, yaw0): the last column of the translated maneuver."""
    x0, y0, yaw0 = pose
    c, s = math.cos(yaw0), math.sin(yaw0)
    return (c * m.dx + (-s) * m.dy + x0, s * m.dx + c * m.dy + y0, yaw0 + m.dyaw)


def _areas_hull(mpa, parents, slice_k):
    """Hull of the maneuver areas of every (parent trim, start pose) in `parents` towards every child of transition slice
    slice_k (0-based); also the children in the reference's order (trimsInfo.childTrims / maneuvers)."""
    T = mpa.transition_matrix_single
    xs, ys, children = [], [], []
    for trim, pose in parents:
        for child in np.nonzero(T[trim, :, slice_k])[0]:
            m = mpa.maneuvers[trim][int(child)]
            ax, ay = translate_global(pose[2], pose[0], pose[1], m.area[0], m.area[1])
            xs.append(ax)
            ys.append(ay)
            children.append((int(child), _end_pose(pose, m)))
    return convex_hull(np.concatenate(xs), np.concatenate(ys)), children


def local_reachable_sets_conv(mpa) -> List[List[np.ndarray]]:
    """reachability_analysis_offline_DP (MotionPrimitiveAutomaton.m:394-647), convexified: [trim][k] = (2, m) hull of the
    area trim (0-based) can reach at step k+1 from the origin, in polyshape's vertex order."""
    Hp = mpa.Hp
    n = mpa.n_trims
    Hp_half = (Hp + 1) // 2
    first = [[None] * Hp_half for _ in range(n)]  # hulls of steps 1..Hp_half
    steps = [[None] * Hp_half for _ in range(n)]  # trimsInfo(i, t).maneuvers: (child trim, end pose) of step t
    parents_at = [[None] * Hp_half for _ in range(n)]  # trimsInfo(i, t).parentTrims with their start poses
    for i in range(n):  # :431-520
        parents = [(i, (0.0, 0.0, 0.0))]
        for t in range(Hp_half):
            parents_at[i][t] = parents
            first[i][t], steps[i][t] = _areas_hull(mpa, parents, t)
            parents = steps[i][t]
    half_final = [None] * n
    if Hp > 1:  # :525-585: Hp_half as the last step, children from the last transition slice
        for i in range(n):
            half_final[i], _ = _areas_hull(mpa, parents_at[i][Hp_half - 1], Hp - 1)
    out = [[None] * Hp for _ in range(n)]
    for i in range(n):
        for t in range(Hp_half):
            out[i][t] = first[i][t]
        for t in range(Hp_half + 1, Hp + 1):  # :587-623 (1-based t)
            xs, ys = [], []
            for child, pose in steps[i][t - Hp_half - 1]:
                h = half_final[child] if t == Hp else first[child][Hp_half - 1]
                ax, ay = translate_global(pose[2], pose[0], pose[1], h[0], h[1])
                xs.append(ax)
                ys.append(ay)
            out[i][t - 1] = convex_hull(np.concatenate(xs), np.concatenate(ys))
    return out


def reachable_sets_at_pose(local_sets, x, y, yaw, trim) -> List[np.ndarray]:
    """reachable_sets_at_pose (MotionPrimitiveAutomaton.m:649-687) for a 1-based trim: the Hp local hulls moved to (x, y, yaw),
    each closed by repeating its first vertex (HighLevelController.m:258-263)."""
    out = []
    for h in local_sets[trim - 1]:
        gx, gy = translate_global(yaw, x, y, h[0], h[1])
        out.append(np.array([np.append(gx, gx[0]), np.append(gy, gy[0])]))
    return out


ORIENT_SNAP = 2.0**-40


def _orient(dx, dy, rx, ry):
    """pdmpc_orient: dx * ry - dy * rx, with rounding noise (below 2^-40 |d| (|d| + |r|), 1-norms) taken for 0."""
    o = dx * ry - dy * rx
    n = np.abs(dx) + np.abs(dy)
    return np.where(np.abs(o) <= ORIENT_SNAP * (n * (n + (np.abs(rx) + np.abs(ry)))), 0.0, o)


def _clipped_sum(ax, ay, bx, by, strict, total):
    """`total` plus, one edge after the other, cross(p0, p1) of the edges of polygon a (open, clockwise) clipped to polygon b
    (Cyrus-Beck).  closed (strict = False): the part inside b or on its boundary, an edge that runs along an edge of b in the same direction
    included; strict: the part strictly inside b."""
    ex0, ey0 = ax, ay
    ex1, ey1 = np.roll(ax, -1), np.roll(ay, -1)
    dx, dy = ex1 - ex0, ey1 - ey0
    qx0, qy0 = bx, by
    qx1, qy1 = np.roll(bx, -1), np.roll(by, -1)
    ux, uy = qx1 - qx0, qy1 - qy0
    # [edge of a, edge of b]: value of cross(u, p - q0) at the start of the a-edge, and its rate along the a-edge
    num = _orient(ux[None, :], uy[None, :], ex0[:, None] - qx0[None, :], ey0[:, None] - qy0[None, :])
    den = _orient(ux[None, :], uy[None, :], dx[:, None], dy[:, None])
    par = den == 0.0
    if strict:
        dead = par & (num >= 0.0)
    else:
        same = (ux[None, :] * dx[:, None] + uy[None, :] * dy[:, None]) > 0.0
        dead = par & ((num > 0.0) | ((num == 0.0) & ~same))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -num / den
    tmin = np.max(np.where(den < 0.0, t, 0.0), axis=1, initial=0.0)
    tmax = np.min(np.where(den > 0.0, t, 1.0), axis=1, initial=1.0)
    for e in range(ax.size):
        if dead[e].any() or not tmin[e] < tmax[e]:
            continue
        p0x = ex0[e] + tmin[e] * dx[e]
        p0y = ey0[e] + tmin[e] * dy[e]
        p1x = ex0[e] + tmax[e] * dx[e]
        p1y = ey0[e] + tmax[e] * dy[e]
        total = total + (p0x * p1y - p1x * p0y)
    return total


def overlap_area(a, b) -> float:
    """Area of the intersection of two convex polygons given clockwise as (2, m) arrays (a closing repeated vertex is
    ignored): Green's theorem over the boundary of the intersection, i.e. the edges of a inside b plus the edges of b strictly
    inside a, in coordinates relative to a's first vertex, summed in edge order."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape[1] > 1 and a[0, 0] == a[0, -1] and a[1, 0] == a[1, -1]:
        a = a[:, :-1]
    if b.shape[1] > 1 and b[0, 0] == b[0, -1] and b[1, 0] == b[1, -1]:
        b = b[:, :-1]
    ox, oy = a[0, 0], a[1, 0]
    ax, ay = a[0] - ox, a[1] - oy
    bx, by = b[0] - ox, b[1] - oy
    s = _clipped_sum(ax, ay, bx, by, False, 0.0)
    s = _clipped_sum(bx, by, ax, ay, True, s)
    return -0.5 * s


def reachable_set_coupling(sets):
    """ReachableSetCoupler.couple on the closed step-Hp sets of every vehicle: (adjacency (n, n) int64, areas (n, n) with the
    overlap area of every pair that passed the bounding-box test, 0 elsewhere)."""
    n = len(sets)
    adj = np.zeros((n, n), dtype=np.int64)
    areas = np.zeros((n, n), dtype=np.float64)
    boxes = [(float(np.min(s[0])), float(np.max(s[0])), float(np.min(s[1])), float(np.max(s[1]))) for s in sets]
    for i in range(n - 1):
        xi0, xi1, yi0, yi1 = boxes[i]
        for j in range(i + 1, n):
            xj0, xj1, yj0, yj1 = boxes[j]
            if xi0 >= xj1 or yi0 >= yj1 or xi1 <= xj0 or yi1 <= yj0:  # :33-36
                continue
            a = overlap_area(sets[i], sets[j])
            areas[i, j] = areas[j, i] = a
            if a > COUPLING_AREA_THRESHOLD:
                adj[i, j] = adj[j, i] = 1
    return adj, areas


# ---- lanelet bounding of the reachable sets (bound_reachable_sets.m, HighLevelController.m:241-246; include/pdmpc_geometry.h) ----
BOUND_RESTORED = 1  # K ∩ L was empty: K returned unchanged
BOUND_MULTIPLE = 2  # K ∩ L had more than one region: the one with the most vertices was kept


def lanelet_polygon(left, right) -> np.ndarray:
    """The predicted-lanelet polygon of get_lanelets_boundary.m:69-74: the left boundary, then the reversed right boundary, (2, P)."""
    left = np.asarray(left, dtype=np.float64).reshape(2, -1)
    right = np.asarray(right, dtype=np.float64).reshape(2, -1)
    return np.concatenate([left, right[:, ::-1]], axis=1)


def normalize_lanelet_polygon(poly) -> np.ndarray:
    """pdmpc_lanelet_polygon_normalize: consecutive duplicate vertices (and trailing copies of the first) dropped, reversed if the
    signed area is positive -> clockwise (2, m)."""
    p = np.asarray(poly, dtype=np.float64).reshape(2, -1)
    xs, ys = [], []
    for x, y in zip(p[0].tolist(), p[1].tolist()):
        if xs and x == xs[-1] and y == ys[-1]:
            continue
        xs.append(x)
        ys.append(y)
    while len(xs) > 1 and xs[-1] == xs[0] and ys[-1] == ys[0]:
        xs.pop()
        ys.pop()
    x = np.array(xs, dtype=np.float64)
    y = np.array(ys, dtype=np.float64)
    if x.size:
        terms = x * np.roll(y, -1) - np.roll(x, -1) * y
        if np.cumsum(terms)[-1] > 0.0:
            x, y = x[::-1].copy(), y[::-1].copy()
    return np.array([x, y]).reshape(2, -1)


def _clip_table(lx, ly, kx, ky):
    """pdmpc_clip_edge_t for every edge of L (open) against the clockwise convex K (open) -> (tmin, tmax) per L edge."""
    dx, dy = np.roll(lx, -1) - lx, np.roll(ly, -1) - ly
    ux, uy = np.roll(kx, -1) - kx, np.roll(ky, -1) - ky
    num = _orient(ux[None, :], uy[None, :], lx[:, None] - kx[None, :], ly[:, None] - ky[None, :])
    den = _orient(ux[None, :], uy[None, :], dx[:, None], dy[:, None])
    dead = ((den == 0.0) & (num >= 0.0)).any(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -num / den
    tmin = np.max(np.where(den < 0.0, t, 0.0), axis=1, initial=0.0) + 0.0  # (+ 0.0: the C loop never holds -0.0)
    tmax = np.min(np.where(den > 0.0, t, 1.0), axis=1, initial=1.0)
    tmin[dead] = 1.0
    tmax[dead] = 0.0
    return tmin.tolist(), tmax.tolist()


def _boundary_position(px, py, kx, ky):
    """pdmpc_boundary_position -> (K edge, parameter)."""
    m = len(kx)
    best, bv = 0, 0.0
    for k in range(m):
        k1 = 0 if k + 1 == m else k + 1
        v = (kx[k1] - kx[k]) * (py - ky[k]) - (ky[k1] - ky[k]) * (px - kx[k])
        if k == 0 or v > bv:
            bv, best = v, k
    b1 = 0 if best + 1 == m else best + 1
    ux, uy = kx[b1] - kx[best], ky[b1] - ky[best]
    s = ((px - kx[best]) * ux + (py - ky[best]) * uy) / (ux * ux + uy * uy)
    if s < 0.0:
        s = 0.0
    if s >= 1.0:
        best, s = b1, 0.0
    return best, s


def bound_reachable_set(K, L):
    """bound_reachable_sets.m for one set: K (2, m) convex, clockwise (a closing repeated vertex is ignored), L the vehicle's
    normalized lanelet polygon (normalize_lanelet_polygon; fewer than 3 vertices: no clipping) -> (the kept region of K ∩ L, closed,
    (2, c); flags BOUND_*).  The rules are pdmpc_bound_region's (include/pdmpc_geometry.h), operation by operation."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape[1] > 1 and K[0, 0] == K[0, -1] and K[1, 0] == K[1, -1]:
        K = K[:, :-1]
    kx, ky = K[0].tolist(), K[1].tolist()
    m = len(kx)
    L = np.asarray(L, dtype=np.float64).reshape(2, -1)
    lx, ly = L[0].tolist(), L[1].tolist()
    nl = len(lx)
    flags = 0
    out = None
    if m >= 3 and nl >= 3:
        tmin, tmax = _clip_table(L[0], L[1], K[0], K[1])
        alive = [tmin[e] < tmax[e] for e in range(nl)]
        link = [alive[e] and alive[(e + 1) % nl] and tmax[e] == 1.0 and tmin[(e + 1) % nl] == 0.0 for e in range(nl)]
        if all(link):
            out = (lx, ly)
        else:
            starts = [e for e in range(nl) if alive[e] and not link[nl - 1 if e == 0 else e - 1]]
            C = len(starts)
            ends, kin, sin, kout, sout = [], [], [], [], []
            for s in starts:
                e = s
                while link[e]:
                    e = 0 if e + 1 == nl else e + 1
                ends.append(e)
                s1, e1 = (s + 1) % nl, (e + 1) % nl
                k, p = _boundary_position(lx[s] + tmin[s] * (lx[s1] - lx[s]), ly[s] + tmin[s] * (ly[s1] - ly[s]), kx, ky)
                kin.append(k)
                sin.append(p)
                k, p = _boundary_position(lx[e] + tmax[e] * (lx[e1] - lx[e]), ly[e] + tmax[e] * (ly[e1] - ly[e]), kx, ky)
                kout.append(k)
                sout.append(p)

            def steps(c, d):
                dk = kin[d] - kout[c]
                if dk < 0:
                    dk += m
                if dk == 0 and sin[d] < sout[c]:
                    dk = m
                return dk

            def link_vertices(c, d):
                dk = steps(c, d)
                return dk - 1 if dk > 0 and sin[d] == 0.0 else dk

            nxt = []
            for c in range(C):
                bd, bk = -1, 0
                for d in range(C):
                    dk = steps(c, d)
                    if bd < 0 or dk < bk or (dk == bk and sin[d] < sin[bd]):
                        bd, bk = d, dk
                nxt.append(bd)
            region = [0] * C
            n_regions, best, best_count, best_steps = 0, -1, 0, 0
            for c in range(C):
                if region[c]:
                    continue
                cnt = n_steps = 0
                cur = c
                while True:
                    region[cur] = c + 1
                    cnt += 2 + (ends[cur] - starts[cur]) % nl + link_vertices(cur, nxt[cur])
                    n_steps += 1
                    cur = nxt[cur]
                    if region[cur]:
                        break
                if cnt >= 3:
                    n_regions += 1
                    if cnt > best_count:
                        best_count, best, best_steps = cnt, c, n_steps
            if C == 0:  # K ⊂ L, or K ∩ L is empty
                cx = cy = 0.0
                for q in range(m):
                    cx = cx + kx[q]
                    cy = cy + ky[q]
                cx = cx / float(m)
                cy = cy / float(m)
                inside = False
                for i in range(nl):
                    j = 0 if i + 1 == nl else i + 1
                    if (ly[i] > cy) != (ly[j] > cy):
                        xi = lx[i] + (cy - ly[i]) * (lx[j] - lx[i]) / (ly[j] - ly[i])
                        if cx < xi:
                            inside = not inside
                if not inside:
                    flags |= BOUND_RESTORED
            elif n_regions == 0:
                flags |= BOUND_RESTORED
            else:
                if n_regions > 1:
                    flags |= BOUND_MULTIPLE
                ox, oy = [], []
                cur = best
                for _ in range(best_steps):
                    s, e = starts[cur], ends[cur]
                    s1, e1 = (s + 1) % nl, (e + 1) % nl
                    ox.append(lx[s] + tmin[s] * (lx[s1] - lx[s]))
                    oy.append(ly[s] + tmin[s] * (ly[s1] - ly[s]))
                    for q in range(1, (e - s) % nl + 1):
                        ox.append(lx[(s + q) % nl])
                        oy.append(ly[(s + q) % nl])
                    ox.append(lx[e] + tmax[e] * (lx[e1] - lx[e]))
                    oy.append(ly[e] + tmax[e] * (ly[e1] - ly[e]))
                    d = nxt[cur]
                    for q in range(1, link_vertices(cur, d) + 1):
                        ox.append(kx[(kout[cur] + q) % m])
                        oy.append(ky[(kout[cur] + q) % m])
                    cur = d
                out = (ox, oy)
    if out is None:
        out = (kx, ky)
    x = np.array(list(out[0]) + [out[0][0]], dtype=np.float64)
    y = np.array(list(out[1]) + [out[1][0]], dtype=np.float64)
    return np.array([x, y]), flags


def bound_reachable_sets(sets, lanelet_poly):
    """bound_reachable_sets.m on a vehicle's Hp closed sets (reachable_sets_at_pose) with its raw lanelet polygon (lanelet_polygon;
    None or fewer than 3 distinct vertices: not clipped) -> (bounded closed sets, flags per set)."""
    if lanelet_poly is None:
        return list(sets), [0] * len(sets)
    L = normalize_lanelet_polygon(lanelet_poly)
    out, flags = [], []
    for K in sets:
        r, f = bound_reachable_set(K, L)
        out.append(r)
        flags.append(f)
    return out, flags


def _inside_fractions(ax, ay, px, py, strict):
    """pdmpc_edge_inside_fraction for every edge of (ax, ay) (open) against the polygon (px, py) (open)."""
    bx, by = np.roll(ax, -1), np.roll(ay, -1)
    dx, dy = bx - ax, by - ay
    dd = dx * dx + dy * dy
    cx, cy = px[None, :], py[None, :]
    ex, ey = np.roll(px, -1)[None, :], np.roll(py, -1)[None, :]
    AX, AY, DX, DY, DD = ax[:, None], ay[:, None], dx[:, None], dy[:, None], dd[:, None]
    oc = _orient(DX, DY, cx - AX, cy - AY)
    oe = _orient(DX, DY, ex - AX, ey - AY)
    lc = oc > 0.0 if strict else oc >= 0.0
    le = oe > 0.0 if strict else oe >= 0.0
    cross = lc != le
    wx, wy = ex - cx, ey - cy
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = ((cx - AX) * DX + (cy - AY) * DY) / DD
        te = ((ex - AX) * DX + (ey - AY) * DY) / DD
        tl = ((cx - AX) * wy - (cy - AY) * wx) / (DX * wy - DY * wx)
    t = np.where(oc == 0.0, tc, np.where(oe == 0.0, te, tl))
    inner = cross & (t < 1.0) & (t > 0.0)
    acc = np.cumsum(np.where(inner, np.where(lc, t, -t), 0.0), axis=1)[:, -1] if px.size else np.zeros(ax.size)
    par = (np.count_nonzero(cross & (t >= 1.0), axis=1) & 1).astype(np.float64)
    f = acc + par
    if strict:
        opp = ~cross & (oc == 0.0) & (oe == 0.0) & (DX * wx + DY * wy < 0.0)
        lo = np.maximum(np.minimum(tc, te), 0.0)  # (no NaN: DD > 0 where it is read)
        hi = np.minimum(np.maximum(tc, te), 1.0)
        use = opp & (hi > lo)
        corr = np.cumsum(np.where(use, hi - lo, 0.0), axis=1)[:, -1] if px.size else np.zeros(ax.size)
        f = f - corr
    f = np.where(dd == 0.0, 0.0, f)
    return f


def polygon_overlap_area(a, b) -> float:
    """Area of the intersection of two simple clockwise polygons (2, m) (a closing repeated vertex is ignored): Green's theorem
    over the boundary of A ∩ B with the crossing rule of pdmpc_edge_inside_fraction (include/pdmpc_geometry.h), in coordinates
    relative to a's first vertex, A's edge terms then B's summed in edge order."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape[1] > 1 and a[0, 0] == a[0, -1] and a[1, 0] == a[1, -1]:
        a = a[:, :-1]
    if b.shape[1] > 1 and b[0, 0] == b[0, -1] and b[1, 0] == b[1, -1]:
        b = b[:, :-1]
    ox, oy = a[0, 0], a[1, 0]
    ax, ay = a[0] - ox, a[1] - oy
    bx, by = b[0] - ox, b[1] - oy
    fa = _inside_fractions(ax, ay, bx, by, False)
    fb = _inside_fractions(bx, by, ax, ay, True)
    ta = fa * (ax * np.roll(ay, -1) - np.roll(ax, -1) * ay)
    tb = fb * (bx * np.roll(by, -1) - np.roll(bx, -1) * by)
    total = np.cumsum(np.concatenate([[0.0], ta, tb]))[-1]
    return -0.5 * float(total)


def polygon_set_coupling(sets):
    """ReachableSetCoupler.couple on any simple closed clockwise sets (the bounded step-Hp sets): the box pre-filter of
    reachable_set_coupling, polygon_overlap_area for every pair that passes it -> (adjacency (n, n) int64, areas (n, n))."""
    n = len(sets)
    adj = np.zeros((n, n), dtype=np.int64)
    areas = np.zeros((n, n), dtype=np.float64)
    boxes = [(float(np.min(s[0])), float(np.max(s[0])), float(np.min(s[1])), float(np.max(s[1]))) for s in sets]
    for i in range(n - 1):
        xi0, xi1, yi0, yi1 = boxes[i]
        for j in range(i + 1, n):
            xj0, xj1, yj0, yj1 = boxes[j]
            if xi0 >= xj1 or yi0 >= yj1 or xi1 <= xj0 or yi1 <= yj0:
                continue
            a = polygon_overlap_area(sets[i], sets[j])
            areas[i, j] = areas[j, i] = a
            if a > COUPLING_AREA_THRESHOLD:
                adj[i, j] = adj[j, i] = 1
    return adj, areas
