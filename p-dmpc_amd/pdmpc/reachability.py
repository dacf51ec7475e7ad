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
    num = ux[None, :] * (ey0[:, None] - qy0[None, :]) - uy[None, :] * (ex0[:, None] - qx0[None, :])
    den = ux[None, :] * dy[:, None] - uy[None, :] * dx[:, None]
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
