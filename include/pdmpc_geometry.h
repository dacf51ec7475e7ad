/* pdmpc_geometry.h — the convex geometry of the reachable-set coupler, shared by host and device.
 *
 * ReachableSetCoupler.couple (hlc/controller/common/couple/ReachableSetCoupler.m:5-56) couples two vehicles whose step-Hp
 * reachable sets overlap by more than 1e-3 m^2.  The sets are convex hulls (MotionPrimitiveAutomaton.local_reachable_sets_conv),
 * so the overlap is a convex-convex intersection; its area follows from Green's theorem over the boundary of A ∩ B: the parts
 * of A's edges inside B (closed: on B's boundary counts, an edge running along an edge of B in the same direction too) plus
 * the parts of B's edges strictly inside A, each contributing cross(p0, p1) / 2 (both polygons clockwise, so the sum is
 * minus twice the area).  A shared edge is counted once, an edge where the two only touch from outside not at all.
 *
 * Every function is one definition for the host twin (csrc/reachable_sets.cpp), the kernel (csrc/reachable_kernel.hip) and,
 * operation by operation, p-dmpc_amd/pdmpc/reachability.py; all of them are compiled with -ffp-contract=off, so every
 * expression is the same sequence of IEEE-754 double operations and the three give the same bits.
 */
#ifndef PDMPC_GEOMETRY_H
#define PDMPC_GEOMETRY_H

#include "pdmpc_math.h" /* PDMPC_HD */

#define PDMPC_COUPLING_AREA_THRESHOLD 1e-3 /* ReachableSetCoupler.m:48 */

/* orientation of b relative to the directed line o -> a (> 0: left of it) */
PDMPC_HD static inline double pdmpc_cross3(double ox, double oy, double ax, double ay, double bx, double by) {
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox);
}

/* translate_global (utility/translate_global.m:19-22) of one point with c = cos(yaw), s = sin(yaw) */
PDMPC_HD static inline void pdmpc_move_point(double c, double s, double x0, double y0, double a, double b, double* gx, double* gy) {
    *gx = c * a + (-s) * b + x0;
    *gy = s * a + c * b + y0;
}

/* Cyrus–Beck clip of the segment (ax, ay) -> (bx, by) against the clockwise convex polygon (qx, qy)[0 .. m) (edges q[k] -> q[k+1],
 * the last one back to q[0]).  strict = 0: the part inside the polygon or on its boundary (a segment along an edge of the polygon
 * only if it runs in the same direction); strict = 1: the part strictly inside.  Returns 1 and *cross = cross(p0, p1) of the
 * clipped part if it has positive length, 0 otherwise. */
PDMPC_HD static inline int pdmpc_clip_edge(double ax, double ay, double bx, double by, const double* qx, const double* qy, int m, int strict,
                                           double* cross) {
    const double dx = bx - ax, dy = by - ay;
    double tmin = 0.0, tmax = 1.0;
    for (int k = 0; k < m; ++k) {
        const int k1 = k + 1 == m ? 0 : k + 1;
        const double ux = qx[k1] - qx[k], uy = qy[k1] - qy[k];
        const double num = ux * (ay - qy[k]) - uy * (ax - qx[k]);
        const double den = ux * dy - uy * dx;
        if (den == 0.0) {
            if (strict) {
                if (num >= 0.0) return 0;
            } else if (num > 0.0 || (num == 0.0 && !(ux * dx + uy * dy > 0.0))) {
                return 0;
            }
        } else {
            const double t = -num / den;
            if (den < 0.0) {
                if (t > tmin) tmin = t;
            } else {
                if (t < tmax) tmax = t;
            }
        }
    }
    if (!(tmin < tmax)) return 0;
    const double p0x = ax + tmin * dx, p0y = ay + tmin * dy;
    const double p1x = ax + tmax * dx, p1y = ay + tmax * dy;
    *cross = p0x * p1y - p1x * p0y;
    return 1;
}

/* Reachable-set coupler's pre-filter (ReachableSetCoupler.m:33-36): 1 if the boxes [x0, x1] x [y0, y1] of i and j can overlap
 * (boxes that only touch cannot) */
PDMPC_HD static inline int pdmpc_boxes_overlap(const double* bi, const double* bj) {
    return !(bi[0] >= bj[1] || bi[2] >= bj[3] || bi[1] <= bj[0] || bi[3] <= bj[2]);
}

#endif /* PDMPC_GEOMETRY_H */
