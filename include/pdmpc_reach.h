/* pdmpc_reach.h — which obstacle segments an edge check of step k can ever meet, shared by host and device.
 *
 * A node of step k has a parent k - 1 maneuvers away from the search's root, and its area reaches at most Amax beyond the parent:
 * every point of every area a search checks at step k lies within R_k = (k - 1) Dmax + Amax of the root, with Dmax the longest
 * maneuver displacement of the automaton and Amax the largest |area point| over its three area variants (used columns only).
 * A segment whose bounding box lies outside the square root +- rho_k (rho_k = R_k plus a margin far above the rounding of an
 * accumulated pose) cannot cross such an area, and a segment with a NaN coordinate gives InterX (InterX.m:63-76) NaN products,
 * none of which is < 0: neither can set an edge's flag.  Everything else is "in reach" — in particular whatever is infinite or so
 * large that the box arithmetic itself could overflow.  The square, not the disc: four comparisons, and it only errs towards "in".
 *
 * That is the disc bound (pdmpc_reach_box, pdmpc_reach_in; host twin pdmpc_reach_lists_host).  The kernel's list builder
 * (csrc/bulk_search.hpp: bk_reach_build) and the arrival rule (bk_incorporate_body) follow the oriented rule further down, which knows
 * where the automaton can go (pdmpc_reach_rect_box, pdmpc_reach_in_oriented; host twin pdmpc_reach_lists_oriented_host).  One
 * definition each for device and host; all are compiled with -ffp-contract=off, so they give the same bits.
 */
#ifndef PDMPC_REACH_H
#define PDMPC_REACH_H

#include <math.h>

#include "pdmpc_math.h" /* PDMPC_HD */

#define PDMPC_REACH_FINITE 0x1p64   /* coordinates beyond this are never culled */
#define PDMPC_REACH_MARGIN 0x1p-20 /* relative margin of rho_k */

/* R_k, rounded up: the sum's rounding error is below 2^-52 of it */
PDMPC_HD static inline double pdmpc_reach_radius(double dmax, double amax, int k) {
    const double r = (double)(k - 1) * dmax + amax;
    return r + r * 0x1p-50;
}

/* the square of step k around the root: box = (x_lo, x_hi, y_lo, y_hi) */
PDMPC_HD static inline void pdmpc_reach_box(double dmax, double amax, int k, double root_x, double root_y, double* box) {
    const double R = pdmpc_reach_radius(dmax, amax, k);
    const double rho = R + PDMPC_REACH_MARGIN * (1.0 + fabs(root_x) + fabs(root_y) + R);
    box[0] = root_x - rho;
    box[1] = root_x + rho;
    box[2] = root_y - rho;
    box[3] = root_y + rho;
}

/* 1: the segment (x0, y0) - (x1, y1) is in reach of the step whose square is (x_lo, x_hi, y_lo, y_hi) */
PDMPC_HD static inline int pdmpc_reach_in(double x0, double y0, double x1, double y1, double x_lo, double x_hi, double y_lo, double y_hi) {
    if (x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1) return 0;
    const int bounded = fabs(x0) <= PDMPC_REACH_FINITE && fabs(y0) <= PDMPC_REACH_FINITE && fabs(x1) <= PDMPC_REACH_FINITE && fabs(y1) <= PDMPC_REACH_FINITE;
    if (!bounded) return 1;
    const double max_x = x0 > x1 ? x0 : x1, min_x = x0 < x1 ? x0 : x1;
    const double max_y = y0 > y1 ? y0 : y1, min_y = y0 < y1 ? y0 : y1;
    return !(max_x < x_lo || min_x > x_hi || max_y < y_lo || min_y > y_hi);
}

/* ---- the oriented rule: the automaton drives forwards with bounded steering, so most of the square can never hold an area.
 *
 * The upload of the automaton computes, per trim r and step k, the bounding rectangle (x_lo, x_hi, y_lo, y_hi) — in the frame of a
 * root at the origin with yaw 0 in trim r — of the convex hull of every area the search can place at step k (all three area
 * variants, the transition masks of the steps; csrc/mpa_reach.hpp: mpa_reach_rects).  A segment is rotated into the root's frame with the
 * cos and sin of the root's yaw (pdmpc_sincos: the same bits on host and device) and is out of reach if its bounding box THERE lies
 * strictly outside the rectangle, widened by the relative margin above (the hull composes maneuvers in another order than the
 * search accumulates a pose) and by 2^-48 of the end points' distances from the root (the rounding of the rotation itself, which
 * only matters for coordinates near 2^64).  NaN: out; non-finite or beyond 2^64: in; it only errs towards "in". */
#define PDMPC_REACH_ROTATION 0x1p-48

/* the rectangle of a step, widened: box = (x_lo, x_hi, y_lo, y_hi) in the root's frame */
PDMPC_HD static inline void pdmpc_reach_rect_box(const double* rect, double root_x, double root_y, double* box) {
    const double ax = fabs(rect[0]) > fabs(rect[1]) ? fabs(rect[0]) : fabs(rect[1]);
    const double ay = fabs(rect[2]) > fabs(rect[3]) ? fabs(rect[2]) : fabs(rect[3]);
    const double m = PDMPC_REACH_MARGIN * (1.0 + fabs(root_x) + fabs(root_y) + (ax > ay ? ax : ay));
    box[0] = rect[0] - m;
    box[1] = rect[1] + m;
    box[2] = rect[2] - m;
    box[3] = rect[3] + m;
}

/* 1: the segment (x0, y0) - (x1, y1) is in reach of the step whose widened rectangle, in the frame of the root at (root_x, root_y)
 * with (cs, sn) = cos and sin of its yaw, is (x_lo, x_hi, y_lo, y_hi) */
PDMPC_HD static inline int pdmpc_reach_in_oriented(double x0, double y0, double x1, double y1, double root_x, double root_y, double cs, double sn, double x_lo, double x_hi, double y_lo,
                                                   double y_hi) {
    if (x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1) return 0;
    const int bounded = fabs(x0) <= PDMPC_REACH_FINITE && fabs(y0) <= PDMPC_REACH_FINITE && fabs(x1) <= PDMPC_REACH_FINITE && fabs(y1) <= PDMPC_REACH_FINITE;
    if (!bounded) return 1;
    const double dx0 = x0 - root_x, dy0 = y0 - root_y, dx1 = x1 - root_x, dy1 = y1 - root_y;
    const double u0 = cs * dx0 + sn * dy0, v0 = cs * dy0 - sn * dx0;
    const double u1 = cs * dx1 + sn * dy1, v1 = cs * dy1 - sn * dx1;
    const double slack = PDMPC_REACH_ROTATION * (fabs(dx0) + fabs(dy0) + fabs(dx1) + fabs(dy1));
    const double max_u = u0 > u1 ? u0 : u1, min_u = u0 < u1 ? u0 : u1;
    const double max_v = v0 > v1 ? v0 : v1, min_v = v0 < v1 ? v0 : v1;
    return !(max_u < x_lo - slack || min_u > x_hi + slack || max_v < y_lo - slack || min_v > y_hi + slack);
}

#endif
