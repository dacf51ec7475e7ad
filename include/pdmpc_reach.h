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
 * One definition for the kernel's list builder (csrc/bulk_search.hpp), the arrival rule (bk_incorporate_body) and the host twin
 * (pdmpc_reach_lists_host, csrc/api.cpp); all are compiled with -ffp-contract=off, so they give the same bits.
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

#endif
