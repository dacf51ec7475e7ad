/* pdmpc_hdv.h — human-driven vehicles (HDVs): closest lanelets, lanelet chains and CAV/HDV adjacency, shared by host and device.
 *
 * HighLevelController.update_hdv_traffic_info (HighLevelController.m:394-447) with map_position_to_closest_lanelets.m:1-25,
 * ManualVehicle.compute_reachable_lane (scenarios/ManualVehicle.m:30-49) and is_hdv_behind.m:13-92, with the semantics DESIGN.md §3.24
 * writes down.  Every function is one definition for the host twin (csrc/hdv.cpp) and the kernels (csrc/hdv_kernel.hip), and,
 * operation by operation, p-dmpc_amd/pdmpc/hdv.py; all are compiled with -ffp-contract=off, so the three give the same bits.  The
 * reachable lane itself (K ∩ chain polygon) is the bounding rule of pdmpc_geometry.h.
 */
#ifndef PDMPC_HDV_H
#define PDMPC_HDV_H

#include <math.h>
#include <stdint.h>

#include "pdmpc.h"      /* PDMPC_HDV_MAX_CHAINS */
#include "pdmpc_math.h" /* PDMPC_HD */

#define PDMPC_HDV_MAX_LANELETS 1024 /* lanelets of a map: the device keeps one distance per lanelet in LDS */
#define PDMPC_HDV_MAX_VEHICLES 64   /* HDVs of one call: each has PDMPC_HDV_MAX_CHAINS * Hp slots of PDMPC_BOUNDED_MAX_COLS vertices on the device (256 KB x Hp: 256 MB at the limit and Hp 16) */
#define PDMPC_HDV_MAX_CAVS (1 << 20) /* CAVs of one call (the adjacency is indexed in 32 bits) */
#define PDMPC_HDV_CLOSEST_BAND 0.1   /* map_position_to_closest_lanelets.m:4: added to a DISTANCE (the variable is called "squared") */
#define PDMPC_HDV_POINT_TOLERANCE 1e-6 /* is_hdv_behind.m:6 */

/* LaneletRelationshipType.m:5-10, 0 = no relationship (an empty cell) */
enum { PDMPC_LANELET_NONE = 0, PDMPC_LANELET_LONGITUDINAL = 1, PDMPC_LANELET_SIDE = 2, PDMPC_LANELET_MERGING = 3, PDMPC_LANELET_FORKING = 4, PDMPC_LANELET_CROSSING = 5 };

/* The map as both sides read it: lanelet i (0-based; id i + 1) has the points pt_off[i] .. pt_off[i + 1] - 1 of its left and right
 * bound and of its centre line (0.5 * (left + right), computed once where the map is taken over). */
typedef struct pdmpc_hdv_map {
    int32_t n_lanelets;
    const int32_t* pt_off;              /* [n_lanelets + 1] */
    const double *lx, *ly, *rx, *ry;    /* left and right bound */
    const double *cx, *cy;              /* centre line */
    const int32_t *succ_off, *succ_idx; /* successors of lanelet i: succ_idx[succ_off[i] .. succ_off[i + 1]), 1-based ids, the map's order */
    const uint8_t* rel;                 /* [n_lanelets x n_lanelets] PDMPC_LANELET_*, read at (min id, max id) */
} pdmpc_hdv_map;

/* d_i of map_position_to_closest_lanelets.m:8-15: the smallest distance from (px, py) to a centre point of lanelet i */
PDMPC_HD static inline double pdmpc_hdv_lanelet_distance(const pdmpc_hdv_map* M, int i, double px, double py) {
    double best = 0.0;
    const int a = M->pt_off[i], b = M->pt_off[i + 1];
    for (int q = a; q < b; ++q) {
        const double ex = M->cx[q] - px, ey = M->cy[q] - py;
        const double d = sqrt(ex * ex + ey * ey);
        if (q == a || d < best) best = d;
    }
    return best;
}

/* The order-dependent scan of map_position_to_closest_lanelets.m:17-22 over d[0 .. n): a smaller distance starts the list anew, one
 * within the band of the best SO FAR is appended.  Writes at most cap ids (1-based, ascending) and returns the list's length. */
PDMPC_HD static inline int pdmpc_hdv_closest_scan(const double* d, int n, int32_t* list, int cap) {
    double best = (double)INFINITY;
    int count = 0;
    for (int i = 0; i < n; ++i) {
        if (d[i] < best) {
            best = d[i];
            count = 0;
            if (cap > 0) list[0] = i + 1;
            count = 1;
        } else if (d[i] <= best + PDMPC_HDV_CLOSEST_BAND) {
            if (count < cap) list[count] = i + 1;
            ++count;
        }
    }
    return count;
}

/* The chains of a list of closest lanelets: (id, successor) for every successor of every id, in list order and the map's successor order;
 * (id, 0) for a lanelet without successor.  Writes at most cap chains and returns their number. */
PDMPC_HD static inline int pdmpc_hdv_list_chains(const pdmpc_hdv_map* M, const int32_t* list, int n_list, int32_t* chain_id, int32_t* chain_succ, int cap) {
    int count = 0;
    for (int q = 0; q < n_list; ++q) {
        const int id = list[q];
        const int a = M->succ_off[id - 1], ns = M->succ_off[id] - a;
        for (int s = 0; s < (ns ? ns : 1); ++s) {
            if (count < cap) {
                chain_id[count] = id;
                chain_succ[count] = ns ? M->succ_idx[a + s] : 0;
            }
            ++count;
        }
    }
    return count;
}

/* Vertices of the raw chain polygon C(id, succ): left(id) ++ left(succ), then reversed(right(id) ++ right(succ)) (succ = 0: id alone) */
PDMPC_HD static inline int pdmpc_hdv_chain_vertices(const pdmpc_hdv_map* M, int id, int succ) {
    const int n1 = M->pt_off[id] - M->pt_off[id - 1];
    const int n2 = succ ? M->pt_off[succ] - M->pt_off[succ - 1] : 0;
    return 2 * (n1 + n2);
}
/* ... and its vertex r, moved by the tile offset (dx, dy) */
PDMPC_HD static inline void pdmpc_hdv_chain_vertex(const pdmpc_hdv_map* M, int id, int succ, double dx, double dy, int r, double* x, double* y) {
    const int a1 = M->pt_off[id - 1], n1 = M->pt_off[id] - a1;
    const int a2 = succ ? M->pt_off[succ - 1] : 0, n2 = succ ? M->pt_off[succ] - a2 : 0;
    const int n = n1 + n2;
    if (r < n) {
        const int q = r < n1 ? a1 + r : a2 + (r - n1);
        *x = M->lx[q] + dx;
        *y = M->ly[q] + dy;
    } else {
        const int j = 2 * n - 1 - r;
        const int q = j < n1 ? a1 + j : a2 + (j - n1);
        *x = M->rx[q] + dx;
        *y = M->ry[q] + dy;
    }
}

/* norm(a - b) > tolerance of is_hdv_behind.m:37-52 */
PDMPC_HD static inline int pdmpc_hdv_points_differ(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return sqrt(dx * dx + dy * dy) > PDMPC_HDV_POINT_TOLERANCE;
}

/* is_hdv_behind.m:13-92 for a CAV on lanelet id_cav at (cav_x, cav_y) and an HDV with the closest lanelets list[0 .. n_list) at
 * (hx, hy), hc / hs = cos / sin of its yaw: 1 if the HDV is on a predecessor lanelet of the CAV's (a longitudinal pair whose end and
 * start points meet, straight or diagonally), or on the same or a merging / forking lanelet and behind the CAV along its own heading.
 * The reference's assert :64 is dropped: no predecessor found means "not on a predecessor lanelet". */
PDMPC_HD static inline int pdmpc_hdv_is_behind(const pdmpc_hdv_map* M, int id_cav, double cav_x, double cav_y, const int32_t* list, int n_list, double hx, double hy,
                                               double hc, double hs) {
    const int n = M->n_lanelets;
    int on_predecessor = 0, on_same = 0, on_overlapping = 0;
    const int sc = M->pt_off[id_cav - 1]; /* the CAV lanelet's first point */
    for (int q = 0; q < n_list; ++q) {
        const int id_hdv = list[q];
        if (id_hdv == id_cav) on_same = 1;
        const int lo = id_cav < id_hdv ? id_cav : id_hdv, hi = id_cav < id_hdv ? id_hdv : id_cav;
        const int type = M->rel[(size_t)(lo - 1) * n + (hi - 1)];
        if (type == PDMPC_LANELET_NONE) continue;
        if (type == PDMPC_LANELET_MERGING || type == PDMPC_LANELET_FORKING) {
            on_overlapping = 1;
            continue;
        }
        if (type != PDMPC_LANELET_LONGITUDINAL) continue;
        const int eh = M->pt_off[id_hdv] - 1; /* the HDV lanelet's last point */
        if (pdmpc_hdv_points_differ(M->cx[sc], M->cy[sc], M->cx[eh], M->cy[eh]) && pdmpc_hdv_points_differ(M->lx[sc], M->ly[sc], M->rx[eh], M->ry[eh]) &&
            pdmpc_hdv_points_differ(M->rx[sc], M->ry[sc], M->lx[eh], M->ly[eh]))
            continue;
        on_predecessor = 1;
    }
    if (on_predecessor) return 1;
    if (on_same || on_overlapping) {
        const double vx = hx - cav_x, vy = hy - cav_y;
        const double scalar = hc * vx + hs * vy;
        if (scalar < 0.0) return 1;
    }
    return 0;
}

#endif /* PDMPC_HDV_H */
