// hdv_host.hpp — what the two sides of the HDV traffic call share on the host (hdv.cpp: the host twin; step_prep.cpp: the device call):
// the map as it is taken over and checked once, the checks of a call's arguments, and the limits.  Host only, no HIP header.
// The device calls' own host side -- workspace layout, check, zero, stage, arguments, scatter -- is hdv_call_host.hpp.  DESIGN.md §3.24.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pdmpc.h"
#include "../../include/pdmpc_hdv.h"

// The map of pdmpc_upload_hdv_map / pdmpc_hdv_traffic_host, checked and with its centre line: `pts` holds lx, ly, rx, ry, cx, cy, n_pts each
struct HdvMapData {
    int32_t n_lanelets = 0, n_pts = 0, n_succ = 0;
    std::vector<int32_t> pt_off, succ_off, succ_idx;
    std::vector<double> pts;
    std::vector<uint8_t> rel;
    int max_chain = 0;  // most vertices of a raw chain polygon

    // Both return PDMPC_OK, or PDMPC_ERR_INVALID / PDMPC_ERR_CAPACITY with *why set.  The lanelets' points and their centre line ...
    int points(int32_t n, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y, const double* right_x, const double* right_y,
               const char** why) {
        *why = "bad argument";
        if (n < 1 || !left_offset || !right_offset || !left_x || !left_y || !right_x || !right_y) return PDMPC_ERR_INVALID;
        if (n > PDMPC_HDV_MAX_LANELETS) {
            *why = "more than 1024 lanelets";
            return PDMPC_ERR_CAPACITY;
        }
        n_lanelets = n;
        pt_off.assign((size_t)n + 1, 0);
        for (int i = 0; i < n; ++i) {
            const int nl = left_offset[i + 1] - left_offset[i], nr = right_offset[i + 1] - right_offset[i];
            *why = "a lanelet needs as many left as right points, and at least one";
            if (nl < 1 || nl != nr) return PDMPC_ERR_INVALID;
            pt_off[i + 1] = pt_off[i] + nl;
        }
        n_pts = pt_off[n];
        pts.resize((size_t)6 * n_pts);
        double *lx = pts.data(), *ly = lx + n_pts, *rx = ly + n_pts, *ry = rx + n_pts, *cx = ry + n_pts, *cy = cx + n_pts;
        for (int i = 0; i < n; ++i)
            for (int q = 0; q < pt_off[i + 1] - pt_off[i]; ++q) {
                const int o = pt_off[i] + q, l = left_offset[i] + q, r = right_offset[i] + q;
                lx[o] = left_x[l];
                ly[o] = left_y[l];
                rx[o] = right_x[r];
                ry[o] = right_y[r];
                cx[o] = 0.5 * (lx[o] + rx[o]);  // RoadDataCommonRoad.m:57-58
                cy[o] = 0.5 * (ly[o] + ry[o]);
            }
        return PDMPC_OK;
    }
    // ... and, after them, the successor lists and the relationship table
    int graph(const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship, const char** why) {
        const int n = n_lanelets;
        *why = "bad successor lists";
        if (!succ_offset || !relationship || succ_offset[0] != 0) return PDMPC_ERR_INVALID;
        for (int i = 0; i < n; ++i)
            if (succ_offset[i + 1] < succ_offset[i]) return PDMPC_ERR_INVALID;
        n_succ = succ_offset[n];
        if (n_succ && !succ_index) return PDMPC_ERR_INVALID;
        succ_off.assign(succ_offset, succ_offset + n + 1);
        succ_idx.assign(succ_index, succ_index + n_succ);
        max_chain = 0;
        for (int i = 0; i < n; ++i) {
            int longest = 0;
            for (int s = succ_off[i]; s < succ_off[i + 1]; ++s) {
                const int id = succ_idx[s];
                *why = "a successor id out of range";
                if (id < 1 || id > n) return PDMPC_ERR_INVALID;
                if (pt_off[id] - pt_off[id - 1] > longest) longest = pt_off[id] - pt_off[id - 1];
            }
            const int c = 2 * (pt_off[i + 1] - pt_off[i] + longest);
            if (c > max_chain) max_chain = c;
        }
        if (max_chain > PDMPC_LANELET_POLY_MAX_COLS) {
            *why = "a lanelet and its successor have more than PDMPC_LANELET_POLY_MAX_COLS boundary points";
            return PDMPC_ERR_CAPACITY;
        }
        rel.assign(relationship, relationship + (size_t)n * n);
        return PDMPC_OK;
    }
    // the view over a copy of these arrays with the same sizes (the device table), or over these arrays themselves
    pdmpc_hdv_map view(const int32_t* off, const double* p, const int32_t* so, const int32_t* si, const uint8_t* r) const {
        pdmpc_hdv_map M;
        M.n_lanelets = n_lanelets;
        M.pt_off = off;
        M.lx = p;
        M.ly = p + n_pts;
        M.rx = p + 2 * (size_t)n_pts;
        M.ry = p + 3 * (size_t)n_pts;
        M.cx = p + 4 * (size_t)n_pts;
        M.cy = p + 5 * (size_t)n_pts;
        M.succ_off = so;
        M.succ_idx = si;
        M.rel = r;
        return M;
    }
    pdmpc_hdv_map view() const { return view(pt_off.data(), pts.data(), succ_off.data(), succ_idx.data(), rel.data()); }
};

// the HDV automaton's local sets: n_trims * Hp polygons of 1 .. PDMPC_REACHABLE_MAX_COLS vertices
inline int hdv_check_sets(int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* sets, const char** why) {
    *why = "bad local sets";
    if (n_trims < 1 || Hp < 1 || Hp > PDMPC_HP_MAX || !sets || !sets->offset || sets->n_polygons != n_trims * Hp || !sets->x || !sets->y) return PDMPC_ERR_INVALID;
    for (int p = 0; p < sets->n_polygons; ++p) {
        const int m = sets->offset[p + 1] - sets->offset[p];
        *why = "an empty local set";
        if (m < 1) return PDMPC_ERR_INVALID;
        *why = "a local set has more than PDMPC_REACHABLE_MAX_COLS vertices";
        if (m > PDMPC_REACHABLE_MAX_COLS) return PDMPC_ERR_CAPACITY;
    }
    return PDMPC_OK;
}

// The host's copy of what a map slot of a handle holds (pdmpc_upload_hdv_map_slot): the map, and the hulls with their offsets from 0
// (x of every vertex, then y)
struct HdvSlotData {
    HdvMapData map;
    int trims = 0, Hp = 0, local_tot = 0;
    std::vector<int32_t> local_off;
    std::vector<double> local_xy;

    void keep_sets(int32_t n_trims, int32_t Hp_, const pdmpc_polygon_set* sets) {  // (after hdv_check_sets)
        const int n_polygons = n_trims * Hp_, p0 = sets->offset[0];
        trims = n_trims;
        Hp = Hp_;
        local_tot = sets->offset[n_polygons] - p0;
        local_off.resize((size_t)n_polygons + 1);
        for (int p = 0; p <= n_polygons; ++p) local_off[(size_t)p] = sets->offset[p] - p0;
        local_xy.assign(sets->x + p0, sets->x + p0 + local_tot);
        local_xy.insert(local_xy.end(), sets->y + p0, sets->y + p0 + local_tot);
    }
    // exactly this map and these hulls, as an upload takes them: every size, offset, point, successor, relationship and vertex compared
    // with the copy, the doubles byte for byte (no hash: equal means equal)
    bool holds(int32_t n, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y, const double* right_x, const double* right_y,
               const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship, int32_t n_trims, int32_t Hp_, const pdmpc_polygon_set* sets) const {
        if (n != map.n_lanelets || n < 1 || !left_offset || !right_offset || !left_x || !left_y || !right_x || !right_y || !succ_offset || !relationship) return false;
        if (n_trims != trims || Hp_ != Hp || !sets || !sets->offset || !sets->x || !sets->y || sets->n_polygons != n_trims * Hp_) return false;
        const double *lx = map.pts.data(), *ly = lx + map.n_pts, *rx = ly + map.n_pts, *ry = rx + map.n_pts;
        for (int i = 0; i < n; ++i) {
            const int a = map.pt_off[(size_t)i], cnt = map.pt_off[(size_t)i + 1] - a;
            if (left_offset[i + 1] - left_offset[i] != cnt || right_offset[i + 1] - right_offset[i] != cnt) return false;
            const size_t bytes = (size_t)cnt * sizeof(double);
            if (std::memcmp(lx + a, left_x + left_offset[i], bytes) || std::memcmp(ly + a, left_y + left_offset[i], bytes) ||
                std::memcmp(rx + a, right_x + right_offset[i], bytes) || std::memcmp(ry + a, right_y + right_offset[i], bytes))
                return false;
        }
        if (std::memcmp(map.succ_off.data(), succ_offset, ((size_t)n + 1) * sizeof(int32_t))) return false;
        if (map.n_succ && (!succ_index || std::memcmp(map.succ_idx.data(), succ_index, (size_t)map.n_succ * sizeof(int32_t)))) return false;
        if (std::memcmp(map.rel.data(), relationship, (size_t)n * n)) return false;
        const int n_polygons = n_trims * Hp_, p0 = sets->offset[0];
        for (int p = 0; p <= n_polygons; ++p)
            if (sets->offset[p] - p0 != local_off[(size_t)p]) return false;
        const size_t bytes = (size_t)local_tot * sizeof(double);
        return !std::memcmp(local_xy.data(), sets->x + p0, bytes) && !std::memcmp(local_xy.data() + local_tot, sets->y + p0, bytes);
    }
};

// the arguments of one traffic call against a map of n_lanelets lanelets and a table of n_trims trims
inline int hdv_check_call(int32_t n_lanelets, int32_t n_trims, int32_t n_hdv, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw,
                          const int32_t* trim, const double* tile_dx, const double* tile_dy, int32_t n_cav, const double* cav_x, const double* cav_y,
                          const int32_t* cav_lanelet, const double* cav_tile_dx, const double* cav_tile_dy, const int32_t* closest_offset, const int32_t* closest_index,
                          int32_t capacity, const int32_t* n_rows, const int32_t* row_hdv, const int32_t* set_offset, const uint8_t* adjacency, const char** why) {
    *why = "bad argument";
    if (n_hdv < 0 || n_cav < 0 || capacity < 0 || !closest_offset || !n_rows || !set_offset) return PDMPC_ERR_INVALID;
    if (n_hdv && (!x || !y || !cos_yaw || !sin_yaw || !trim || !tile_dx || !tile_dy || !closest_index || !row_hdv)) return PDMPC_ERR_INVALID;
    if (n_cav && (!cav_x || !cav_y || !cav_lanelet || !cav_tile_dx || !cav_tile_dy)) return PDMPC_ERR_INVALID;
    if (n_hdv && n_cav && !adjacency) return PDMPC_ERR_INVALID;
    *why = "more than PDMPC_HDV_MAX_VEHICLES HDVs or PDMPC_HDV_MAX_CAVS CAVs";
    if (n_hdv > PDMPC_HDV_MAX_VEHICLES || n_cav > PDMPC_HDV_MAX_CAVS) return PDMPC_ERR_CAPACITY;
    *why = "trim out of range";
    for (int h = 0; h < n_hdv; ++h)
        if (trim[h] < 1 || trim[h] > n_trims) return PDMPC_ERR_INVALID;
    *why = "a CAV's lanelet id out of range";
    for (int v = 0; v < n_cav; ++v)
        if (cav_lanelet[v] < 1 || cav_lanelet[v] > n_lanelets) return PDMPC_ERR_INVALID;
    return PDMPC_OK;
}

// reachable_sets.cpp: the bounded set of the clockwise convex K (open, m vertices) and the normalized L, closed, into (ox, oy) -> PDMPC_BOUND_*
unsigned pdmpc_bound_one_host(const double* kx, const double* ky, int m, const double* lx, const double* ly, int nl, std::vector<double>& ox, std::vector<double>& oy);
