// hdv.cpp — the host twin of the HDV traffic call (pdmpc_hdv_traffic; hdv_kernel.hip): closest lanelets, chains, the reachable lane
// of every chain and step, and the CAV/HDV adjacency (HighLevelController.update_hdv_traffic_info, HighLevelController.m:394-447, with
// the semantics of DESIGN.md §3.24).  Host code only.  Every decision and every vertex comes from the header functions the kernels
// compile too (include/pdmpc_hdv.h, include/pdmpc_geometry.h), so both give the same bits.
#include <cstring>
#include <string>

#include "hdv_drive_host.hpp"
#include "hdv_grouped_host.hpp"
#include "hdv_host.hpp"

#include "../../include/pdmpc_geometry.h"

extern "C" void pdmpc_set_last_error(const char* msg);  // api.cpp: the string pdmpc_last_error returns

extern "C" {

int pdmpc_hdv_lanelet_distances_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                                     const double* right_x, const double* right_y, double px, double py, double* distance) {
    HdvMapData map;
    const char* why = nullptr;
    if (!distance) return PDMPC_ERR_INVALID;
    if (const int rc = map.points(n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, &why)) return rc;
    const pdmpc_hdv_map M = map.view();
    for (int i = 0; i < n_lanelets; ++i) distance[i] = pdmpc_hdv_lanelet_distance(&M, i, px, py);
    return PDMPC_OK;
}

int pdmpc_hdv_check_map_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                             const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                             int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets) {
    HdvMapData map;
    const char* why = nullptr;
    int rc = map.points(n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, &why);
    if (!rc) rc = map.graph(succ_offset, succ_index, relationship, &why);
    if (!rc) rc = hdv_check_sets(n_trims, Hp, hdv_local_sets, &why);
    if (rc) pdmpc_set_last_error((std::string("pdmpc_hdv_check_map_host: ") + why).c_str());  // (the reason, as an upload reports it)
    return rc;
}

int pdmpc_hdv_grouped_layout_host(int32_t n_groups, const int32_t* hdv_offset, const int32_t* cav_offset, int32_t Hp, int32_t* closest_at, int32_t* list_at,
                                  int32_t* set_offset_at, int32_t* set_at, int64_t* adjacency_at) {
    return hdv_grouped_layout(n_groups, hdv_offset, cav_offset, Hp, closest_at, list_at, set_offset_at, set_at, adjacency_at);
}

int pdmpc_hdv_traffic_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                           const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                           int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets, int32_t n_hdv, const double* x, const double* y,
                           const double* cos_yaw, const double* sin_yaw, const int32_t* trim, const double* tile_dx, const double* tile_dy, int32_t n_cav,
                           const double* cav_x, const double* cav_y, const int32_t* cav_lanelet, const double* cav_tile_dx, const double* cav_tile_dy,
                           int32_t* closest_offset, int32_t* closest_index, int32_t capacity, int32_t* n_rows, int32_t* row_hdv, int32_t* set_offset, double* set_x,
                           double* set_y, uint8_t* set_flags, uint8_t* adjacency) {
    HdvMapData map;
    const char* why = nullptr;
    if (const int rc = map.points(n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, &why)) return rc;
    if (const int rc = map.graph(succ_offset, succ_index, relationship, &why)) return rc;
    if (const int rc = hdv_check_sets(n_trims, Hp, hdv_local_sets, &why)) return rc;
    if (const int rc = hdv_check_call(n_lanelets, n_trims, n_hdv, x, y, cos_yaw, sin_yaw, trim, tile_dx, tile_dy, n_cav, cav_x, cav_y, cav_lanelet, cav_tile_dx,
                                      cav_tile_dy, closest_offset, closest_index, capacity, n_rows, row_hdv, set_offset, adjacency, &why))
        return rc;
    const pdmpc_hdv_map M = map.view();
    *n_rows = -1;
    // (a) closest lanelets and (b) chains of every HDV
    std::vector<double> d((size_t)n_lanelets);
    std::vector<int32_t> chain_id((size_t)n_hdv * PDMPC_HDV_MAX_CHAINS), chain_succ((size_t)n_hdv * PDMPC_HDV_MAX_CHAINS), n_chains((size_t)n_hdv);
    closest_offset[0] = 0;
    for (int h = 0; h < n_hdv; ++h) {
        const double px = x[h] - tile_dx[h], py = y[h] - tile_dy[h];
        for (int i = 0; i < n_lanelets; ++i) d[i] = pdmpc_hdv_lanelet_distance(&M, i, px, py);
        int32_t* list = closest_index + closest_offset[h];
        int32_t local[PDMPC_HDV_MAX_CHAINS];
        const int n_list = pdmpc_hdv_closest_scan(d.data(), n_lanelets, local, PDMPC_HDV_MAX_CHAINS);
        if (n_list > PDMPC_HDV_MAX_CHAINS) return PDMPC_ERR_CAPACITY;
        std::memcpy(list, local, (size_t)n_list * sizeof(int32_t));
        closest_offset[h + 1] = closest_offset[h] + n_list;
        n_chains[h] = pdmpc_hdv_list_chains(&M, list, n_list, &chain_id[(size_t)h * PDMPC_HDV_MAX_CHAINS], &chain_succ[(size_t)h * PDMPC_HDV_MAX_CHAINS], PDMPC_HDV_MAX_CHAINS);
        if (n_chains[h] > PDMPC_HDV_MAX_CHAINS) return PDMPC_ERR_CAPACITY;
    }
    // (c) the reachable lane of every (row, step)
    int rows = 0;
    for (int h = 0; h < n_hdv; ++h)
        for (int c = 0; c < n_chains[h]; ++c) row_hdv[rows++] = h;
    std::vector<std::vector<double>> rx((size_t)rows * Hp), ry((size_t)rows * Hp);
    std::vector<uint8_t> fl((size_t)rows * Hp, 0);
    std::vector<double> raw_x((size_t)map.max_chain + 1), raw_y((size_t)map.max_chain + 1), lx((size_t)map.max_chain + 1), ly((size_t)map.max_chain + 1), kx, ky;
    bool too_big = false;
    for (int h = 0, row = 0; h < n_hdv; ++h)
        for (int c = 0; c < n_chains[h]; ++c, ++row) {
            const int id = chain_id[(size_t)h * PDMPC_HDV_MAX_CHAINS + c], succ = chain_succ[(size_t)h * PDMPC_HDV_MAX_CHAINS + c];
            const int nr = pdmpc_hdv_chain_vertices(&M, id, succ);
            for (int r = 0; r < nr; ++r) pdmpc_hdv_chain_vertex(&M, id, succ, tile_dx[h], tile_dy[h], r, &raw_x[r], &raw_y[r]);
            const int nl = pdmpc_lanelet_polygon_normalize(raw_x.data(), raw_y.data(), nr, lx.data(), ly.data());
            for (int k = 0; k < Hp; ++k) {
                const int p = (trim[h] - 1) * Hp + k;
                const int a = hdv_local_sets->offset[p], m = hdv_local_sets->offset[p + 1] - a;
                kx.resize((size_t)m);
                ky.resize((size_t)m);
                for (int r = 0; r < m; ++r) pdmpc_move_point(cos_yaw[h], sin_yaw[h], x[h], y[h], hdv_local_sets->x[a + r], hdv_local_sets->y[a + r], &kx[r], &ky[r]);
                const size_t o = (size_t)row * Hp + k;
                fl[o] = (uint8_t)pdmpc_bound_one_host(kx.data(), ky.data(), m, lx.data(), ly.data(), nl, rx[o], ry[o]);
                if (fl[o] & PDMPC_BOUND_RESTORED) {  // K ∩ L is empty: a polygon of 0 columns (HighLevelController.m:416-419), not K
                    rx[o].clear();
                    ry[o].clear();
                }
                if (rx[o].size() > (size_t)PDMPC_BOUNDED_MAX_COLS) too_big = true;
            }
        }
    // (d) adjacency
    for (int v = 0; v < n_cav; ++v)
        for (int h = 0; h < n_hdv; ++h) {
            int adjacent = 0;
            if (cav_tile_dx[v] == tile_dx[h] && cav_tile_dy[v] == tile_dy[h])
                adjacent = !pdmpc_hdv_is_behind(&M, cav_lanelet[v], cav_x[v], cav_y[v], closest_index + closest_offset[h], closest_offset[h + 1] - closest_offset[h], x[h],
                                                y[h], cos_yaw[h], sin_yaw[h]);
            adjacency[(size_t)v * n_hdv + h] = (uint8_t)adjacent;
        }
    *n_rows = rows;
    set_offset[0] = 0;
    for (size_t o = 0; o < rx.size(); ++o) set_offset[o + 1] = set_offset[o] + (int32_t)rx[o].size();
    if (too_big) return PDMPC_ERR_CAPACITY;
    const int32_t total = set_offset[rx.size()];
    if (capacity < total || (total && (!set_x || !set_y))) return PDMPC_ERR_CAPACITY;
    for (size_t o = 0; o < rx.size(); ++o) {
        std::memcpy(set_x + set_offset[o], rx[o].data(), rx[o].size() * sizeof(double));
        std::memcpy(set_y + set_offset[o], ry[o].data(), ry[o].size() * sizeof(double));
    }
    if (set_flags) std::memcpy(set_flags, fl.data(), fl.size());
    return PDMPC_OK;
}

// ---- the driver model (include/pdmpc_hdv.h; hdv_drive_host.hpp)
namespace {
// the map of a driver call, and the routes against it
int drive_map(const char* who, HdvMapData& map, int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
              const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship, int32_t n_hdv,
              const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed) {
    const char* why = nullptr;
    std::string text;
    int rc = map.points(n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, &why);
    if (!rc) rc = map.graph(succ_offset, succ_index, relationship, &why);
    if (rc) text = why;
    if (!rc && (!route_offset || route_offset[0] != 0)) rc = PDMPC_ERR_INVALID, text = "route offsets that do not start at 0";
    if (!rc) rc = hdv_check_routes(map, n_hdv, route_offset, route_lanelet, closed, &text);
    if (rc) pdmpc_set_last_error((std::string(who) + ": " + text).c_str());
    return rc;
}
}  // namespace

int pdmpc_hdv_route_check_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                               const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                               int32_t n_hdv, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed) {
    HdvMapData map;
    return drive_map("pdmpc_hdv_route_check_host", map, n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, succ_offset, succ_index, relationship, n_hdv,
                     route_offset, route_lanelet, closed);
}

int pdmpc_hdv_place_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y, const double* right_x,
                         const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship, int32_t n_hdv,
                         const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const double* start_distance, const double* tile_dx,
                         const double* tile_dy, int32_t* state_seg, double* state_u, double* x, double* y, double* cos_yaw, double* sin_yaw) {
    const char* who = "pdmpc_hdv_place_host";
    HdvMapData map;
    if (const int rc = drive_map(who, map, n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, succ_offset, succ_index, relationship, n_hdv, route_offset,
                                 route_lanelet, closed))
        return rc;
    if (n_hdv && (!start_distance || !tile_dx || !tile_dy || !state_seg || !state_u || !x || !y || !cos_yaw || !sin_yaw)) {
        pdmpc_set_last_error((std::string(who) + ": null argument").c_str());
        return PDMPC_ERR_INVALID;
    }
    const pdmpc_hdv_map M = map.view();
    for (int h = 0; h < n_hdv; ++h) {
        const pdmpc_hdv_route R = hdv_route(route_offset, route_lanelet, closed, h);
        pdmpc_hdv_drive_state S;
        std::string why;
        if (const int rc = hdv_place(M, R, start_distance[h], &S, &why)) {
            pdmpc_set_last_error((std::string(who) + ": HDV " + std::to_string(h) + ": " + why).c_str());
            return rc;
        }
        state_seg[h] = S.r;
        state_seg[n_hdv + h] = S.j;
        state_u[h] = S.u;
        pdmpc_hdv_state_pose(&M, &R, &S, tile_dx[h], tile_dy[h], &x[h], &y[h], &cos_yaw[h], &sin_yaw[h]);
    }
    return PDMPC_OK;
}

int pdmpc_hdv_drive_host(int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y, const double* right_x,
                         const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship, int32_t n_hdv,
                         const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_seg, const double* state_u,
                         const double* tile_dx, const double* tile_dy, const double* v_des, int32_t n_cav, const double* cav_x, const double* cav_y,
                         const double* cav_tile_dx, const double* cav_tile_dy, const double* parameters, double dt, int32_t* new_seg, double* new_u, double* x, double* y,
                         double* cos_yaw, double* sin_yaw, double* speed, double* gap) {
    const char* who = "pdmpc_hdv_drive_host";
    HdvMapData map;
    if (const int rc = drive_map(who, map, n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, succ_offset, succ_index, relationship, n_hdv, route_offset,
                                 route_lanelet, closed))
        return rc;
    std::string why = "null argument";
    int rc = (n_hdv && (!tile_dx || !tile_dy || !new_seg || !new_u || !x || !y || !cos_yaw || !sin_yaw || !speed || !gap)) || n_cav < 0 ||
                     (n_cav && (!cav_x || !cav_y || !cav_tile_dx || !cav_tile_dy))
                 ? PDMPC_ERR_INVALID
                 : PDMPC_OK;
    if (!rc) rc = hdv_check_states(map, n_hdv, route_offset, route_lanelet, closed, state_seg, state_seg ? state_seg + n_hdv : nullptr, state_u, &why);
    if (!rc) rc = hdv_check_drive(parameters, dt, n_hdv, v_des, &why);
    if (rc) {
        pdmpc_set_last_error((std::string(who) + ": " + why).c_str());
        return rc;
    }
    hdv_drive_member(map.view(), n_hdv, route_offset, route_lanelet, closed, state_seg, state_u, tile_dx, tile_dy, v_des, n_cav, cav_x, cav_y, cav_tile_dx, cav_tile_dy,
                     parameters, dt, new_seg, new_u, x, y, cos_yaw, sin_yaw, speed, gap);
    return PDMPC_OK;
}

}  // extern "C"
