// hdv_drive_host.hpp — the host side of the HDV driver model (include/pdmpc_hdv.h: "the driver model"): the checks of
// routes, states and parameters that the host twin (hdv.cpp) and the device calls' check stage (hdv_call_host.hpp) share, the placement of an HDV at a
// distance along its route, and one step of all HDVs of a member on the host -- the body of pdmpc_hdv_drive_host, which the kernel
// (hdv_kernel.hip: pdmpc_hdv_drive_kernel) restates with the same header functions.  Host only, no HIP header
// (tests/hdv_drive_checks.cpp runs this file under the sanitizers).
#pragma once
#include <cmath>
#include <string>

#include "hdv_host.hpp"

// route h of a call's routes (route_offset [n_hdv + 1] from 0, route_lanelet, closed [n_hdv])
inline pdmpc_hdv_route hdv_route(const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, int h) {
    return pdmpc_hdv_route{route_lanelet + route_offset[h], route_offset[h + 1] - route_offset[h], closed[h] ? 1 : 0};
}

// The routes of n_hdv HDVs (route h: route_lanelet[route_offset[h] .. route_offset[h + 1])) against the map: 1 .. PDMPC_HDV_ROUTE_MAX ids in range, each a successor of the one before it, the first of
// the last on a closed route, and a segment of positive length to stand on.  *why names the HDV and the position.
inline int hdv_check_routes(const HdvMapData& map, int32_t n_hdv, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, std::string* why) {
    *why = "bad route arguments";
    if (n_hdv < 0 || !route_offset || (n_hdv && (!route_lanelet || !closed))) return PDMPC_ERR_INVALID;
    const pdmpc_hdv_map M = map.view();
    for (int h = 0; h < n_hdv; ++h) {
        const auto who = [h]() { return "HDV " + std::to_string(h) + ": "; };  // (a refusal's text is put together only when there is one)
        const int n = route_offset[h + 1] - route_offset[h];
        if (n < 1 || n > PDMPC_HDV_ROUTE_MAX) {
            *why = who() + "a route of " + std::to_string(n) + " lanelets (1 .. PDMPC_HDV_ROUTE_MAX)";
            return PDMPC_ERR_INVALID;
        }
        const int32_t* id = route_lanelet + route_offset[h];
        for (int r = 0; r < n; ++r)
            if (id[r] < 1 || id[r] > map.n_lanelets) {
                *why = who() + "route position " + std::to_string(r) + ": lanelet id " + std::to_string(id[r]) + " out of range";
                return PDMPC_ERR_INVALID;
            }
        for (int r = 0; r < n; ++r) {
            if (r == n - 1 && !closed[h]) break;
            const int from = id[r], to = id[r + 1 < n ? r + 1 : 0];
            bool found = false;
            for (int s = map.succ_off[(size_t)from - 1]; s < map.succ_off[(size_t)from]; ++s) found = found || map.succ_idx[(size_t)s] == to;
            if (!found) {
                *why = who() + "route position " + std::to_string(r + 1 < n ? r + 1 : 0) + ": lanelet " + std::to_string(to) + " is no successor of lanelet " +
                       std::to_string(from) + (r + 1 < n ? "" : " (the route is flagged closed)");
                return PDMPC_ERR_INVALID;
            }
        }
        const pdmpc_hdv_route R = hdv_route(route_offset, route_lanelet, closed, h);
        bool stands = false;
        for (int r = 0; r < n && !stands; ++r)
            for (int j = 0; j < pdmpc_hdv_route_segments(&M, &R, r) && !stands; ++j) {
                double ax, ay, dx, dy;
                stands = pdmpc_hdv_route_segment(&M, &R, r, j, &ax, &ay, &dx, &dy) > 0.0;
            }
        if (!stands) {
            *why = who() + "a route without a segment of positive length";
            return PDMPC_ERR_INVALID;
        }
    }
    return PDMPC_OK;
}

// the states (state_r, state_j, state_u) of checked routes: a segment that exists and has a positive length, 0 <= u <= that length
inline int hdv_check_states(const HdvMapData& map, int32_t n_hdv, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_r,
                            const int32_t* state_j, const double* state_u, std::string* why) {
    *why = "null state";
    if (n_hdv && (!state_r || !state_j || !state_u)) return PDMPC_ERR_INVALID;
    const pdmpc_hdv_map M = map.view();
    for (int h = 0; h < n_hdv; ++h) {
        const pdmpc_hdv_route R = hdv_route(route_offset, route_lanelet, closed, h);
        const int r = state_r[h], j = state_j[h];
        bool on = r >= 0 && r < R.n && j >= 0 && j < pdmpc_hdv_route_segments(&M, &R, r) && state_u[h] >= 0.0;
        if (on) {  // ... of positive length, and u within it
            double ax, ay, dx, dy;
            const double len = pdmpc_hdv_route_segment(&M, &R, r, j, &ax, &ay, &dx, &dy);
            on = len > 0.0 && state_u[h] <= len;
        }
        if (!on) {
            *why = "HDV " + std::to_string(h) + ": a state that is not on its route";
            return PDMPC_ERR_INVALID;
        }
    }
    return PDMPC_OK;
}

// parameters[4] = look_ahead, gap_min, headway, lateral, all positive and finite, headway >= dt > 0 (then an HDV closes at most
// gap - gap_min per step); v_des[n_hdv] >= 0 and finite
inline int hdv_check_drive(const double* parameters, double dt, int32_t n_hdv, const double* v_des, std::string* why) {
    *why = "null parameters";
    if (!parameters || (n_hdv && !v_des)) return PDMPC_ERR_INVALID;
    *why = "look_ahead, gap_min, headway, lateral and dt must be positive and finite";
    for (int q = 0; q < 4; ++q)
        if (!(parameters[q] > 0.0) || !std::isfinite(parameters[q])) return PDMPC_ERR_INVALID;
    if (!(dt > 0.0) || !std::isfinite(dt)) return PDMPC_ERR_INVALID;
    *why = "headway < dt: an HDV could close more than gap - gap_min in one step";
    if (parameters[2] < dt) return PDMPC_ERR_INVALID;
    *why = "a desired speed that is negative or not finite";
    for (int h = 0; h < n_hdv; ++h)
        if (!(v_des[h] >= 0.0) || !std::isfinite(v_des[h])) return PDMPC_ERR_INVALID;
    return PDMPC_OK;
}

// The state `distance` metres from the start of a checked route: the first segment of positive length, then the walk of the step
inline int hdv_place(const pdmpc_hdv_map& M, const pdmpc_hdv_route& R, double distance, pdmpc_hdv_drive_state* S, std::string* why) {
    *why = "a start distance that is negative or not finite";
    if (!(distance >= 0.0) || !std::isfinite(distance)) return PDMPC_ERR_INVALID;
    int r = 0, j = -1;
    double ax, ay, dx, dy;
    do {
        *why = "a route without a segment of positive length";
        if (!pdmpc_hdv_route_next(&M, &R, &r, &j)) return PDMPC_ERR_INVALID;
    } while (!(pdmpc_hdv_route_segment(&M, &R, r, j, &ax, &ay, &dx, &dy) > 0.0));
    *S = pdmpc_hdv_drive_state{r, j, 0.0};
    *why = "a start distance at or beyond the end of an open route";
    if (pdmpc_hdv_walk(&M, &R, S, distance)) return PDMPC_ERR_INVALID;
    return PDMPC_OK;
}

// One step of the n_hdv HDVs of one member (checked arguments): the gap of each to the CAVs and to the other HDVs at their poses BEFORE
// the step, on its own tile only; then all move at once.  new_seg / new_u may not alias the old state.
inline void hdv_drive_member(const pdmpc_hdv_map& M, int32_t n_hdv, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_seg,
                             const double* state_u, const double* tile_dx, const double* tile_dy, const double* v_des, int32_t n_cav, const double* cav_x,
                             const double* cav_y, const double* cav_tile_dx, const double* cav_tile_dy, const double* parameters, double dt, int32_t* new_seg, double* new_u,
                             double* x, double* y, double* cos_yaw, double* sin_yaw, double* speed, double* gap) {
    std::vector<double> ox((size_t)n_hdv), oy((size_t)n_hdv);
    for (int q = 0; q < n_hdv; ++q) {
        const pdmpc_hdv_route R = hdv_route(route_offset, route_lanelet, closed, q);
        const pdmpc_hdv_drive_state S{state_seg[q], state_seg[n_hdv + q], state_u[q]};
        double c, s;
        pdmpc_hdv_state_pose(&M, &R, &S, tile_dx[q], tile_dy[q], &ox[(size_t)q], &oy[(size_t)q], &c, &s);
    }
    pdmpc_hdv_window W;
    for (int h = 0; h < n_hdv; ++h) {
        const pdmpc_hdv_route R = hdv_route(route_offset, route_lanelet, closed, h);
        pdmpc_hdv_drive_state S{state_seg[h], state_seg[n_hdv + h], state_u[h]};
        const int nw = pdmpc_hdv_build_window(&M, &R, &S, parameters[0], &W);
        double best = (double)INFINITY;
        for (int o = 0; o < n_cav + n_hdv; ++o) {
            const bool cav = o < n_cav;
            const int q = o - n_cav;
            if (!cav && q == h) continue;
            if (!((cav ? cav_tile_dx[o] : tile_dx[q]) == tile_dx[h] && (cav ? cav_tile_dy[o] : tile_dy[q]) == tile_dy[h])) continue;
            const double px = (cav ? cav_x[o] : ox[(size_t)q]) - tile_dx[h], py = (cav ? cav_y[o] : oy[(size_t)q]) - tile_dy[h];
            for (int w = 0; w < nw; ++w) {
                const double ahead = pdmpc_hdv_gap_item(&W, w, S.u, px, py, parameters[3]);
                if (ahead < best) best = ahead;
            }
        }
        gap[h] = best;
        speed[h] = pdmpc_hdv_move(&M, &R, &S, best, v_des[h], parameters, dt);
        new_seg[h] = S.r;
        new_seg[n_hdv + h] = S.j;
        new_u[h] = S.u;
        pdmpc_hdv_state_pose(&M, &R, &S, tile_dx[h], tile_dy[h], &x[h], &y[h], &cos_yaw[h], &sin_yaw[h]);
    }
}
