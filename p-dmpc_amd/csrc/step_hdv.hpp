// step_hdv.hpp — human-driven vehicles on narrow state (step_controller.cpp, stage 3 of 9): a member's map as the
// arguments every entry point takes it with, the ONE capacity retry of the step preparation, what the pdmpc_controller_set_hdv_* entry
// points do to a member's HdvTraffic, the solo path (the host twins) and the batch path (gather, call, scatter around one grouped
// device call, which the caller passes in).  The controller and the handle are not known here: tests/step_hdv_checks.cpp runs the batch
// path against the solo path under the sanitizers, with the host twins group by group in the device call's place.
// What it restates (file:line relative to the reference root):
//   HDV traffic info          HighLevelController.update_hdv_traffic_info (hlc/controller/HighLevelController.m:394-447), through
//                             pdmpc_hdv_traffic_host / pdmpc_hdv_traffic_grouped; the HDVs' trim: ManualVehicle.m:33
//   the HDV sets of a CAV     vectorize_all_obstacles.m:33-62 (HdvTraffic::gather, step_types.hpp)
// The drivers and recordings have no counterpart in the reference (include/pdmpc_hdv.h: the driver model).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>

#include "hdv_drive_host.hpp"    // the checks of the HDV drivers' parameters
#include "hdv_grouped_host.hpp"  // the batches of the traffic stage
#include "step_types.hpp"

namespace {
// ---- a member's map as arguments: its lanelets as pdmpc_hdv_drive_host / _place_host take them (10 arguments), and with the HDV
// automaton's hulls behind them as the traffic calls, the map check and the handle's map slots do (13)
template <class F>
inline auto hdv_with_lanelets(const HdvTraffic& H, F&& f) {
    return f((int32_t)H.lan_off.size() - 1, H.lan_off.data(), H.lan_off.data(), H.left_x.data(), H.left_y.data(), H.right_x.data(), H.right_y.data(), H.succ_off.data(),
             H.succ_idx.data(), H.rel.data());
}
template <class F>
inline auto hdv_with_map(const HdvTraffic& H, int Hp, F&& f) {
    const pdmpc_polygon_set local = view_polygons(H.local_off, H.local_x, H.local_y);
    return hdv_with_lanelets(H, [&](auto... lanelets) { return f(lanelets..., (int32_t)H.n_trims, (int32_t)Hp, &local); });
}

// ---- the ONE capacity retry of the step preparation (how much room was asked for, how to grow, the call).  call(room, x, y) writes its vertices into (x, y) of capacity room = x.size();
// after PDMPC_ERR_CAPACITY asked() is the room it asked for (< 0: it did not get as far as sizing), and if that is above the room the
// call is made once more with room grow(asked): exactly that for the bounding calls, a quarter more for the HDV traffic calls.
inline size_t exactly(size_t need) { return need; }
inline size_t and_a_quarter(size_t need) { return need + need / 4; }
template <class Asked, class Grow, class Call>
inline int with_room(std::vector<double>& x, std::vector<double>& y, Asked&& asked, Grow&& grow, Call&& call) {
    int rc = call((int32_t)x.size(), x.empty() ? nullptr : x.data(), y.empty() ? nullptr : y.data());
    if (rc != PDMPC_ERR_CAPACITY) return rc;
    const int64_t need = asked();
    if (need <= (int64_t)x.size()) return rc;
    x.resize(grow((size_t)need));
    y.resize(grow((size_t)need));
    return call((int32_t)x.size(), x.data(), y.data());
}

// ---- what the stage reads of a member besides its HdvTraffic
struct HdvMember {
    HdvTraffic* hdv;
    int n_cav, Hp;  // its CAVs and its horizon
    double dt;
    const double *cav_x, *cav_y;  // [n_cav] where the CAVs are measured, and the lanelets they are on
    const int32_t* cav_lanelet;
};
// one grouped HDV traffic call: the HDVs and CAVs of a batch of members, member after member, and what it returns in the blocks of
// pdmpc_hdv_grouped_layout_host
struct HdvCallScratch {
    std::vector<int32_t> slot, hdv_offset, cav_offset, trim, cav_lanelet;
    std::vector<double> x, y, cos_yaw, sin_yaw, tile_dx, tile_dy, cav_x, cav_y, cav_tile_dx, cav_tile_dy;
    std::vector<int32_t> closest_at, list_at, set_offset_at, set_at;
    std::vector<int64_t> adjacency_at;
    std::vector<int32_t> closest_off, closest_idx, n_rows, row_hdv, set_off, set_base;
    std::vector<double> set_x, set_y;
    std::vector<uint8_t> set_flags, adjacency;
    // the drive pass in front (pdmpc_hdv_drive_traffic_grouped), when a member of the batch has drivers
    std::vector<uint8_t> drives, route_closed;
    std::vector<int32_t> route_off, route_id, seg, new_seg;
    std::vector<double> u, v_des, params, dt, new_u, speed, gap;
};
constexpr size_t HDV_ROOM_FLOOR = 4096;  // vertices a member's and a call's set arrays have room for from the start
inline void at_least(std::vector<double>& x, std::vector<double>& y, size_t room) {
    if (x.size() < room) x.resize(room), y.resize(room);
}
using Doubles = std::pair<std::vector<double>*, const std::vector<double>*>;  // (to, from) of a copy between a member and a call

// ---- a member's HDV state (the bodies of the pdmpc_controller_set_hdv_* entry points: a refusal is its code, and *why its text)
template <class T>
inline bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}
inline bool same_hdv_map(const HdvTraffic& A, const HdvTraffic& B) {
    return &A == &B || (A.n_trims == B.n_trims && same_bytes(A.lan_off, B.lan_off) && same_bytes(A.succ_off, B.succ_off) && same_bytes(A.succ_idx, B.succ_idx) &&
                        same_bytes(A.rel, B.rel) && same_bytes(A.local_off, B.local_off) && same_bytes(A.left_x, B.left_x) && same_bytes(A.left_y, B.left_y) &&
                        same_bytes(A.right_x, B.right_x) && same_bytes(A.right_y, B.right_y) && same_bytes(A.local_x, B.local_x) && same_bytes(A.local_y, B.local_y));
}
// cos and sin of H.yaw, per HDV, as the traffic passes read them ...
inline void hdv_yaw_to_cos_sin(HdvTraffic& H) {
    H.cos_yaw.resize((size_t)H.n);
    H.sin_yaw.resize((size_t)H.n);
    for (int q = 0; q < H.n; ++q) H.cos_yaw[(size_t)q] = std::cos(H.yaw[(size_t)q]), H.sin_yaw[(size_t)q] = std::sin(H.yaw[(size_t)q]);
}
// ... and the yaw of poses given as cos and sin, for read-back only
inline void hdv_driven_yaw(HdvTraffic& H) {
    H.yaw.resize((size_t)H.n);
    for (int q = 0; q < H.n; ++q) H.yaw[(size_t)q] = std::atan2(H.sin_yaw[(size_t)q], H.cos_yaw[(size_t)q]);
}
// Poses from outside, as yaw (measurements) or as directions (cos_yaw, sin_yaw: yaw == nullptr), for HDVs that are set and do not move
// themselves.  `who` was called; their poses are not `what`.
inline int hdv_set_poses(HdvTraffic& H, const char* who, const char* what, const double* x, const double* y, const double* yaw, const double* cos_yaw, const double* sin_yaw,
                         std::string* why) {
    if (H.n == 0) return *why = std::string(who) + " before pdmpc_controller_set_hdvs", PDMPC_ERR_INVALID;
    if (H.driven || H.rec_T > 0)
        return *why = std::string(who) + ": the HDVs move themselves (pdmpc_controller_set_hdv_drivers / _set_hdv_recording); their poses are not " + what, PDMPC_ERR_INVALID;
    H.x.assign(x, x + H.n);
    H.y.assign(y, y + H.n);
    if (yaw) {
        H.yaw.assign(yaw, yaw + H.n);
        hdv_yaw_to_cos_sin(H);
    } else {
        H.cos_yaw.assign(cos_yaw, cos_yaw + H.n);
        H.sin_yaw.assign(sin_yaw, sin_yaw + H.n);
        hdv_driven_yaw(H);
    }
    H.measured = true;
    return PDMPC_OK;
}
inline int hdv_set_recording(HdvTraffic& H, int32_t T, const double* x, const double* y, const double* yaw, std::string* why) {
    *why = "pdmpc_controller_set_hdv_recording: ";
    if (H.n == 0) return *why += "before pdmpc_controller_set_hdvs", PDMPC_ERR_INVALID;
    if (H.driven) return *why += "the HDVs have drivers (pdmpc_controller_set_hdv_drivers)", PDMPC_ERR_INVALID;
    H.rec_T = T;
    H.rec_builds = 0;
    H.rec_x.assign(x, x + (size_t)T * H.n);
    H.rec_y.assign(y, y + (size_t)T * H.n);
    H.rec_yaw.assign(yaw, yaw + (size_t)T * H.n);
    return PDMPC_OK;
}
// the routes against the member's map, and the placement on them adopted as the drivers' state: the "measurement" of the first step
inline int hdv_set_drivers(HdvTraffic& H, double dt, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const double* start_distance,
                           const double* v_des, const double* params, std::string* why) {
    const std::string who = "pdmpc_controller_set_hdv_drivers: ";
    if (H.n == 0) return *why = who + "before pdmpc_controller_set_hdvs", PDMPC_ERR_INVALID;
    if (H.rec_T > 0) return *why = who + "the HDVs replay a recording (pdmpc_controller_set_hdv_recording)", PDMPC_ERR_INVALID;
    if (route_offset[0] != 0) return *why = who + "route offsets that do not start at 0", PDMPC_ERR_INVALID;
    for (int q = 0; q < H.n; ++q)
        if (route_offset[q + 1] < route_offset[q]) return *why = who + "route offsets decrease", PDMPC_ERR_INVALID;
    if (const int rc = hdv_check_drive(params, dt, H.n, v_des, why)) return *why = who + *why, rc;
    std::vector<int32_t> seg((size_t)2 * H.n);
    std::vector<double> u((size_t)H.n), x((size_t)H.n), y((size_t)H.n), cs((size_t)H.n), sn((size_t)H.n);
    const int rc = hdv_with_lanelets(H, [&](auto... lanelets) {
        return pdmpc_hdv_place_host(lanelets..., H.n, route_offset, route_lanelet, closed, start_distance, H.tile_dx.data(), H.tile_dy.data(), seg.data(), u.data(), x.data(),
                                    y.data(), cs.data(), sn.data());
    });
    if (rc) return *why = who + pdmpc_last_error(), rc;
    H.route_off.assign(route_offset, route_offset + H.n + 1);
    H.route_id.assign(route_lanelet, route_lanelet + route_offset[H.n]);
    H.route_id.push_back(0);
    H.route_closed.assign(closed, closed + H.n);
    H.v_des.assign(v_des, v_des + H.n);
    std::copy(params, params + 4, H.drive_params);
    H.seg = seg;
    H.u = u;
    H.new_seg.assign((size_t)2 * H.n, 0);
    H.new_u.assign((size_t)H.n, 0.0);
    H.speed.assign((size_t)H.n, 0.0);
    H.gap.assign((size_t)H.n, (double)INFINITY);
    H.x = x;
    H.y = y;
    H.cos_yaw = cs;
    H.sin_yaw = sn;
    hdv_driven_yaw(H);
    H.driven = true;
    H.driven_builds = 0;
    H.measured = true;
    return PDMPC_OK;
}

// What a member's HDVs are measured as at this built step.  A recording: its next row.  Drivers: true if they move this step (every
// built step but the first after pdmpc_controller_set_hdv_drivers, whose measurement is the placement).
inline bool hdv_begin_build(HdvTraffic& H) {
    if (H.rec_T > 0) {
        H.rec_builds += 1;
        const size_t row = (size_t)(std::min(H.rec_builds, H.rec_T) - 1) * H.n;
        H.x.assign(H.rec_x.begin() + row, H.rec_x.begin() + row + H.n);
        H.y.assign(H.rec_y.begin() + row, H.rec_y.begin() + row + H.n);
        H.yaw.assign(H.rec_yaw.begin() + row, H.rec_yaw.begin() + row + H.n);
        hdv_yaw_to_cos_sin(H);
        H.measured = true;
    }
    if (H.driven) H.driven_builds += 1;
    return H.driven && H.driven_builds > 1;
}
// the room a member's results need (what its own traffic call would size)
inline void hdv_size_results(HdvTraffic& H, int n_cav, int Hp) {
    const size_t lists = (size_t)H.n * PDMPC_HDV_MAX_CHAINS;
    H.closest_off.assign((size_t)H.n + 1, 0);
    H.closest_idx.resize(lists);
    H.row_hdv.resize(lists);
    H.set_off.assign(lists * Hp + 1, 0);
    H.set_flags.resize(lists * Hp);
    H.adjacency.assign((size_t)n_cav * H.n, 0);
    at_least(H.set_x, H.set_y, HDV_ROOM_FLOOR);
}

// ---- the solo path: one member through the host twins, the driver step (if its HDVs move this step) in front of its traffic call
inline int hdv_solo_step(const HdvMember& m, bool drives, std::string* why) {
    HdvTraffic& H = *m.hdv;
    if (drives) {
        const int rc = hdv_with_lanelets(H, [&](auto... lanelets) {
            return pdmpc_hdv_drive_host(lanelets..., H.n, H.route_off.data(), H.route_id.data(), H.route_closed.data(), H.seg.data(), H.u.data(), H.tile_dx.data(), H.tile_dy.data(),
                                        H.v_des.data(), m.n_cav, m.cav_x, m.cav_y, H.cav_tile_dx.data(), H.cav_tile_dy.data(), H.drive_params, m.dt, H.new_seg.data(),
                                        H.new_u.data(), H.x.data(), H.y.data(), H.cos_yaw.data(), H.sin_yaw.data(), H.speed.data(), H.gap.data());
        });
        if (rc) return *why = std::string("pdmpc_hdv_drive_host: ") + pdmpc_last_error(), rc;
        H.seg.swap(H.new_seg);
        H.u.swap(H.new_u);
        hdv_driven_yaw(H);
    }
    hdv_size_results(H, m.n_cav, m.Hp);
    auto asked = [&]() { return H.n_rows >= 0 ? (int64_t)H.set_off[(size_t)H.n_rows * m.Hp] : -1; };  // (the offsets size the second call)
    const int rc = with_room(H.set_x, H.set_y, asked, and_a_quarter, [&](int32_t room, double* set_x, double* set_y) {
        return hdv_with_map(H, m.Hp, [&](auto... map) {
            return pdmpc_hdv_traffic_host(map..., H.n, H.x.data(), H.y.data(), H.cos_yaw.data(), H.sin_yaw.data(), H.trim.data(), H.tile_dx.data(), H.tile_dy.data(), m.n_cav, m.cav_x,
                                          m.cav_y, m.cav_lanelet, H.cav_tile_dx.data(), H.cav_tile_dy.data(), H.closest_off.data(), H.closest_idx.data(), room, &H.n_rows,
                                          H.row_hdv.data(), H.set_off.data(), set_x, set_y, H.set_flags.data(), H.adjacency.data());
        });
    });
    if (rc) return *why = "pdmpc_hdv_traffic_host failed", rc;
    H.gather(m.n_cav, m.Hp);
    return PDMPC_OK;
}

// ---- the batch path: the members of batch B (their maps are in the slots B.slot) as the groups of ONE device call, in three parts.
// Gather: members -> C, with every group's blocks by pdmpc_hdv_grouped_layout_host; *any_drives: a member moves its HDVs this step
// (drives_of[member]), so the call is the one with the drive pass in front.  The set arrays get room for `floor` vertices at least.
inline int hdv_gather_batch(const HdvMember* members, const HdvBatch& B, const uint8_t* drives_of, HdvCallScratch& C, bool* any_drives, size_t floor = HDV_ROOM_FLOOR) {
    const int G = (int)B.members.size(), Hp = members[B.members[0]].Hp;
    *any_drives = false;
    for (auto* v : {&C.drives, &C.route_closed}) v->clear();
    for (auto* v : {&C.route_id, &C.seg, &C.new_seg, &C.slot, &C.trim, &C.cav_lanelet}) v->clear();
    for (auto* v : {&C.u, &C.v_des, &C.params, &C.dt, &C.x, &C.y, &C.cos_yaw, &C.sin_yaw, &C.tile_dx, &C.tile_dy, &C.cav_x, &C.cav_y, &C.cav_tile_dx, &C.cav_tile_dy}) v->clear();
    for (auto* v : {&C.route_off, &C.hdv_offset, &C.cav_offset}) v->assign(1, 0);
    auto append = [](auto& to, const auto& from, size_t count) { to.insert(to.end(), from, from + (ptrdiff_t)count); };
    for (int g = 0; g < G; ++g) {
        const HdvMember& m = members[B.members[(size_t)g]];
        const HdvTraffic& H = *m.hdv;
        const size_t nh = (size_t)H.n, nc = (size_t)m.n_cav;
        C.slot.push_back(B.slot[(size_t)B.map_of[(size_t)g]]);
        for (Doubles v : {Doubles{&C.x, &H.x}, {&C.y, &H.y}, {&C.cos_yaw, &H.cos_yaw}, {&C.sin_yaw, &H.sin_yaw}, {&C.tile_dx, &H.tile_dx}, {&C.tile_dy, &H.tile_dy}})
            append(*v.first, v.second->begin(), nh);
        for (Doubles v : {Doubles{&C.cav_tile_dx, &H.cav_tile_dx}, {&C.cav_tile_dy, &H.cav_tile_dy}}) append(*v.first, v.second->begin(), nc);
        append(C.trim, H.trim.begin(), nh);
        append(C.cav_x, m.cav_x, nc);
        append(C.cav_y, m.cav_y, nc);
        append(C.cav_lanelet, m.cav_lanelet, nc);
        C.hdv_offset.push_back((int32_t)C.x.size());
        C.cav_offset.push_back((int32_t)C.cav_x.size());
        // the drive pass: a member that does not move this step has no routes (the offsets do not move over its HDVs)
        const bool drives = drives_of[B.members[(size_t)g]] != 0;
        *any_drives = *any_drives || drives;
        C.drives.push_back(drives ? 1 : 0);
        for (size_t q = 0; q < nh; ++q) {
            if (drives) C.route_id.insert(C.route_id.end(), H.route_id.begin() + H.route_off[q], H.route_id.begin() + H.route_off[q + 1]);
            C.route_off.push_back((int32_t)C.route_id.size());
            C.route_closed.push_back(drives ? H.route_closed[q] : 0);
            C.seg.push_back(drives ? H.seg[q] : 0);          // r of every HDV of the call ...
            C.new_seg.push_back(drives ? H.seg[nh + q] : 0);  // (... and j, put behind them below)
            C.u.push_back(drives ? H.u[q] : 0.0);
            C.v_des.push_back(drives ? H.v_des[q] : 0.0);
        }
        for (int q = 0; q < 4; ++q) C.params.push_back(drives ? H.drive_params[q] : 1.0);
        C.dt.push_back(m.dt);
    }
    const size_t n_all = C.x.size();
    C.seg.insert(C.seg.end(), C.new_seg.begin(), C.new_seg.end());
    C.seg.push_back(0);  // (never an empty array: one entry more, here and below)
    C.route_id.push_back(0);
    C.new_seg.assign(2 * n_all + 1, 0);
    for (auto* v : {&C.new_u, &C.speed, &C.gap}) v->assign(n_all + 1, 0.0);
    for (auto* v : {&C.closest_at, &C.list_at, &C.set_offset_at, &C.set_at}) v->assign((size_t)G + 1, 0);
    C.adjacency_at.assign((size_t)G + 1, 0);
    if (const int rc = pdmpc_hdv_grouped_layout_host(G, C.hdv_offset.data(), C.cav_offset.data(), Hp, C.closest_at.data(), C.list_at.data(), C.set_offset_at.data(), C.set_at.data(),
                                                     C.adjacency_at.data()))
        return rc;
    C.closest_off.assign((size_t)C.closest_at[(size_t)G], 0);
    C.closest_idx.assign((size_t)C.list_at[(size_t)G] + 1, 0);
    C.row_hdv.assign((size_t)C.list_at[(size_t)G] + 1, 0);
    C.set_off.assign((size_t)C.set_offset_at[(size_t)G], 0);
    C.set_flags.assign((size_t)C.set_at[(size_t)G] + 1, 0);
    C.adjacency.assign((size_t)C.adjacency_at[(size_t)G] + 1, 0);
    C.n_rows.assign((size_t)G, 0);
    C.set_base.assign((size_t)G + 1, 0);
    at_least(C.set_x, C.set_y, floor);
    return PDMPC_OK;
}
// The call: call(C, any_drives) is pdmpc_hdv_drive_traffic_grouped (any_drives) or pdmpc_hdv_traffic_grouped on C's arrays with room
// C.set_x.size(), under the retry: the totals size the second call, if every group got as far as its rows.
template <class Call>
inline int hdv_call_batch(HdvCallScratch& C, bool any_drives, Call&& call) {
    auto asked = [&]() { return *std::min_element(C.n_rows.begin(), C.n_rows.end()) >= 0 ? (int64_t)C.set_base.back() : -1; };
    return with_room(C.set_x, C.set_y, asked, and_a_quarter, [&](int32_t, double*, double*) { return call(C, any_drives); });
}
// Scatter: every member's blocks of C back into its own arrays, as its own call leaves them
inline void hdv_scatter_batch(const HdvMember* members, const HdvBatch& B, const HdvCallScratch& C) {
    const size_t n_all = (size_t)C.hdv_offset.back();
    for (size_t g = 0; g < B.members.size(); ++g) {
        const HdvMember& m = members[B.members[g]];
        HdvTraffic& H = *m.hdv;
        const size_t h0 = (size_t)C.hdv_offset[g], nh = (size_t)H.n;
        if (C.drives[g]) {  // where the drive pass left the member's HDVs
            for (Doubles v : {Doubles{&H.u, &C.new_u}, {&H.speed, &C.speed}, {&H.gap, &C.gap}, {&H.x, &C.x}, {&H.y, &C.y}, {&H.cos_yaw, &C.cos_yaw}, {&H.sin_yaw, &C.sin_yaw}})
                std::copy_n(v.second->begin() + h0, nh, v.first->begin());
            std::copy_n(C.new_seg.begin() + h0, nh, H.seg.begin());
            std::copy_n(C.new_seg.begin() + n_all + h0, nh, H.seg.begin() + nh);
            hdv_driven_yaw(H);
        }
        hdv_size_results(H, m.n_cav, m.Hp);
        const size_t rows = (size_t)C.n_rows[g], sets = rows * m.Hp;
        const int32_t* so = C.set_off.data() + C.set_offset_at[g];
        const size_t total = (size_t)so[sets];
        H.n_rows = (int32_t)rows;
        std::copy_n(C.closest_off.begin() + C.closest_at[g], nh + 1, H.closest_off.begin());
        std::copy_n(C.closest_idx.begin() + C.list_at[g], (size_t)H.closest_off[nh], H.closest_idx.begin());
        std::copy_n(C.row_hdv.begin() + C.list_at[g], rows, H.row_hdv.begin());
        std::copy_n(so, sets + 1, H.set_off.begin());
        std::copy_n(C.set_flags.begin() + C.set_at[g], sets, H.set_flags.begin());
        std::copy_n(C.adjacency.begin() + (ptrdiff_t)C.adjacency_at[g], (size_t)m.n_cav * nh, H.adjacency.begin());
        if (H.set_x.size() < total) at_least(H.set_x, H.set_y, and_a_quarter(total));
        std::copy_n(C.set_x.begin() + C.set_base[g], total, H.set_x.begin());
        std::copy_n(C.set_y.begin() + C.set_base[g], total, H.set_y.begin());
        H.gather(m.n_cav, m.Hp);
    }
}
}  // namespace
