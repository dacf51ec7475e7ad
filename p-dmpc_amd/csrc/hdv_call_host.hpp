// hdv_call_host.hpp — the host-only plan of the HDV device calls (pdmpc_hdv_traffic, pdmpc_hdv_traffic_grouped, pdmpc_hdv_drive_grouped,
// pdmpc_hdv_drive_traffic_grouped): the map table, ONE workspace layout for all four, the caller's arrays as records,
// and the stages of a call -- check, zero, stage, arguments, scatter -- on plain blocks of memory.  step_prep.cpp puts the handle's
// buffers, the two copies, the launch and the synchronisation between them.  No HIP header, no handle (tests/hdv_grouped_checks.cpp runs
// this file under the sanitizers with blocks of exactly the computed sizes).
#pragma once
#include <algorithm>
#include <string>

#include "carver.hpp"
#include "hdv_drive_host.hpp"
#include "hdv_grouped_host.hpp"
#include "pdmpc_device.h"

// HdvMapSlot::table: the map (HdvMapData's arrays) and the HDV automaton's local hulls (x of every vertex, then y)
struct HdvTable {
    size_t pt_off, pts, succ_off, succ_idx, rel, local_off, local_xy, total;
};
inline HdvTable hdv_table(const HdvMapData& m, int n_polygons, int local_tot) {
    Carver c;
    HdvTable T;
    T.pt_off = c.take<int32_t>((size_t)m.n_lanelets + 1);
    T.pts = c.take<double>((size_t)6 * m.n_pts);
    T.succ_off = c.take<int32_t>((size_t)m.n_lanelets + 1);
    T.succ_idx = c.take<int32_t>((size_t)m.n_succ);
    T.rel = c.take<uint8_t>((size_t)m.n_lanelets * m.n_lanelets);
    T.local_off = c.take<int32_t>((size_t)n_polygons + 1);
    T.local_xy = c.take<double>((size_t)2 * local_tot);
    T.total = c.end8();
    return T;
}

// ---- the caller's arrays.  A call has its vehicles, a traffic part or none (null), a drive part or none (null).
// The vehicles of all groups, group after group, and what every pass reads of them.  n_groups = 0 in the ungrouped call.
struct HdvGroups {
    int32_t n_groups;
    const int32_t *group_slot, *hdv_offset, *cav_offset;
    const double *tile_dx, *tile_dy, *cav_x, *cav_y, *cav_tile_dx, *cav_tile_dy;
};
// the five traffic passes: poses in, lists, lanes and adjacency out (set_base: the grouped calls'; n_rows: [n_groups], or one entry)
struct HdvTrafficCall {
    const double *x, *y, *cos_yaw, *sin_yaw;
    const int32_t *trim, *cav_lanelet;
    int32_t *closest_offset, *closest_index;
    int32_t capacity;
    int32_t *n_rows, *row_hdv, *set_offset, *set_base;
    double *set_x, *set_y;
    uint8_t *set_flags, *adjacency;
};
// the drive pass: what pdmpc_hdv_drive_grouped and pdmpc_hdv_drive_traffic_grouped take beyond pdmpc_hdv_traffic_grouped
struct HdvDriveCall {
    const uint8_t* drives;  // [n_groups], or null: every group drives
    const int32_t *route_offset, *route_lanelet;
    const uint8_t* closed;
    const int32_t* state_seg;
    const double *state_u, *v_des, *parameters, *dt;
    int32_t* new_seg;
    double *new_u, *x, *y, *cos_yaw, *sin_yaw, *speed, *gap;
};

// What the checks find out about a call: the sizes, where every group's blocks stand in the caller's arrays (hdv_grouped_layout; empty
// in the ungrouped call) and the vertices actually read back -- no more than the slots can hold, whatever room the caller has.
struct HdvPlan {
    int n = 0, nc = 0, Hp = 1, n_route = -1, cap = 0;
    int64_t pairs = 0;
    std::vector<int32_t> closest_at, list_at, set_offset_at, set_at;
    std::vector<int64_t> adjacency_at;
};
// HdvState::slots, the lane pass's work: x of PDMPC_BOUND_SLOT vertices for every (HDV, chain, step), then y
inline size_t hdv_slot_doubles(const HdvPlan& P) { return 2 * (size_t)P.n * PDMPC_HDV_MAX_CHAINS * P.Hp * PDMPC_BOUND_SLOT; }
inline int hdv_read_back_cap(int n, int Hp, const HdvTrafficCall* T) {
    const size_t slots = (size_t)n * PDMPC_HDV_MAX_CHAINS * Hp;
    return (int)std::min<size_t>(T ? (size_t)T->capacity : 0, T && T->set_x && T->set_y ? slots * PDMPC_BOUND_SLOT : 0);
}
// the plan of the ungrouped call (arguments checked by hdv_check_call)
inline HdvPlan hdv_plan_one(int n, int nc, int Hp, const HdvTrafficCall& T) {
    HdvPlan P;
    P.n = n;
    P.nc = nc;
    P.Hp = Hp;
    P.pairs = (int64_t)nc * n;
    P.cap = hdv_read_back_cap(n, Hp, &T);
    return P;
}

// HdvState::ws and its pinned staging for a planned call of G groups: the inputs are the block's first in_bytes, the device-only
// regions follow, what the call reads back is everything from `out` on (the packed vertices last: x of P.cap vertices, then y).
// The ungrouped call is G = 0: the groups' records and lookups and the scan's regions are empty.  With a drive pass in front
// (P.n_route >= 0: the lanelet ids of all routes): the routes, old states, desired speeds and parameters among the inputs, the new
// states, speeds, gaps and poses among what is read back; without one those regions are empty.
struct HdvWs {
    size_t in, cav, trim, cav_lanelet, groups, group_of, pair_first, drives, route_off, route_id, closed, state_seg, state_u, v_des, params, in_bytes;
    size_t n_chains, chain_id, chain_succ, slot_n, slot_flags, slot_before, row_base;
    size_t out, status, n_rows, set_base, n_closest, closest, row_hdv, set_off, set_flags, adjacency, new_seg, new_u, speed, gap, pose, set_xy, total;
};
inline HdvWs hdv_ws(int G, const HdvPlan& P) {
    const int n = P.n, nc = P.nc, Hp = P.Hp, n_route = P.n_route;
    const size_t dn = n_route < 0 ? 0 : (size_t)n, dG = n_route < 0 ? 0 : (size_t)G;  // (no drive pass)
    const size_t lists = (size_t)n * PDMPC_HDV_MAX_CHAINS, slots = lists * Hp;
    const size_t gn = G ? (size_t)n : 0, gslots = G ? slots : 0, G1 = G ? (size_t)G + 1 : 0;  // (no groups)
    Carver c;
    HdvWs L;
    L.in = c.take<double>((size_t)6 * n);
    L.cav = c.take<double>((size_t)4 * nc);
    L.trim = c.take<int32_t>((size_t)n);
    L.cav_lanelet = c.take<int32_t>((size_t)nc);
    L.groups = c.take<HdvGroup>((size_t)G);
    L.group_of = c.take<int32_t>(gn);
    L.pair_first = c.take<int32_t>(G1);
    L.drives = c.take<uint8_t>(dG);
    L.route_off = c.take<int32_t>(dn ? dn + 1 : 0);
    L.route_id = c.take<int32_t>(n_route < 0 ? 0 : (size_t)n_route);
    L.closed = c.take<uint8_t>(dn);
    L.state_seg = c.take<int32_t>(2 * dn);
    L.state_u = c.take<double>(dn);
    L.v_des = c.take<double>(dn);
    L.params = c.take<double>(PDMPC_HDV_DRIVE_PARAMS * dG);
    L.in_bytes = c.end8();
    L.n_chains = c.take<int32_t>((size_t)n);
    L.chain_id = c.take<int32_t>(lists);
    L.chain_succ = c.take<int32_t>(lists);
    L.slot_n = c.take<int32_t>(slots);
    L.slot_flags = c.take<uint8_t>(slots);
    L.slot_before = c.take<int32_t>(gslots);
    L.row_base = c.take<int32_t>(gn);
    L.out = c.end8();
    L.status = c.take<int32_t>(2);
    L.n_rows = c.take<int32_t>((size_t)G);
    L.set_base = c.take<int32_t>(G1);
    L.n_closest = c.take<int32_t>((size_t)n);
    L.closest = c.take<int32_t>(lists);
    L.row_hdv = c.take<int32_t>(lists);
    L.set_off = c.take<int32_t>(slots + G + 1);
    L.set_flags = c.take<uint8_t>(slots);
    L.adjacency = c.take<uint8_t>((size_t)P.pairs);
    L.new_seg = c.take<int32_t>(2 * dn);
    L.new_u = c.take<double>(dn);
    L.speed = c.take<double>(dn);
    L.gap = c.take<double>(dn);
    L.pose = c.take<double>(4 * dn);
    L.set_xy = c.take<double>((size_t)2 * P.cap);
    L.total = c.at;
    return L;
}

// ---- stage 1, check: a grouped call against the map slots (slot[s] null: nothing uploaded).  PDMPC_OK and the plan, or the code of the
// first test that fails with its text in *why.  Without the traffic passes the poses, trims, CAV lanelets and traffic outputs are not read.
inline int hdv_check_grouped(const char* who, const HdvGroups& G, const HdvTrafficCall* T, const HdvDriveCall* D, const HdvSlotData* const* slot, HdvPlan& P,
                             std::string* why) {
    const auto refuse = [&](int rc, const std::string& text) {
        *why = who + text;
        return rc;
    };
    const auto refuse_group = [&](int rc, int g, const std::string& text) { return refuse(rc, "group " + std::to_string(g) + ": " + text); };
    const int32_t n_groups = G.n_groups, *hdv_offset = G.hdv_offset, *cav_offset = G.cav_offset;
    P = HdvPlan();
    if (n_groups < 0 || (T && T->capacity < 0) || (n_groups && (!G.group_slot || !hdv_offset || !cav_offset)) ||
        (T && (!T->set_base || (n_groups && (!T->closest_offset || !T->n_rows || !T->set_offset)))))
        return refuse(PDMPC_ERR_INVALID, "bad argument");
    if (n_groups == 0) return PDMPC_OK;
    if (hdv_offset[0] != 0 || cav_offset[0] != 0) return refuse(PDMPC_ERR_INVALID, "offsets that do not start at 0");
    int Hp = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (hdv_offset[g + 1] < hdv_offset[g] || cav_offset[g + 1] < cav_offset[g]) return refuse_group(PDMPC_ERR_INVALID, g, "offsets decrease");
        if (G.group_slot[g] < 0 || G.group_slot[g] >= PDMPC_HDV_MAP_SLOTS) return refuse_group(PDMPC_ERR_INVALID, g, "map slot out of range");
        const HdvSlotData* M = slot[G.group_slot[g]];
        if (!M) return refuse_group(PDMPC_ERR_INVALID, g, "no map was uploaded into its slot");
        if (T && Hp && M->Hp != Hp) return refuse_group(PDMPC_ERR_INVALID, g, "the Hp of its slot differs from the slots of the groups before");
        Hp = T ? M->Hp : 1;
    }
    const int n = hdv_offset[n_groups], nc = cav_offset[n_groups];
    const size_t G1 = (size_t)n_groups + 1;
    P.closest_at.resize(G1);
    P.list_at.resize(G1);
    P.set_offset_at.resize(G1);
    P.set_at.resize(G1);
    P.adjacency_at.resize(G1);
    if (const int rc = hdv_grouped_layout(n_groups, hdv_offset, cav_offset, Hp, P.closest_at.data(), P.list_at.data(), P.set_offset_at.data(), P.set_at.data(), P.adjacency_at.data()))
        return refuse(rc, "bad offsets");
    const int64_t pairs = P.adjacency_at[(size_t)n_groups];
    for (int g = 0; g < n_groups; ++g)
        if (hdv_offset[g + 1] - hdv_offset[g] > PDMPC_HDV_MAX_VEHICLES || cav_offset[g + 1] - cav_offset[g] > PDMPC_HDV_MAX_CAVS)
            return refuse_group(PDMPC_ERR_CAPACITY, g, "more than PDMPC_HDV_MAX_VEHICLES HDVs or PDMPC_HDV_MAX_CAVS CAVs");
    if (n > PDMPC_HDV_GROUPED_MAX_VEHICLES) return refuse(PDMPC_ERR_CAPACITY, "more than PDMPC_HDV_GROUPED_MAX_VEHICLES HDVs in the call");
    if (pairs > INT32_MAX) return refuse(PDMPC_ERR_CAPACITY, "2^31 or more (CAV, HDV) pairs");
    if (n && (!G.tile_dx || !G.tile_dy || (T && (!T->x || !T->y || !T->cos_yaw || !T->sin_yaw || !T->trim || !T->closest_index || !T->row_hdv))))
        return refuse(PDMPC_ERR_INVALID, "a null HDV array");
    if (nc && (!G.cav_x || !G.cav_y || !G.cav_tile_dx || !G.cav_tile_dy || (T && !T->cav_lanelet))) return refuse(PDMPC_ERR_INVALID, "a null CAV array");
    if (T && pairs && !T->adjacency) return refuse(PDMPC_ERR_INVALID, "no adjacency array");
    // the drive pass: routes and states of the groups that drive against their maps (an HDV of a group that does not drive has no route)
    if (D) {
        if (!D->route_offset || D->route_offset[0] != 0 || !D->parameters || !D->dt ||
            (n && (!D->closed || !D->state_seg || !D->state_u || !D->v_des || !D->new_seg || !D->new_u || !D->x || !D->y || !D->cos_yaw || !D->sin_yaw || !D->speed || !D->gap)))
            return refuse(PDMPC_ERR_INVALID, "a null driver array, or route offsets that do not start at 0");
        for (int q = 0; q < n; ++q)
            if (D->route_offset[q + 1] < D->route_offset[q]) return refuse(PDMPC_ERR_INVALID, "route offsets decrease");
        P.n_route = D->route_offset[n];
        for (int g = 0; g < n_groups; ++g) {
            if (D->drives && !D->drives[g]) continue;
            const int h0 = hdv_offset[g], ng = hdv_offset[g + 1] - h0;
            const HdvMapData& map = slot[G.group_slot[g]]->map;
            std::string text;
            int rc = hdv_check_routes(map, ng, D->route_offset + h0, D->route_lanelet, D->closed + h0, &text);
            if (!rc) rc = hdv_check_states(map, ng, D->route_offset + h0, D->route_lanelet, D->closed + h0, D->state_seg + h0, D->state_seg + n + h0, D->state_u + h0, &text);
            if (!rc) rc = hdv_check_drive(D->parameters + 4 * (size_t)g, D->dt[g], ng, D->v_des + h0, &text);
            if (rc) return refuse_group(rc, g, text);
        }
    }
    for (int g = 0; T && g < n_groups; ++g) {
        const HdvSlotData& S = *slot[G.group_slot[g]];
        for (int q = hdv_offset[g]; q < hdv_offset[g + 1]; ++q)
            if (T->trim[q] < 1 || T->trim[q] > S.trims) return refuse_group(PDMPC_ERR_INVALID, g, "trim out of range");
        for (int v = cav_offset[g]; v < cav_offset[g + 1]; ++v)
            if (T->cav_lanelet[v] < 1 || T->cav_lanelet[v] > S.map.n_lanelets) return refuse_group(PDMPC_ERR_INVALID, g, "a CAV's lanelet id out of range");
    }
    P.n = n;
    P.nc = nc;
    P.Hp = Hp;
    P.pairs = pairs;
    P.cap = hdv_read_back_cap(n, Hp, T);
    return PDMPC_OK;
}

// ---- stage 2, zero: what has a size whatever happens (after the checks; a call without HDVs ends behind it)
inline void hdv_zero_outputs(const HdvGroups& G, const HdvTrafficCall* T, const HdvPlan& P) {
    if (!T) return;
    for (int g = 0; g < G.n_groups; ++g) {
        T->n_rows[g] = 0;
        T->closest_offset[P.closest_at[(size_t)g]] = 0;
        T->set_offset[P.set_offset_at[(size_t)g]] = 0;
        T->set_base[g] = 0;
    }
    if (T->set_base)
        T->set_base[G.n_groups] = 0;
    else  // (the ungrouped call)
        T->n_rows[0] = T->closest_offset[0] = T->set_offset[0] = 0;
}

// ---- stage 3, stage: the inputs into a block of L.in_bytes bytes (P.n > 0).  Without the traffic passes the poses are zeros.
inline void hdv_stage(unsigned char* hin, const HdvWs& L, const HdvPlan& P, const HdvGroups& G, const HdvTrafficCall* T, const HdvDriveCall* D) {
    const size_t n = (size_t)P.n, nc = (size_t)P.nc;
    double* in = (double*)(hin + L.in);
    if (T)
        stage_poses(in, n, T->x, T->y, T->cos_yaw, T->sin_yaw, (int32_t*)(hin + L.trim), T->trim);
    else
        std::memset(in, 0, 4 * n * sizeof(double));
    std::memcpy(in + 4 * n, G.tile_dx, n * sizeof(double));
    std::memcpy(in + 5 * n, G.tile_dy, n * sizeof(double));
    if (nc) {
        stage_poses((double*)(hin + L.cav), nc, G.cav_x, G.cav_y, G.cav_tile_dx, G.cav_tile_dy);
        if (T) std::memcpy(hin + L.cav_lanelet, T->cav_lanelet, nc * sizeof(int32_t));
    }
    HdvGroup* groups = (HdvGroup*)(hin + L.groups);
    int32_t *group_of = (int32_t*)(hin + L.group_of), *pair_first = (int32_t*)(hin + L.pair_first);
    for (int g = 0; g < G.n_groups; ++g) {
        groups[g] = HdvGroup{G.group_slot[g], G.hdv_offset[g], G.hdv_offset[g + 1] - G.hdv_offset[g], G.cav_offset[g], G.cav_offset[g + 1] - G.cav_offset[g]};
        for (int q = G.hdv_offset[g]; q < G.hdv_offset[g + 1]; ++q) group_of[q] = g;
        pair_first[g] = (int32_t)P.adjacency_at[(size_t)g];
    }
    if (G.n_groups) pair_first[G.n_groups] = (int32_t)P.pairs;
    if (!D) return;
    uint8_t* drives = hin + L.drives;
    for (int g = 0; g < G.n_groups; ++g) {
        drives[g] = D->drives ? (D->drives[g] ? 1 : 0) : 1;
        double* p = (double*)(hin + L.params) + (size_t)g * PDMPC_HDV_DRIVE_PARAMS;
        std::memcpy(p, D->parameters + 4 * (size_t)g, 4 * sizeof(double));
        p[4] = D->dt[g];
    }
    std::memcpy(hin + L.route_off, D->route_offset, (n + 1) * sizeof(int32_t));
    if (P.n_route) std::memcpy(hin + L.route_id, D->route_lanelet, (size_t)P.n_route * sizeof(int32_t));
    std::memcpy(hin + L.closed, D->closed, n);
    std::memcpy(hin + L.state_seg, D->state_seg, 2 * n * sizeof(int32_t));
    std::memcpy(hin + L.state_u, D->state_u, n * sizeof(double));
    std::memcpy(hin + L.v_des, D->v_des, n * sizeof(double));
}

// ---- stage 4, arguments: the kernels' records over a workspace at `ws`, the lane pass's slots at `slots` (x of every slot, then y)
// and -- the grouped calls -- the map records at `maps`.  `one`: the ungrouped call's map, in the record itself.
inline HdvArgs hdv_args(const HdvWs& L, const HdvPlan& P, unsigned char* ws, double* slots, const HdvMapRecord* one = nullptr) {
    HdvArgs A;
    std::memset(&A, 0, sizeof A);
    if (one) {
        A.map = one->map;
        A.local_x = one->local_x;
        A.local_y = one->local_y;
        A.local_off = one->local_off;
    }
    A.n_hdv = P.n;
    A.n_cav = P.nc;
    A.Hp = P.Hp;
    A.capacity = P.cap;
    A.in = (const double*)(ws + L.in);
    A.trim = (const int32_t*)(ws + L.trim);
    A.cav = (const double*)(ws + L.cav);
    A.cav_lanelet = (const int32_t*)(ws + L.cav_lanelet);
    A.n_closest = (int32_t*)(ws + L.n_closest);
    A.closest = (int32_t*)(ws + L.closest);
    A.n_chains = (int32_t*)(ws + L.n_chains);
    A.chain_id = (int32_t*)(ws + L.chain_id);
    A.chain_succ = (int32_t*)(ws + L.chain_succ);
    A.slot_x = slots;
    A.slot_y = slots + hdv_slot_doubles(P) / 2;
    A.slot_n = (int32_t*)(ws + L.slot_n);
    A.slot_flags = ws + L.slot_flags;
    A.status = (int32_t*)(ws + L.status);
    A.row_hdv = (int32_t*)(ws + L.row_hdv);
    A.set_off = (int32_t*)(ws + L.set_off);
    A.set_flags = ws + L.set_flags;
    A.set_x = (double*)(ws + L.set_xy);
    A.set_y = A.set_x + P.cap;
    A.adjacency = ws + L.adjacency;
    return A;
}
inline HdvGroupedArgs hdv_grouped_args(int n_groups, const HdvWs& L, const HdvPlan& P, unsigned char* ws, double* slots, const HdvMapRecord* maps) {
    HdvGroupedArgs GA{};
    GA.a = hdv_args(L, P, ws, slots);
    GA.maps = maps;
    GA.groups = (const HdvGroup*)(ws + L.groups);
    GA.group_of = (const int32_t*)(ws + L.group_of);
    GA.pair_first = (const int32_t*)(ws + L.pair_first);
    GA.n_groups = n_groups;
    GA.n_pairs = (int32_t)P.pairs;
    GA.slot_before = (int32_t*)(ws + L.slot_before);
    GA.row_base = (int32_t*)(ws + L.row_base);
    GA.n_rows = (int32_t*)(ws + L.n_rows);
    GA.set_base = (int32_t*)(ws + L.set_base);
    return GA;
}
inline HdvDriveArgs hdv_drive_args(const HdvWs& L, const HdvPlan& P, unsigned char* ws, const HdvMapRecord* maps) {
    HdvDriveArgs D{};
    D.maps = maps;
    D.groups = (const HdvGroup*)(ws + L.groups);
    D.group_of = (const int32_t*)(ws + L.group_of);
    D.drives = ws + L.drives;
    D.n_hdv = P.n;
    D.n_cav = P.nc;
    D.route_off = (const int32_t*)(ws + L.route_off);
    D.route_id = (const int32_t*)(ws + L.route_id);
    D.closed = ws + L.closed;
    D.state_seg = (const int32_t*)(ws + L.state_seg);
    D.state_u = (const double*)(ws + L.state_u);
    D.v_des = (const double*)(ws + L.v_des);
    D.params = (const double*)(ws + L.params);
    D.cav = (const double*)(ws + L.cav);
    D.in = (double*)(ws + L.in);
    D.new_seg = (int32_t*)(ws + L.new_seg);
    D.new_u = (double*)(ws + L.new_u);
    D.speed = (double*)(ws + L.speed);
    D.gap = (double*)(ws + L.gap);
    D.pose = (double*)(ws + L.pose);
    return D;
}

// ---- stage 5, scatter: from the read-back block (L.total - L.out bytes, the workspace from L.out on) into the caller's arrays
struct HdvBack {
    const unsigned char* block;
    size_t out;
    template <class T>
    const T* at(size_t offset) const {  // the region at the workspace's offset
        return (const T*)(block + (offset - out));
    }
};
// the vertices, when they fit: x of the first `total`, then y from P.cap on
inline void hdv_scatter_vertices(const HdvBack& back, const HdvWs& L, const HdvPlan& P, const HdvTrafficCall& T, int32_t total) {
    if (!total) return;
    const double* hx = back.at<double>(L.set_xy);
    std::memcpy(T.set_x, hx, (size_t)total * sizeof(double));
    std::memcpy(T.set_y, hx + P.cap, (size_t)total * sizeof(double));
}
// The ungrouped call.  Refusals, in this order: lists over (n_rows -1, nothing else written), slot over, capacity (lists, offsets and
// adjacency written, no vertices and no flags).
inline int hdv_scatter_one(const unsigned char* block, const HdvWs& L, const HdvPlan& P, const HdvTrafficCall& T, const char** why) {
    const HdvBack back{block, L.out};
    const int32_t* status = back.at<int32_t>(L.status);
    *T.n_rows = -1;
    *why = "pdmpc_hdv_traffic: an HDV has more than PDMPC_HDV_MAX_CHAINS closest lanelets or chains";
    if (status[1] & PDMPC_HDV_OVER_LISTS) return PDMPC_ERR_CAPACITY;
    const int32_t *n_closest = back.at<int32_t>(L.n_closest), *closest = back.at<int32_t>(L.closest);
    for (int q = 0; q < P.n; ++q) {
        std::memcpy(T.closest_index + T.closest_offset[q], closest + (size_t)q * PDMPC_HDV_MAX_CHAINS, (size_t)n_closest[q] * sizeof(int32_t));
        T.closest_offset[q + 1] = T.closest_offset[q] + n_closest[q];
    }
    const int rows = status[0];
    *T.n_rows = rows;
    std::memcpy(T.row_hdv, back.at<int32_t>(L.row_hdv), (size_t)rows * sizeof(int32_t));
    std::memcpy(T.set_offset, back.at<int32_t>(L.set_off), ((size_t)rows * P.Hp + 1) * sizeof(int32_t));
    if (P.nc) std::memcpy(T.adjacency, back.at<uint8_t>(L.adjacency), (size_t)P.pairs);
    *why = "pdmpc_hdv_traffic: a reachable lane has more than PDMPC_BOUNDED_MAX_COLS vertices";
    if (status[1] & PDMPC_HDV_OVER_SLOT) return PDMPC_ERR_CAPACITY;
    const int32_t total = T.set_offset[(size_t)rows * P.Hp];
    *why = "pdmpc_hdv_traffic: capacity too small for the reachable lanes";
    if (T.capacity < total || (total && (!T.set_x || !T.set_y))) return PDMPC_ERR_CAPACITY;
    hdv_scatter_vertices(back, L, P, T, total);
    if (T.set_flags) std::memcpy(T.set_flags, back.at<uint8_t>(L.set_flags), (size_t)rows * P.Hp);
    return PDMPC_OK;
}
// The grouped calls: the drive results of the groups that drove (the others' entries are left as they are); every group's traffic blocks,
// which stand in the workspace where the caller's arrays have them, but for a group whose lists ran over (n_rows -1 and nothing else);
// set_base and the adjacency; the vertices when they fit.  Refusals: lists over, then slot over, then capacity.
inline int hdv_scatter(const char* who, const unsigned char* block, const HdvWs& L, const HdvPlan& P, const HdvGroups& G, const HdvTrafficCall* T, const HdvDriveCall* D,
                       std::string* why) {
    const HdvBack back{block, L.out};
    const size_t n = (size_t)P.n;
    for (int g = 0; D && g < G.n_groups; ++g) {
        if (D->drives && !D->drives[g]) continue;
        const size_t h0 = (size_t)G.hdv_offset[g], ng = (size_t)G.hdv_offset[g + 1] - h0;
        const int32_t* seg = back.at<int32_t>(L.new_seg);
        const double* pose = back.at<double>(L.pose);
        std::memcpy(D->new_seg + h0, seg + h0, ng * sizeof(int32_t));
        std::memcpy(D->new_seg + n + h0, seg + n + h0, ng * sizeof(int32_t));
        std::memcpy(D->new_u + h0, back.at<double>(L.new_u) + h0, ng * sizeof(double));
        std::memcpy(D->speed + h0, back.at<double>(L.speed) + h0, ng * sizeof(double));
        std::memcpy(D->gap + h0, back.at<double>(L.gap) + h0, ng * sizeof(double));
        std::memcpy(D->x + h0, pose + h0, ng * sizeof(double));
        std::memcpy(D->y + h0, pose + n + h0, ng * sizeof(double));
        std::memcpy(D->cos_yaw + h0, pose + 2 * n + h0, ng * sizeof(double));
        std::memcpy(D->sin_yaw + h0, pose + 3 * n + h0, ng * sizeof(double));
    }
    if (!T) return PDMPC_OK;
    const int32_t* status = back.at<int32_t>(L.status);
    const int32_t *rows_of = back.at<int32_t>(L.n_rows), *n_closest = back.at<int32_t>(L.n_closest), *closest = back.at<int32_t>(L.closest);
    int over = -1;  // the first group with an HDV whose lists ran over
    for (int g = 0; g < G.n_groups; ++g) {
        const int h0 = G.hdv_offset[g], ng = G.hdv_offset[g + 1] - h0, rows = rows_of[g];
        const size_t list_at = (size_t)P.list_at[(size_t)g], set_offset_at = (size_t)P.set_offset_at[(size_t)g], set_at = (size_t)P.set_at[(size_t)g];
        T->n_rows[g] = rows;
        if (rows < 0) {
            if (over < 0) over = g;
            continue;
        }
        int32_t* co = T->closest_offset + P.closest_at[(size_t)g];
        for (int q = 0; q < ng; ++q) {
            std::memcpy(T->closest_index + list_at + co[q], closest + (size_t)(h0 + q) * PDMPC_HDV_MAX_CHAINS, (size_t)n_closest[h0 + q] * sizeof(int32_t));
            co[q + 1] = co[q] + n_closest[h0 + q];
        }
        if (rows) std::memcpy(T->row_hdv + list_at, back.at<int32_t>(L.row_hdv) + list_at, (size_t)rows * sizeof(int32_t));
        std::memcpy(T->set_offset + set_offset_at, back.at<int32_t>(L.set_off) + set_offset_at, ((size_t)rows * P.Hp + 1) * sizeof(int32_t));
        if (T->set_flags && rows) std::memcpy(T->set_flags + set_at, back.at<uint8_t>(L.set_flags) + set_at, (size_t)rows * P.Hp);
    }
    std::memcpy(T->set_base, back.at<int32_t>(L.set_base), ((size_t)G.n_groups + 1) * sizeof(int32_t));
    if (P.pairs) std::memcpy(T->adjacency, back.at<uint8_t>(L.adjacency), (size_t)P.pairs);
    const int32_t total = T->set_base[G.n_groups];
    const bool slot_over = status[1] & PDMPC_HDV_OVER_SLOT, fits = T->capacity >= total && (!total || (T->set_x && T->set_y)) && !slot_over;
    if (fits) hdv_scatter_vertices(back, L, P, *T, total);
    if (over >= 0)
        *why = std::string(who) + "group " + std::to_string(over) + ": an HDV has more than PDMPC_HDV_MAX_CHAINS closest lanelets or chains";
    else if (slot_over)
        *why = std::string(who) + "a reachable lane has more than PDMPC_BOUNDED_MAX_COLS vertices";
    else if (!fits)
        *why = std::string(who) + "capacity too small for the reachable lanes";
    return over >= 0 || !fits ? PDMPC_ERR_CAPACITY : PDMPC_OK;
}
