// step_prepare.hpp — ONE step preparation over a span of members (step_controller.cpp, stage 8 of 9): a sweep's
// members, or the one controller that steps alone.  build_members puts the grouped device calls -- or, without a handle, their host
// twins -- between the members' begin_step and finish_step (step_assembly.hpp) and their batches behind them (step_batch.hpp); it is
// the only place that asks which.  The part of the HDV traffic stage that needs the handle is here too (step_hdv.hpp has the rest).
// What it restates (file:line relative to the reference root):
//   lanelet bounding          HighLevelController.m:219-263 with get_lanelets_boundary.m:69-74 (reachable_sets.cpp / bounded_kernel.hip)
//   coupling by sets          ReachableSetCoupler.m:5-56 (reachable_sets.cpp / reachable_kernel.hip)
//   collision assessment      FcaPrioritizer.m:11-92 (fca.cpp / fca_kernel.hip)
//   a batch's seed            PrioritizedExplorativeController.m:249
#pragma once
#include "step_batch.hpp"

namespace {
// the poses of the members `who` one after the other (and their lanelet polygons: with_lanelets)
inline void gather(pdmpc_controller* const* members, PrepScratch::Call& C, const std::vector<int>& who, bool with_lanelets) {
    C.who = who;
    C.group_offset.assign(1, 0);
    for (auto* v : {&C.x, &C.y, &C.cos_yaw, &C.sin_yaw, &C.lan_x, &C.lan_y}) v->clear();
    C.trim.clear();
    C.lan_off.assign(1, 0);
    for (int m : who) {
        pdmpc_controller* c = members[m];
        C.x.insert(C.x.end(), c->tr.mx.begin(), c->tr.mx.end());
        C.y.insert(C.y.end(), c->tr.my.begin(), c->tr.my.end());
        C.cos_yaw.insert(C.cos_yaw.end(), c->reach.cos_yaw.begin(), c->reach.cos_yaw.end());
        C.sin_yaw.insert(C.sin_yaw.end(), c->reach.sin_yaw.begin(), c->reach.sin_yaw.end());
        C.trim.insert(C.trim.end(), c->in.trims.begin(), c->in.trims.end());
        C.group_offset.push_back((int32_t)C.x.size());
        if (with_lanelets) {
            lanelet_polygons(c->sc, c->in, c->reach);
            const int32_t base = (int32_t)C.lan_x.size(), nl = c->reach.lan_off[(size_t)c->sc.n];
            C.lan_x.insert(C.lan_x.end(), c->reach.lan_x.begin(), c->reach.lan_x.begin() + nl);
            C.lan_y.insert(C.lan_y.end(), c->reach.lan_y.begin(), c->reach.lan_y.begin() + nl);
            for (int v = 0; v < c->sc.n; ++v) C.lan_off.push_back(base + c->reach.lan_off[(size_t)v + 1]);
        }
    }
    C.lan_x.push_back(0.0);  // (never empty)
    C.lan_y.push_back(0.0);
    size_t entries = 0;
    for (size_t g = 0; g + 1 < C.group_offset.size(); ++g) entries += (size_t)(C.group_offset[g + 1] - C.group_offset[g]) * (C.group_offset[g + 1] - C.group_offset[g]);
    C.adjacency.assign(entries + 1, 0);
}
// the blocks of a grouped coupler call -> c->in.adjacency of the members that couple by reachable sets
inline void scatter_blocks(pdmpc_controller* const* members, const PrepScratch::Call& C) {
    size_t block = 0;
    for (int m : C.who) {
        pdmpc_controller* c = members[m];
        const size_t nn = (size_t)c->sc.n * c->sc.n;
        if (c->sc.cfg.coupling == PDMPC_COUPLING_REACHABLE_SET) c->in.adjacency.assign(C.adjacency.begin() + block, C.adjacency.begin() + block + nn);
        block += nn;
    }
}
inline bool any_couples_by_sets(pdmpc_controller* const* members, const std::vector<int>& who) {
    for (int m : who)
        if (members[m]->sc.cfg.coupling == PDMPC_COUPLING_REACHABLE_SET) return true;
    return false;
}

// lanelet bounding of the members `who` (one all_steps for all of them) in ONE device call on the concatenated vehicles, then the
// coupler on the bounded step-Hp sets (on the device they are still there), grouped by member
inline int bound_on_device(pdmpc_handle* h, pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who, bool all_steps) {
    if (who.empty()) return PDMPC_OK;
    PrepScratch::Call& C = S.call;
    gather(members, C, who, true);
    const int Hp = members[who[0]]->sc.Hp, sets_each = all_steps ? Hp : 1, n = C.group_offset.back();
    const pdmpc_polygon_set lan = view_polygons(C.lan_off, C.lan_x, C.lan_y);
    C.set_off.assign((size_t)n * sets_each + 1, 0);
    S.prep_calls[0] += 1;
    int rc = with_room(C.set_x, C.set_y, [&]() { return (int64_t)C.set_off.back(); }, exactly, [&](int32_t cap, double* ox, double* oy) {
        return pdmpc_bound_reachable_sets(h, n, C.x.data(), C.y.data(), C.cos_yaw.data(), C.sin_yaw.data(), C.trim.data(), &lan, all_steps, cap, C.set_off.data(), ox, oy, nullptr);
    });
    if (rc) return cfail(nullptr, rc, std::string("pdmpc_bound_reachable_sets: ") + pdmpc_last_error());
    for (size_t g = 0; g < who.size(); ++g) {  // every member's own sets, offsets from 0, as a bounding call for it alone leaves them
        pdmpc_controller* c = members[who[g]];
        const size_t o0 = (size_t)C.group_offset[g] * sets_each, sets = (size_t)c->sc.n * sets_each;
        const int32_t a = C.set_off[o0], total = C.set_off[o0 + sets] - a;
        c->reach.bound_off.resize(sets + 1);
        for (size_t o = 0; o <= sets; ++o) c->reach.bound_off[o] = C.set_off[o0 + o] - a;
        if (c->reach.bound_x.size() < (size_t)total) {
            c->reach.bound_x.resize((size_t)total);
            c->reach.bound_y.resize((size_t)total);
        }
        std::copy(C.set_x.begin() + a, C.set_x.begin() + a + total, c->reach.bound_x.begin());
        std::copy(C.set_y.begin() + a, C.set_y.begin() + a + total, c->reach.bound_y.begin());
        adopt_bounded_sets(c->sc, c->reach, all_steps);
    }
    if (!any_couples_by_sets(members, who)) return PDMPC_OK;
    S.prep_calls[1] += 1;
    rc = pdmpc_bounded_set_coupling_grouped(h, (int32_t)who.size(), C.group_offset.data(), C.adjacency.data(), nullptr);
    if (rc) return cfail(nullptr, rc, std::string("pdmpc_bounded_set_coupling_grouped: ") + pdmpc_last_error());
    scatter_blocks(members, C);
    return PDMPC_OK;
}
// ... without a handle: every member's own bounding on the host twin (on its own table of local hulls), then the grouped host twin of
// the coupler on the members' step-Hp sets
inline int bound_on_host(pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who) {
    if (who.empty()) return PDMPC_OK;
    PrepScratch::Call& C = S.call;
    for (int m : who) {
        pdmpc_controller* c = members[m];
        const bool all_steps = S.prep[(size_t)m].reach_parallel;
        lanelet_polygons(c->sc, c->in, c->reach);
        const pdmpc_polygon_set lan = view_polygons(c->reach.lan_off, c->reach.lan_x, c->reach.lan_y), local = view_polygons(c->sc.reach_off, c->sc.reach_x, c->sc.reach_y);
        c->reach.bound_off.assign((size_t)c->sc.n * (all_steps ? c->sc.Hp : 1) + 1, 0);
        S.prep_calls[0] += 1;
        const int rc = with_room(c->reach.bound_x, c->reach.bound_y, [&]() { return (int64_t)c->reach.bound_off.back(); }, exactly, [&](int32_t cap, double* ox, double* oy) {
            return pdmpc_bound_reachable_sets_host((int32_t)c->sc.trim_speed.size(), c->sc.Hp, &local, c->sc.n, c->tr.mx.data(), c->tr.my.data(), c->reach.cos_yaw.data(), c->reach.sin_yaw.data(),
                                                   c->in.trims.data(), &lan, all_steps, cap, c->reach.bound_off.data(), ox, oy, nullptr);
        });
        if (rc) return cfail(c, rc, "pdmpc_bound_reachable_sets_host failed");
        adopt_bounded_sets(c->sc, c->reach, all_steps);
    }
    if (!any_couples_by_sets(members, who)) return PDMPC_OK;
    gather(members, C, who, false);
    C.set_off.assign(1, 0);
    C.set_x.clear();
    C.set_y.clear();
    for (int m : who) {
        pdmpc_controller* c = members[m];
        const int sets_each = S.prep[(size_t)m].reach_parallel ? c->sc.Hp : 1;
        for (int v = 0; v < c->sc.n; ++v) {
            const int o = v * sets_each + sets_each - 1, a = c->reach.bound_off[o], cnt = c->reach.bound_off[o + 1] - a;
            C.set_x.insert(C.set_x.end(), c->reach.bound_x.begin() + a, c->reach.bound_x.begin() + a + cnt);
            C.set_y.insert(C.set_y.end(), c->reach.bound_y.begin() + a, c->reach.bound_y.begin() + a + cnt);
            C.set_off.push_back((int32_t)C.set_x.size());
        }
    }
    C.set_x.push_back(0.0);
    C.set_y.push_back(0.0);
    const pdmpc_polygon_set ps = view_polygons(C.set_off, C.set_x, C.set_y);
    S.prep_calls[1] += 1;
    const int rc = pdmpc_polygon_set_coupling_grouped_host(&ps, (int32_t)who.size(), C.group_offset.data(), C.adjacency.data(), nullptr);
    if (rc) return cfail(nullptr, rc, "pdmpc_polygon_set_coupling_grouped_host failed");
    scatter_blocks(members, C);
    return PDMPC_OK;
}
// the coupler on the unbounded step-Hp hulls of the members `who` (ReachableSetCoupler.m:5-56), grouped by member: with a handle the
// members share its table of local hulls (as they share its automaton) ...
inline int couple_hulls_on_device(pdmpc_handle* h, pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who) {
    if (who.empty()) return PDMPC_OK;
    PrepScratch::Call& C = S.call;
    gather(members, C, who, false);
    S.prep_calls[2] += 1;
    const int rc = pdmpc_reachable_set_coupling_grouped(h, (int32_t)who.size(), C.group_offset.data(), C.x.data(), C.y.data(), C.cos_yaw.data(), C.sin_yaw.data(), C.trim.data(),
                                                        C.adjacency.data(), nullptr);
    if (rc) return cfail(nullptr, rc, std::string("pdmpc_reachable_set_coupling_grouped: ") + pdmpc_last_error());
    scatter_blocks(members, C);
    return PDMPC_OK;
}
// ... without one, members that hold the same table share a call of the grouped host twin
inline int couple_hulls_on_host(pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who) {
    PrepScratch::Call& C = S.call;
    std::vector<int> rest = who, same, other;
    while (!rest.empty()) {
        const pdmpc_controller* c0 = members[rest[0]];
        same.clear();
        other.clear();
        for (int m : rest) {
            const pdmpc_controller* c = members[m];
            (c->sc.reach_off == c0->sc.reach_off && c->sc.reach_x == c0->sc.reach_x && c->sc.reach_y == c0->sc.reach_y ? same : other).push_back(m);
        }
        gather(members, C, same, false);
        const pdmpc_polygon_set ps = view_polygons(c0->sc.reach_off, c0->sc.reach_x, c0->sc.reach_y);
        S.prep_calls[2] += 1;
        const int rc = pdmpc_reachable_set_coupling_grouped_host((int32_t)c0->sc.trim_speed.size(), c0->sc.Hp, &ps, (int32_t)same.size(), C.group_offset.data(), C.x.data(),
                                                                 C.y.data(), C.cos_yaw.data(), C.sin_yaw.data(), C.trim.data(), C.adjacency.data(), nullptr);
        if (rc) return cfail(nullptr, rc, "pdmpc_reachable_set_coupling_grouped_host failed");
        scatter_blocks(members, C);
        rest = other;
    }
    return PDMPC_OK;
}

// the inputs of the future collision assessment of the members `who` (their adjacency is there) as ONE grouped call takes them: every
// member with its own coupled pairs, scenario obstacles and vehicle sizes, the reference points member after member
inline int gather_fca(pdmpc_controller* const* members, PrepScratch::Fca& F, const std::vector<int>& who) {
    F.groups.assign(who.size(), pdmpc_fca_group());
    F.obstacles.resize(who.size());
    for (auto* v : {&F.x, &F.y, &F.cos_yaw, &F.sin_yaw}) v->clear();
    size_t n = 0;
    for (size_t g = 0; g < who.size(); ++g) {
        pdmpc_controller* c = members[who[g]];
        if (!fca_inputs(c->sc, c->in, c->fca)) return cfail(c, PDMPC_ERR_INVALID, "FCA priorities need Hp >= 2 (calculate_yaw needs two reference points)");
        F.x.insert(F.x.end(), c->fca.x.begin(), c->fca.x.end());
        F.y.insert(F.y.end(), c->fca.y.begin(), c->fca.y.end());
        F.cos_yaw.insert(F.cos_yaw.end(), c->fca.cos_yaw.begin(), c->fca.cos_yaw.end());
        F.sin_yaw.insert(F.sin_yaw.end(), c->fca.sin_yaw.begin(), c->fca.sin_yaw.end());
        F.obstacles[g] = view_polygons(c->fca.obst_off, c->fca.obst_x, c->fca.obst_y);
        pdmpc_fca_group& G = F.groups[g];
        G.n = c->sc.n;
        G.n_pairs = (int32_t)(c->fca.pairs.size() / 2);
        G.pairs = c->fca.pairs.data();
        G.obstacles = &F.obstacles[g];
        G.dynamic_rows = nullptr;
        G.length = c->sc.cfg.vehicle_length;
        G.width = c->sc.cfg.vehicle_width;
        G.offset = c->sc.cfg.offset;
        n += (size_t)c->sc.n;
    }
    F.collisions.assign(n, 0);
    F.priorities.assign(n, 0);
    return PDMPC_OK;
}

// ---- human-driven vehicles: the traffic-info stage over all members.  With a handle (on a group: its rank 0, which h
// is) the members with HDVs are the groups of ONE pdmpc_hdv_traffic_grouped (hdv_grouped_host.hpp: a further call per
// PDMPC_HDV_MAP_SLOTS distinct maps or PDMPC_HDV_GROUPED_MAX_VEHICLES HDVs); members whose maps are equal share a map slot of the handle,
// and a map that is still resident -- the slot's generation as the member noted it, or the handle's byte-for-byte check -- is not
// uploaded again.  Without a handle every such member takes the solo path.  (step_hdv.hpp: both paths, on the members' views.)
inline int hdv_traffic_stage(pdmpc_handle* h, pdmpc_controller* const* members, size_t M, PrepScratch& S) {
    S.hdv_calls[0] = S.hdv_calls[1] = 0;
    std::vector<HdvMember> view(M);
    std::vector<int32_t> n_hdv(M, 0);
    std::vector<uint8_t> drives(M, 0);
    std::string why;
    for (size_t m = 0; m < M; ++m) {
        pdmpc_controller* c = members[m];
        view[m] = HdvMember{&c->hdv, c->sc.n, c->sc.Hp, c->sc.cfg.dt_seconds, c->tr.mx.data(), c->tr.my.data(), c->in.current_lanelet.data()};
        n_hdv[m] = c->hdv.n;
        if (!c->hdv.n) continue;
        drives[m] = hdv_begin_build(c->hdv) ? 1 : 0;
        if (!c->hdv.measured) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_measurements before the first step with HDVs");
        if (h) continue;
        S.hdv_calls[0] += 1;
        if (const int rc = hdv_solo_step(view[m], drives[m] != 0, &why)) return cfail(c, rc, why);
    }
    if (!h) return PDMPC_OK;
    std::vector<HdvBatch> batches = hdv_split_batches((int)M, n_hdv.data(), [&](int a, int b) { return same_hdv_map(members[a]->hdv, members[b]->hdv); });
    std::vector<HdvSlotNote> note(M);
    int64_t generation[PDMPC_HDV_MAP_SLOTS];
    auto read_generations = [&]() {
        for (int s = 0; s < PDMPC_HDV_MAP_SLOTS; ++s)
            if (const int rc = pdmpc_hdv_map_slot_state(h, s, &generation[s], nullptr, nullptr)) return cfail(nullptr, rc, pdmpc_last_error());
        return (int)PDMPC_OK;
    };
    // ONE call: the drive launch in front of the five (x, y, cos_yaw, sin_yaw of the members that drive are written) if a member drives
    auto device_call = [h](HdvCallScratch& C, bool any_drives) {
        const int32_t G = (int32_t)C.n_rows.size(), room = (int32_t)C.set_x.size();
        if (any_drives)
            return pdmpc_hdv_drive_traffic_grouped(h, G, C.slot.data(), C.hdv_offset.data(), C.cav_offset.data(), C.drives.data(), C.route_off.data(), C.route_id.data(),
                                                   C.route_closed.data(), C.seg.data(), C.u.data(), C.v_des.data(), C.params.data(), C.dt.data(), C.new_seg.data(),
                                                   C.new_u.data(), C.speed.data(), C.gap.data(), C.x.data(), C.y.data(), C.cos_yaw.data(), C.sin_yaw.data(), C.trim.data(),
                                                   C.tile_dx.data(), C.tile_dy.data(), C.cav_x.data(), C.cav_y.data(), C.cav_lanelet.data(), C.cav_tile_dx.data(),
                                                   C.cav_tile_dy.data(), C.closest_off.data(), C.closest_idx.data(), room, C.n_rows.data(), C.row_hdv.data(), C.set_off.data(),
                                                   C.set_base.data(), C.set_x.data(), C.set_y.data(), C.set_flags.data(), C.adjacency.data());
        return pdmpc_hdv_traffic_grouped(h, G, C.slot.data(), C.hdv_offset.data(), C.cav_offset.data(), C.x.data(), C.y.data(), C.cos_yaw.data(), C.sin_yaw.data(), C.trim.data(),
                                         C.tile_dx.data(), C.tile_dy.data(), C.cav_x.data(), C.cav_y.data(), C.cav_lanelet.data(), C.cav_tile_dx.data(), C.cav_tile_dy.data(),
                                         C.closest_off.data(), C.closest_idx.data(), room, C.n_rows.data(), C.row_hdv.data(), C.set_off.data(), C.set_base.data(), C.set_x.data(),
                                         C.set_y.data(), C.set_flags.data(), C.adjacency.data());
    };
    for (HdvBatch& B : batches) {
        if (const int rc = read_generations()) return rc;
        for (int m : B.members) note[(size_t)m] = HdvSlotNote{members[m]->hdv.map_slot, members[m]->hdv.map_generation};
        hdv_assign_slots(B, note.data(), generation, [&](int slot, int m) {
            int32_t holds = 0;
            (void)hdv_with_map(members[m]->hdv, members[m]->sc.Hp, [&](auto... map) { return pdmpc_hdv_map_slot_holds(h, slot, map..., &holds); });
            return holds != 0;
        });
        for (size_t d = 0; d < B.maps.size(); ++d) {
            if (!B.upload[d]) continue;
            S.hdv_calls[1] += 1;
            pdmpc_controller* c = members[B.maps[d]];
            if (const int rc = hdv_with_map(c->hdv, c->sc.Hp, [&](auto... map) { return pdmpc_upload_hdv_map_slot(h, B.slot[d], map...); }))
                return cfail(c, rc, std::string("pdmpc_upload_hdv_map_slot: ") + pdmpc_last_error());
        }
        if (const int rc = read_generations()) return rc;
        for (size_t i = 0; i < B.members.size(); ++i) {
            HdvTraffic& H = members[B.members[i]]->hdv;
            H.map_slot = B.slot[(size_t)B.map_of[i]];
            H.map_generation = generation[H.map_slot];
        }
        S.hdv_calls[0] += 1;
        bool any_drives = false;
        if (const int rc = hdv_gather_batch(view.data(), B, drives.data(), S.hdv, &any_drives)) return cfail(nullptr, rc, "pdmpc_hdv_grouped_layout_host failed");
        if (const int rc = hdv_call_batch(S.hdv, any_drives, device_call)) return cfail(nullptr, rc, std::string("pdmpc_hdv_traffic_grouped: ") + pdmpc_last_error());
        hdv_scatter_batch(view.data(), B, S.hdv);
    }
    return PDMPC_OK;
}

// The step problems of M members (of one Hp, all on the handle h or all without one), built with ONE step preparation for all of them:
// with a handle the grouped device calls, without one the host twins.  This is the only place that asks which.  batch.n_perm > 0: every
// member's explorative batch of n_perm prioritizations behind its step (pdmpc_controller_explore_build's statements, in its order).
// batch.max_instances > 0: every member's optimal-priority batch behind the steps -- ONE enumeration of the unique prioritizations of all
// members' coupling graphs, then pdmpc_controller_optimal_build's instances per member.
inline int build_members(pdmpc_handle* h, pdmpc_controller* const* members, size_t M, BatchKind batch, PrepScratch& S) {
    const int n_perm = batch.n_perm;
    struct ExploringAll {  // (the members' memos of the obstacle sets are on while their prioritizations are assembled)
        pdmpc_controller* const* members;
        size_t M;
        bool on;
        ExploringAll(pdmpc_controller* const* ms, size_t n, bool o) : members(ms), M(n), on(o) { set(on); }
        ~ExploringAll() { set(false); }
        void set(bool v) {
            for (size_t m = 0; on && m < M; ++m) members[m]->as.exploring = v;
        }
    } exploring(members, M, n_perm > 0 || batch.max_instances > 0);
    S.prep.assign(M, StepPrep());
    std::fill(S.prep_calls, S.prep_calls + 4, 0);
    S.prio.calls = 0;
    for (size_t m = 0; m < M; ++m)
        if (const int rc = begin_step(members[m], S.prep[m])) return rc;
    if (const int rc = hdv_traffic_stage(h, members, M, S)) return rc;
    // who takes part in which grouped call: bounded (step Hp only / every step: one bounding call each) or the plain hulls
    std::vector<int> bounded_last, bounded_all, hulls;
    for (size_t m = 0; m < M; ++m) {
        const StepPrep& P = S.prep[m];
        if (P.bounded)
            (P.reach_parallel ? bounded_all : bounded_last).push_back((int)m);
        else if (members[m]->sc.cfg.coupling == PDMPC_COUPLING_REACHABLE_SET)
            hulls.push_back((int)m);
    }
    int rc = PDMPC_OK;
    if (h) {
        rc = bound_on_device(h, members, S, bounded_last, false);
        if (!rc) rc = bound_on_device(h, members, S, bounded_all, true);
        if (!rc) rc = couple_hulls_on_device(h, members, S, hulls);
    } else {
        bounded_last.insert(bounded_last.end(), bounded_all.begin(), bounded_all.end());
        std::sort(bounded_last.begin(), bounded_last.end());
        rc = bound_on_host(members, S, bounded_last);
        if (!rc) rc = couple_hulls_on_host(members, S, hulls);
    }
    if (rc) return rc;
    std::vector<int> assessed;  // the members with FCA priorities: assessed together once every member's adjacency is there
    for (size_t m = 0; m < M; ++m) {
        couple(members[m]->sc, members[m]->tr, members[m]->in);
        if (members[m]->sc.cfg.priority_strategy == PDMPC_PRIORITY_FCA) assessed.push_back((int)m);
    }
    PrepScratch::Fca& F = S.fca;
    if (!assessed.empty()) {
        if ((rc = gather_fca(members, F, assessed))) return rc;
        const int Hp = members[0]->sc.Hp;
        S.prep_calls[3] += 1;
        rc = h ? pdmpc_fca_collisions_grouped(h, (int32_t)F.groups.size(), F.groups.data(), Hp, F.x.data(), F.y.data(), F.cos_yaw.data(), F.sin_yaw.data(), F.collisions.data(),
                                              F.priorities.data())
               : pdmpc_fca_collisions_grouped_host((int32_t)F.groups.size(), F.groups.data(), Hp, F.x.data(), F.y.data(), F.cos_yaw.data(), F.sin_yaw.data(), F.collisions.data(),
                                                   F.priorities.data());
        if (rc) return cfail(nullptr, rc, h ? std::string("pdmpc_fca_collisions_grouped: ") + pdmpc_last_error() : "pdmpc_fca_collisions_grouped_host failed");
    }
    for (size_t m = 0, g = 0, v0 = 0; m < M; ++m) {
        pdmpc_controller* c = members[m];
        const bool fca = g < assessed.size() && assessed[g] == (int)m;
        rc = finish_step(c, fca ? F.collisions.data() + v0 : nullptr, fca ? F.priorities.data() + v0 : nullptr);
        if (fca) {
            v0 += (size_t)c->sc.n;
            ++g;
        }
        if (!rc && n_perm > 0) rc = permute_instances(c, n_perm, (uint32_t)c->tr.k);  // RandStream("mt19937ar", Seed = obj.k) (:249)
        if (rc) return rc;
    }
    if (batch.max_instances < 1) return PDMPC_OK;
    // every unique prioritization of every member's coupling graph: one call whatever M is
    PrepScratch::Prio& Q = S.prio;
    Q.group_n.resize(M);
    Q.adjacency.resize(M);
    Q.max_out.assign(M, batch.max_instances);
    Q.n_out.assign(M, 0);
    size_t rows = 0;
    for (size_t m = 0; m < M; ++m) {
        Q.group_n[m] = members[m]->sc.n;
        Q.adjacency[m] = members[m]->in.adjacency.data();
        rows += (size_t)batch.max_instances * members[m]->sc.n;
    }
    Q.masks.resize(M * (size_t)batch.max_instances);
    Q.priorities.resize(rows);
    Q.calls += 1;
    rc = h ? pdmpc_unique_priorities_grouped(h, (int32_t)M, Q.group_n.data(), Q.adjacency.data(), Q.max_out.data(), Q.n_out.data(), Q.masks.data(), Q.priorities.data())
           : pdmpc_unique_priorities_grouped_host((int32_t)M, Q.group_n.data(), Q.adjacency.data(), Q.max_out.data(), Q.n_out.data(), Q.masks.data(), Q.priorities.data());
    if (rc) return h ? cfail(nullptr, rc, pdmpc_last_error()) : rc;
    const uint32_t* masks = Q.masks.data();
    const int32_t* priorities = Q.priorities.data();
    for (size_t m = 0; m < M; ++m) {
        if ((rc = optimal_instances(members[m], Q.n_out[m], masks, priorities))) return rc;
        masks += Q.n_out[m];
        priorities += Q.n_out[m] * members[m]->sc.n;
    }
    return PDMPC_OK;
}
}  // namespace
