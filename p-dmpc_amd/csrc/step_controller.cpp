// step_controller.cpp — the caller's side of the optimizer boundary, natively: one MPC time step of the prioritized
// sequential controller around pdmpc_plan_step.  Host code only (no device code in this file).
//
// What it restates (file:line relative to the reference root), the C++ twin of p-dmpc_amd/pdmpc/controller.py, in stages, each a header
// that names only the ones before it and says at its head what it restates (`make host-parts` compiles each alone):
// step_types.hpp (the records), step_inputs.hpp (what a step reads of the traffic), step_priorities.hpp (couplings -> a prioritization),
// step_state.hpp (the controller as the parts that are written together), step_assembly.hpp (a member's StepProblem), step_batch.hpp (the
// batches of prioritizations and the choice among their plans), step_centralized.hpp (centralized control: the joint problem).  This file: the step preparation over a span of members (build_members),
// planning a built problem (plan_built), the steps and their loops, the sweep, every entry point of the C ABI, and
//   exhaustion, fallbacks     handle_graph_search_exhaustion / plan_fallback (:568-616, 678-718), check_others_fallback (:623-676),
//                             HighLevelController.handle_others_fallback (HighLevelController.m:449-463)
//   plant                     Simulation.apply (plant/Simulation.m:86-100)
// Every floating-point expression keeps the order of the Python twin (which keeps the reference's), and both call the
// same libm, so the step problems the two build are bit-identical (tests/test_native_controller.py).
#include <algorithm>
#include <cassert>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pdmpc.h"
#include "hdv_drive_host.hpp"    // the checks of the HDV drivers' parameters (host only)
#include "hdv_grouped_host.hpp"  // the batches of the HDV traffic stage (host only)
#include "step_types.hpp"  // the stages, in their order
#include "step_inputs.hpp"
#include "step_priorities.hpp"
#include "step_state.hpp"
#include "step_assembly.hpp"
#include "step_batch.hpp"
#include "step_centralized.hpp"

namespace {

// ---- the shared paths of the steps below (templates: outside the extern "C" block)
// A bounding call that writes its sets into (x, y) of capacity x.size() and their offsets into off: after PDMPC_ERR_CAPACITY it is
// made once more with the room it asked for (off.back()).  The one capacity retry of the step preparation.
template <class Bound>
int bound_with_room(std::vector<int32_t>& off, std::vector<double>& x, std::vector<double>& y, Bound&& bound) {
    int rc = bound((int32_t)x.size(), x.empty() ? nullptr : x.data(), y.empty() ? nullptr : y.data());
    if (rc == PDMPC_ERR_CAPACITY && off.back() > (int32_t)x.size()) {
        x.resize((size_t)off.back());
        y.resize((size_t)off.back());
        rc = bound((int32_t)x.size(), x.data(), y.data());
    }
    return rc;
}

// the twin over a group of each backend call a built problem is planned with
using PlanRecords = int (*)(pdmpc_handle*, int32_t, const pdmpc_vehicle_in*, const int32_t*, const int32_t*, const pdmpc_polygon_set*, pdmpc_vehicle_out*);
using PlanLean = int (*)(pdmpc_handle*, int32_t, const pdmpc_vehicle_in*, const int32_t*, const int32_t*, const pdmpc_polygon_set*, int32_t*, double*);
using PlanChosen = int (*)(pdmpc_handle*, int32_t, const pdmpc_vehicle_in*, const int32_t*, const int32_t*, const pdmpc_polygon_set*, const pdmpc_choice*, int32_t*, double*,
                           pdmpc_vehicle_out*);
inline auto group_twin(PlanRecords) { return &pdmpc_group_plan_step; }
inline auto group_twin(PlanLean) { return &pdmpc_group_plan_step_lean; }
inline auto group_twin(PlanChosen) { return &pdmpc_group_plan_step_chosen; }

// Plans a problem that has been built -- a controller's, its batch of prioritizations or a sweep's -- on `on`: last step's work as the
// expected work of this one (pops_of(slot) + 1: heavy searches are dispatched first; weigh = false: no step has been planned yet), the
// slots' seeds for the next pack if the optimizer is the sampled one (a sampled bank; nothing for the graph search), the backend call
// `call` with the problem's arrays and `rest` (pdmpc_plan_step, _lean or _chosen), and its parts (pdmpc_last_call_timing) into timing[1..3].
// Over a group the same through the call's twin: the expected work is the partition's weights too, the seeds travel with the
// sub-problems, and the parts are pdmpc_group_last_timing's (pack incl. the partition; enqueue; wait and read-back).
template <class Pops, class Call, class... Rest>
int plan_built(const PlanTarget& on, StepProblem& P, bool weigh, Pops&& pops_of, int optimizer, double* timing, Call call, Rest... rest) {
    pdmpc_handle* h = on.h;
    if (weigh) {
        const int N = P.n();
        P.weights.resize((size_t)N);
        for (int s = 0; s < N; ++s) P.weights[(size_t)s] = pops_of(s) + 1.0;
        if (!on.g) (void)pdmpc_set_step_weights(h, N, P.weights.data());
    }
    if (on.g) {
        if (optimizer == PDMPC_OPTIMIZER_SAMPLED)
            if (const int rc = pdmpc_group_set_step_seeds(on.g, (int32_t)P.seeds.size(), P.seeds.data())) return cfail(nullptr, rc, pdmpc_last_error());
        if (const int rc = P.plan_on_group(group_twin(call), on.g, weigh ? P.weights.data() : nullptr, on.mode, rest...)) return cfail(nullptr, rc, pdmpc_last_error());
        double ms[6] = {0, 0, 0, 0, 0, 0};
        if (pdmpc_group_last_timing(on.g, ms) == PDMPC_OK) {
            timing[1] = ms[1] + ms[2];
            timing[2] = ms[3];
            timing[3] = ms[4] + ms[5];
        }
        return PDMPC_OK;
    }
    if (optimizer == PDMPC_OPTIMIZER_SAMPLED)
        if (const int rc = pdmpc_set_step_seeds(h, (int32_t)P.seeds.size(), P.seeds.data())) return cfail(nullptr, rc, pdmpc_last_error());
    if (const int rc = P.plan(call, h, rest...)) return cfail(nullptr, rc, pdmpc_last_error());
    double us[3] = {0, 0, 0};
    if (pdmpc_last_call_timing(h, us) == PDMPC_OK)
        for (int i = 0; i < 3; ++i) timing[1 + i] = us[i] * 1e-3;
    return PDMPC_OK;
}
// n_steps closed-loop time steps in one call; ms[i] (may be NULL) receives the wall time of step i: build + pack + launch + fetch +
// apply, everything a caller of the boundary pays per MPC step
template <class Step>
int timed_steps(int32_t n_steps, double* ms, Step&& step) {
    for (int i = 0; i < n_steps; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        if (const int rc = step()) return rc;
        if (ms) ms[i] = ms_since(t0);
    }
    return PDMPC_OK;
}

// ---- ONE step preparation over a span of members: a sweep's members, or the one controller that steps alone
// the poses of the members `who` one after the other (and their lanelet polygons: with_lanelets)
void gather(pdmpc_controller* const* members, PrepScratch::Call& C, const std::vector<int>& who, bool with_lanelets) {
    C.who = who;
    C.group_offset.assign(1, 0);
    C.x.clear();
    C.y.clear();
    C.cos_yaw.clear();
    C.sin_yaw.clear();
    C.trim.clear();
    C.lan_off.assign(1, 0);
    C.lan_x.clear();
    C.lan_y.clear();
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
void scatter_blocks(pdmpc_controller* const* members, const PrepScratch::Call& C) {
    size_t block = 0;
    for (int m : C.who) {
        pdmpc_controller* c = members[m];
        const size_t nn = (size_t)c->sc.n * c->sc.n;
        if (c->sc.cfg.coupling == PDMPC_COUPLING_REACHABLE_SET) c->in.adjacency.assign(C.adjacency.begin() + block, C.adjacency.begin() + block + nn);
        block += nn;
    }
}
bool any_couples_by_sets(pdmpc_controller* const* members, const std::vector<int>& who) {
    for (int m : who)
        if (members[m]->sc.cfg.coupling == PDMPC_COUPLING_REACHABLE_SET) return true;
    return false;
}

// lanelet bounding of the members `who` (one all_steps for all of them) in ONE device call on the concatenated vehicles, then the
// coupler on the bounded step-Hp sets (on the device they are still there), grouped by member
int bound_on_device(pdmpc_handle* h, pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who, bool all_steps) {
    if (who.empty()) return PDMPC_OK;
    PrepScratch::Call& C = S.call;
    gather(members, C, who, true);
    const int Hp = members[who[0]]->sc.Hp, sets_each = all_steps ? Hp : 1, n = C.group_offset.back();
    const pdmpc_polygon_set lan = view_polygons(C.lan_off, C.lan_x, C.lan_y);
    C.set_off.assign((size_t)n * sets_each + 1, 0);
    S.prep_calls[0] += 1;
    int rc = bound_with_room(C.set_off, C.set_x, C.set_y, [&](int32_t cap, double* ox, double* oy) {
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
int bound_on_host(pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who) {
    if (who.empty()) return PDMPC_OK;
    PrepScratch::Call& C = S.call;
    for (int m : who) {
        pdmpc_controller* c = members[m];
        const bool all_steps = S.prep[(size_t)m].reach_parallel;
        lanelet_polygons(c->sc, c->in, c->reach);
        const pdmpc_polygon_set lan = view_polygons(c->reach.lan_off, c->reach.lan_x, c->reach.lan_y), local = view_polygons(c->sc.reach_off, c->sc.reach_x, c->sc.reach_y);
        c->reach.bound_off.assign((size_t)c->sc.n * (all_steps ? c->sc.Hp : 1) + 1, 0);
        S.prep_calls[0] += 1;
        const int rc = bound_with_room(c->reach.bound_off, c->reach.bound_x, c->reach.bound_y, [&](int32_t cap, double* ox, double* oy) {
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
int couple_hulls_on_device(pdmpc_handle* h, pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who) {
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
int couple_hulls_on_host(pdmpc_controller* const* members, PrepScratch& S, const std::vector<int>& who) {
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
int gather_fca(pdmpc_controller* const* members, PrepScratch::Fca& F, const std::vector<int>& who) {
    F.groups.assign(who.size(), pdmpc_fca_group());
    F.obstacles.resize(who.size());
    F.x.clear();
    F.y.clear();
    F.cos_yaw.clear();
    F.sin_yaw.clear();
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
// uploaded again.  Without a handle every such member calls the host twin.
template <class T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}
bool same_hdv_map(const HdvTraffic& A, const HdvTraffic& B) {
    return &A == &B || (A.n_trims == B.n_trims && same_bytes(A.lan_off, B.lan_off) && same_bytes(A.succ_off, B.succ_off) && same_bytes(A.succ_idx, B.succ_idx) &&
                        same_bytes(A.rel, B.rel) && same_bytes(A.local_off, B.local_off) && same_bytes(A.left_x, B.left_x) && same_bytes(A.left_y, B.left_y) &&
                        same_bytes(A.right_x, B.right_x) && same_bytes(A.right_y, B.right_y) && same_bytes(A.local_x, B.local_x) && same_bytes(A.local_y, B.local_y));
}
// the room a member's results need (what its own traffic call would size)
void hdv_size_results(pdmpc_controller* c) {
    HdvTraffic& H = c->hdv;
    const size_t lists = (size_t)H.n * PDMPC_HDV_MAX_CHAINS;
    H.closest_off.assign((size_t)H.n + 1, 0);
    H.closest_idx.resize(lists);
    H.row_hdv.resize(lists);
    H.set_off.assign(lists * c->sc.Hp + 1, 0);
    H.set_flags.resize(lists * c->sc.Hp);
    H.adjacency.assign((size_t)c->sc.n * H.n, 0);
    if (H.set_x.size() < 4096) {
        H.set_x.resize(4096);
        H.set_y.resize(4096);
    }
}

int hdv_traffic_on_host(pdmpc_controller* c) {
    HdvTraffic& H = c->hdv;
    const int n = c->sc.n, Hp = c->sc.Hp;
    hdv_size_results(c);
    const pdmpc_polygon_set local = view_polygons(H.local_off, H.local_x, H.local_y);
    auto call = [&]() {
        return pdmpc_hdv_traffic_host((int32_t)H.lan_off.size() - 1, H.lan_off.data(), H.lan_off.data(), H.left_x.data(), H.left_y.data(), H.right_x.data(), H.right_y.data(),
                                      H.succ_off.data(), H.succ_idx.data(), H.rel.data(), H.n_trims, Hp, &local, H.n, H.x.data(), H.y.data(), H.cos_yaw.data(), H.sin_yaw.data(),
                                      H.trim.data(), H.tile_dx.data(), H.tile_dy.data(), n, c->tr.mx.data(), c->tr.my.data(), c->in.current_lanelet.data(), H.cav_tile_dx.data(),
                                      H.cav_tile_dy.data(), H.closest_off.data(), H.closest_idx.data(), (int32_t)H.set_x.size(), &H.n_rows, H.row_hdv.data(), H.set_off.data(),
                                      H.set_x.data(), H.set_y.data(), H.set_flags.data(), H.adjacency.data());
    };
    int rc = call();
    if (rc == PDMPC_ERR_CAPACITY && H.n_rows >= 0 && (size_t)H.set_off[(size_t)H.n_rows * Hp] > H.set_x.size()) {  // (the offsets size the second call)
        const size_t need = (size_t)H.set_off[(size_t)H.n_rows * Hp];
        H.set_x.resize(need + need / 4);
        H.set_y.resize(need + need / 4);
        rc = call();
    }
    if (rc) return cfail(c, rc, "pdmpc_hdv_traffic_host failed");
    H.gather(n, Hp);
    return PDMPC_OK;
}

// the yaw of the driven poses, for read-back only (the traffic passes read cos and sin as the driver step gave them)
void hdv_driven_yaw(HdvTraffic& H) {
    H.yaw.resize((size_t)H.n);
    for (int q = 0; q < H.n; ++q) H.yaw[(size_t)q] = std::atan2(H.sin_yaw[(size_t)q], H.cos_yaw[(size_t)q]);
}

// What a member's HDVs are measured as at this built step.  A recording: its next row.  Drivers: *drives = 1 if they move this step
// (every built step but the first after pdmpc_controller_set_hdv_drivers, whose measurement is the placement).
void hdv_begin_build(pdmpc_controller* c, bool* drives) {
    HdvTraffic& H = c->hdv;
    *drives = false;
    if (H.rec_T > 0) {
        H.rec_builds += 1;
        const size_t row = (size_t)(std::min(H.rec_builds, H.rec_T) - 1) * H.n;
        H.x.assign(H.rec_x.begin() + row, H.rec_x.begin() + row + H.n);
        H.y.assign(H.rec_y.begin() + row, H.rec_y.begin() + row + H.n);
        H.yaw.assign(H.rec_yaw.begin() + row, H.rec_yaw.begin() + row + H.n);
        H.cos_yaw.resize((size_t)H.n);
        H.sin_yaw.resize((size_t)H.n);
        for (int q = 0; q < H.n; ++q) {
            H.cos_yaw[(size_t)q] = std::cos(H.yaw[(size_t)q]);
            H.sin_yaw[(size_t)q] = std::sin(H.yaw[(size_t)q]);
        }
        H.measured = true;
    }
    if (H.driven) {
        H.driven_builds += 1;
        *drives = H.driven_builds > 1;
    }
}

// the driver step of one member on the host (pdmpc_hdv_drive_host), in front of its traffic call
int hdv_drive_on_host(pdmpc_controller* c) {
    HdvTraffic& H = c->hdv;
    const int rc = pdmpc_hdv_drive_host((int32_t)H.lan_off.size() - 1, H.lan_off.data(), H.lan_off.data(), H.left_x.data(), H.left_y.data(), H.right_x.data(), H.right_y.data(),
                                        H.succ_off.data(), H.succ_idx.data(), H.rel.data(), H.n, H.route_off.data(), H.route_id.data(), H.route_closed.data(), H.seg.data(),
                                        H.u.data(), H.tile_dx.data(), H.tile_dy.data(), H.v_des.data(), c->sc.n, c->tr.mx.data(), c->tr.my.data(), H.cav_tile_dx.data(),
                                        H.cav_tile_dy.data(), H.drive_params, c->sc.cfg.dt_seconds, H.new_seg.data(), H.new_u.data(), H.x.data(), H.y.data(), H.cos_yaw.data(),
                                        H.sin_yaw.data(), H.speed.data(), H.gap.data());
    if (rc) return cfail(c, rc, std::string("pdmpc_hdv_drive_host: ") + pdmpc_last_error());
    H.seg.swap(H.new_seg);
    H.u.swap(H.new_u);
    hdv_driven_yaw(H);
    return PDMPC_OK;
}

// the members of batch B (their maps are in the slots B.slot) as the groups of one call, and every member's blocks back into its own
// arrays, as its own call leaves them.  The capacity retry is here, once: the room is the last total and a quarter.
int hdv_call_for_batch(pdmpc_handle* h, pdmpc_controller* const* members, const HdvBatch& B, PrepScratch::Hdv& C, const std::vector<uint8_t>& drives_of) {
    const int G = (int)B.members.size(), Hp = members[B.members[0]]->sc.Hp;
    bool any_drives = false;
    for (auto* v : {&C.drives, &C.route_closed}) v->clear();
    for (auto* v : {&C.route_id, &C.seg_r, &C.seg_j}) v->clear();
    for (auto* v : {&C.u, &C.v_des, &C.params, &C.dt}) v->clear();
    C.route_off.assign(1, 0);
    for (auto* v : {&C.slot, &C.trim, &C.cav_lanelet}) v->clear();
    for (auto* v : {&C.x, &C.y, &C.cos_yaw, &C.sin_yaw, &C.tile_dx, &C.tile_dy, &C.cav_x, &C.cav_y, &C.cav_tile_dx, &C.cav_tile_dy}) v->clear();
    C.hdv_offset.assign(1, 0);
    C.cav_offset.assign(1, 0);
    auto append = [](auto& to, const auto& from, size_t count) { to.insert(to.end(), from.begin(), from.begin() + (ptrdiff_t)count); };
    for (int g = 0; g < G; ++g) {
        pdmpc_controller* c = members[B.members[(size_t)g]];
        const HdvTraffic& H = c->hdv;
        const size_t nh = (size_t)H.n, nc = (size_t)c->sc.n;
        C.slot.push_back(B.slot[(size_t)B.map_of[(size_t)g]]);
        append(C.x, H.x, nh);
        append(C.y, H.y, nh);
        append(C.cos_yaw, H.cos_yaw, nh);
        append(C.sin_yaw, H.sin_yaw, nh);
        append(C.trim, H.trim, nh);
        append(C.tile_dx, H.tile_dx, nh);
        append(C.tile_dy, H.tile_dy, nh);
        append(C.cav_x, c->tr.mx, nc);
        append(C.cav_y, c->tr.my, nc);
        append(C.cav_lanelet, c->in.current_lanelet, nc);
        append(C.cav_tile_dx, H.cav_tile_dx, nc);
        append(C.cav_tile_dy, H.cav_tile_dy, nc);
        C.hdv_offset.push_back((int32_t)C.x.size());
        C.cav_offset.push_back((int32_t)C.cav_x.size());
        // the drive pass: a member that does not move this step has no routes (the offsets do not move over its HDVs)
        const bool drives = drives_of[(size_t)B.members[(size_t)g]] != 0;
        any_drives = any_drives || drives;
        C.drives.push_back(drives ? 1 : 0);
        for (size_t q = 0; q < nh; ++q) {
            if (drives) C.route_id.insert(C.route_id.end(), H.route_id.begin() + H.route_off[q], H.route_id.begin() + H.route_off[q + 1]);
            C.route_off.push_back((int32_t)C.route_id.size());
            C.route_closed.push_back(drives ? H.route_closed[q] : 0);
            C.seg_r.push_back(drives ? H.seg[q] : 0);
            C.seg_j.push_back(drives ? H.seg[nh + q] : 0);
            C.u.push_back(drives ? H.u[q] : 0.0);
            C.v_des.push_back(drives ? H.v_des[q] : 0.0);
        }
        for (int q = 0; q < 4; ++q) C.params.push_back(drives ? H.drive_params[q] : 1.0);
        C.dt.push_back(c->sc.cfg.dt_seconds);
    }
    const size_t n_all = C.x.size();
    C.seg = C.seg_r;
    C.seg.insert(C.seg.end(), C.seg_j.begin(), C.seg_j.end());
    C.seg.push_back(0);
    C.route_id.push_back(0);
    C.new_seg.assign(2 * n_all + 1, 0);
    for (auto* v : {&C.new_u, &C.speed, &C.gap}) v->assign(n_all + 1, 0.0);
    for (auto* v : {&C.closest_at, &C.list_at, &C.set_offset_at, &C.set_at}) v->assign((size_t)G + 1, 0);
    C.adjacency_at.assign((size_t)G + 1, 0);
    if (const int rc = pdmpc_hdv_grouped_layout_host(G, C.hdv_offset.data(), C.cav_offset.data(), Hp, C.closest_at.data(), C.list_at.data(), C.set_offset_at.data(), C.set_at.data(),
                                                     C.adjacency_at.data()))
        return cfail(nullptr, rc, "pdmpc_hdv_grouped_layout_host failed");
    C.closest_off.assign((size_t)C.closest_at[(size_t)G], 0);
    C.closest_idx.assign((size_t)C.list_at[(size_t)G] + 1, 0);
    C.row_hdv.assign((size_t)C.list_at[(size_t)G] + 1, 0);
    C.set_off.assign((size_t)C.set_offset_at[(size_t)G], 0);
    C.set_flags.assign((size_t)C.set_at[(size_t)G] + 1, 0);
    C.adjacency.assign((size_t)C.adjacency_at[(size_t)G] + 1, 0);
    C.n_rows.assign((size_t)G, 0);
    C.set_base.assign((size_t)G + 1, 0);
    if (C.set_x.size() < 4096) {
        C.set_x.resize(4096);
        C.set_y.resize(4096);
    }
    auto call = [&]() {
        if (any_drives)  // ONE call: the drive launch in front of the five (x, y, cos_yaw, sin_yaw of the members that drive are written)
            return pdmpc_hdv_drive_traffic_grouped(h, G, C.slot.data(), C.hdv_offset.data(), C.cav_offset.data(), C.drives.data(), C.route_off.data(), C.route_id.data(),
                                                   C.route_closed.data(), C.seg.data(), C.u.data(), C.v_des.data(), C.params.data(), C.dt.data(), C.new_seg.data(),
                                                   C.new_u.data(), C.speed.data(), C.gap.data(), C.x.data(), C.y.data(), C.cos_yaw.data(), C.sin_yaw.data(), C.trim.data(),
                                                   C.tile_dx.data(), C.tile_dy.data(), C.cav_x.data(), C.cav_y.data(), C.cav_lanelet.data(), C.cav_tile_dx.data(),
                                                   C.cav_tile_dy.data(), C.closest_off.data(), C.closest_idx.data(), (int32_t)C.set_x.size(), C.n_rows.data(), C.row_hdv.data(),
                                                   C.set_off.data(), C.set_base.data(), C.set_x.data(), C.set_y.data(), C.set_flags.data(), C.adjacency.data());
        return pdmpc_hdv_traffic_grouped(h, G, C.slot.data(), C.hdv_offset.data(), C.cav_offset.data(), C.x.data(), C.y.data(), C.cos_yaw.data(), C.sin_yaw.data(), C.trim.data(),
                                         C.tile_dx.data(), C.tile_dy.data(), C.cav_x.data(), C.cav_y.data(), C.cav_lanelet.data(), C.cav_tile_dx.data(), C.cav_tile_dy.data(),
                                         C.closest_off.data(), C.closest_idx.data(), (int32_t)C.set_x.size(), C.n_rows.data(), C.row_hdv.data(), C.set_off.data(), C.set_base.data(),
                                         C.set_x.data(), C.set_y.data(), C.set_flags.data(), C.adjacency.data());
    };
    int rc = call();
    if (rc == PDMPC_ERR_CAPACITY && *std::min_element(C.n_rows.begin(), C.n_rows.end()) >= 0 && (size_t)C.set_base[(size_t)G] > C.set_x.size()) {  // (the totals size the second call)
        const size_t need = (size_t)C.set_base[(size_t)G];
        C.set_x.resize(need + need / 4);
        C.set_y.resize(need + need / 4);
        rc = call();
    }
    if (rc) return cfail(nullptr, rc, std::string("pdmpc_hdv_traffic_grouped: ") + pdmpc_last_error());
    for (int g = 0; g < G; ++g) {
        pdmpc_controller* c = members[B.members[(size_t)g]];
        HdvTraffic& H = c->hdv;
        if (C.drives[(size_t)g]) {  // where the drive pass left the member's HDVs
            const size_t h0 = (size_t)C.hdv_offset[(size_t)g], nh = (size_t)H.n;
            for (size_t q = 0; q < nh; ++q) {
                H.seg[q] = C.new_seg[h0 + q];
                H.seg[nh + q] = C.new_seg[n_all + h0 + q];
                H.u[q] = C.new_u[h0 + q];
                H.speed[q] = C.speed[h0 + q];
                H.gap[q] = C.gap[h0 + q];
                H.x[q] = C.x[h0 + q];
                H.y[q] = C.y[h0 + q];
                H.cos_yaw[q] = C.cos_yaw[h0 + q];
                H.sin_yaw[q] = C.sin_yaw[h0 + q];
            }
            hdv_driven_yaw(H);
        }
        hdv_size_results(c);
        const size_t rows = (size_t)C.n_rows[(size_t)g], sets = rows * Hp, nh = (size_t)H.n;
        const int32_t* so = C.set_off.data() + C.set_offset_at[(size_t)g];
        const size_t total = (size_t)so[sets];
        H.n_rows = (int32_t)rows;
        std::copy_n(C.closest_off.begin() + C.closest_at[(size_t)g], nh + 1, H.closest_off.begin());
        std::copy_n(C.closest_idx.begin() + C.list_at[(size_t)g], (size_t)H.closest_off[nh], H.closest_idx.begin());
        std::copy_n(C.row_hdv.begin() + C.list_at[(size_t)g], rows, H.row_hdv.begin());
        std::copy_n(so, sets + 1, H.set_off.begin());
        std::copy_n(C.set_flags.begin() + C.set_at[(size_t)g], sets, H.set_flags.begin());
        std::copy_n(C.adjacency.begin() + (ptrdiff_t)C.adjacency_at[(size_t)g], (size_t)c->sc.n * nh, H.adjacency.begin());
        if (H.set_x.size() < total) {
            H.set_x.resize(total + total / 4);
            H.set_y.resize(total + total / 4);
        }
        std::copy_n(C.set_x.begin() + C.set_base[(size_t)g], total, H.set_x.begin());
        std::copy_n(C.set_y.begin() + C.set_base[(size_t)g], total, H.set_y.begin());
        H.gather(c->sc.n, Hp);
    }
    return PDMPC_OK;
}

int hdv_traffic_stage(pdmpc_handle* h, pdmpc_controller* const* members, size_t M, PrepScratch& S) {
    S.hdv_calls[0] = S.hdv_calls[1] = 0;
    std::vector<int32_t> n_hdv(M, 0);
    std::vector<uint8_t> drives(M, 0);
    for (size_t m = 0; m < M; ++m) {
        pdmpc_controller* c = members[m];
        n_hdv[m] = c->hdv.n;
        if (c->hdv.n) {
            bool d = false;
            hdv_begin_build(c, &d);
            drives[m] = d ? 1 : 0;
        }
        if (c->hdv.n && !c->hdv.measured) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_measurements before the first step with HDVs");
        if (c->hdv.n && !h) {
            S.hdv_calls[0] += 1;
            if (drives[m])
                if (const int rc = hdv_drive_on_host(c)) return rc;
            if (const int rc = hdv_traffic_on_host(c)) return rc;
        }
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
    // a member's map as the handle's entry points take it
    auto with_map = [&](int m, auto&& f) {
        const HdvTraffic& H = members[m]->hdv;
        const pdmpc_polygon_set local = view_polygons(H.local_off, H.local_x, H.local_y);
        return f((int32_t)H.lan_off.size() - 1, H.lan_off.data(), H.lan_off.data(), H.left_x.data(), H.left_y.data(), H.right_x.data(), H.right_y.data(), H.succ_off.data(),
                 H.succ_idx.data(), H.rel.data(), (int32_t)H.n_trims, (int32_t)members[m]->sc.Hp, &local);
    };
    for (HdvBatch& B : batches) {
        if (const int rc = read_generations()) return rc;
        for (int m : B.members) note[(size_t)m] = HdvSlotNote{members[m]->hdv.map_slot, members[m]->hdv.map_generation};
        hdv_assign_slots(B, note.data(), generation, [&](int slot, int m) {
            int32_t holds = 0;
            (void)with_map(m, [&](auto... map) { return pdmpc_hdv_map_slot_holds(h, slot, map..., &holds); });
            return holds != 0;
        });
        for (size_t d = 0; d < B.maps.size(); ++d) {
            if (!B.upload[d]) continue;
            S.hdv_calls[1] += 1;
            if (const int rc = with_map(B.maps[d], [&](auto... map) { return pdmpc_upload_hdv_map_slot(h, B.slot[d], map...); }))
                return cfail(members[B.maps[d]], rc, std::string("pdmpc_upload_hdv_map_slot: ") + pdmpc_last_error());
        }
        if (const int rc = read_generations()) return rc;
        for (size_t i = 0; i < B.members.size(); ++i) {
            HdvTraffic& H = members[B.members[i]]->hdv;
            H.map_slot = B.slot[(size_t)B.map_of[i]];
            H.map_generation = generation[H.map_slot];
        }
        S.hdv_calls[0] += 1;
        if (const int rc = hdv_call_for_batch(h, members, B, S.hdv, drives)) return rc;
    }
    return PDMPC_OK;
}

// The step problems of M members (of one Hp, all on the handle h or all without one), built with ONE step preparation for all of them:
// with a handle the grouped device calls, without one the host twins.  This is the only place that asks which.  batch.n_perm > 0: every
// member's explorative batch of n_perm prioritizations behind its step (pdmpc_controller_explore_build's statements, in its order).
// batch.max_instances > 0: every member's optimal-priority batch behind the steps -- ONE enumeration of the unique prioritizations of all
// members' coupling graphs, then pdmpc_controller_optimal_build's instances per member.
int build_members(pdmpc_handle* h, pdmpc_controller* const* members, size_t M, BatchKind batch, PrepScratch& S) {
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

// ---- how a step ends that the controller takes alone
PlanTarget target_of(const pdmpc_controller* c) { return {c->h, c->group, c->group_mode}; }
// a failure inside a step the controller takes alone is the controller's error too (the global message has it either way)
int own(pdmpc_controller* c, int rc) {
    if (rc) c->err = g_cerr;
    return rc;
}
// the end of a step the controller takes alone: the records in c->out applied (timing[5]), and the step's parts added to the controller's sums
int apply_and_account(pdmpc_controller* c) {
    const auto t = std::chrono::steady_clock::now();
    const int rc = pdmpc_controller_apply(c, c->out.data());
    c->timing[5] = ms_since(t);
    for (int i = 0; i < 6; ++i) c->timing_sum[i] += c->timing[i];
    c->timing_steps += 1;
    return rc;
}
// a switch that is on for a scope: lean_explore (nobody looks at the plans that were not chosen: the explorative and optimal-priority
// steps keep them all, their *_run loops do not), as.exploring (the memos of the obstacle sets, while a step's prioritizations are assembled)
struct SwitchedOn {
    bool& flag;
    bool was;
    explicit SwitchedOn(bool& f) : flag(f), was(f) { flag = true; }
    ~SwitchedOn() { flag = was; }
};

// One time step over a batch of prioritizations (explorative or optimal): the batch is built, ONE launch plans all of it, `choose`
// picks per vehicle the instance it goes on with (c->x.chosen), and the chosen plans are applied.
int batch_step(pdmpc_controller* c, std::chrono::steady_clock::time_point t, bool follow_own, const BatchChoice& how) {
    c->timing[0] = ms_since(t);
    const int N = c->x.prob.n();
    auto plan = [&](auto call, auto... rest) {
        const int rc = plan_built(target_of(c), c->x.prob, c->tr.last_pops.size() == (size_t)c->sc.n, [&](int s) { return c->tr.last_pops[(size_t)c->x.vehicle[(size_t)s]]; }, c->optimizer,
                                  c->timing, call, rest...);
        t = std::chrono::steady_clock::now();
        return own(c, rc);
    };
    int rc = PDMPC_OK;
    if (c->lean_explore && c->device_choice) {
        // the closed loop keeps the chosen plans only, and the choice and their gather run on the device directly behind the search: ONE
        // call and one read-back (the chosen records, the choice and the cost table)
        c->x.out.clear();
        ChoiceLists& D = c->x.choice;
        how.describe(c, D);
        pick_chosen_plans(c, D, follow_own, how.graph_per_vehicle);
        c->x.choice_chosen.resize((size_t)D.n_graphs());
        c->x.choice_cost.resize((size_t)D.n_cells());
        c->out.resize((size_t)c->sc.n);
        const pdmpc_choice ch = D.view();
        rc = plan(pdmpc_plan_step_chosen, &ch, c->x.choice_chosen.data(), c->x.choice_cost.data(), c->out.data());
        if (rc) return rc;
        how.adopt(c, D, c->x.choice_chosen.data(), c->x.choice_cost.data(), follow_own);
    } else if (c->lean_explore) {
        // the closed loop keeps the chosen plans only (obj.iter = obj.iter_array_tmp{chosen_solution}, :157-158): status and final
        // cost of every plan come back for the choice, the chosen vehicles' records afterwards — not 2.9 KB for each of the N plans
        c->x.out.clear();
        c->x.status.resize((size_t)N);
        c->x.final_cost.resize((size_t)N);
        rc = plan(pdmpc_plan_step_lean, c->x.status.data(), c->x.final_cost.data());
        if (rc) return rc;
        rc = choose_on_host(c, how, c->x.status.data(), c->x.final_cost.data(), follow_own);
        if (rc) return rc;
        std::vector<int32_t> want((size_t)c->sc.n);
        for (int s = 0; s < c->sc.n; ++s) want[(size_t)s] = kept_slot_at(c, follow_own, s);
        c->out.resize((size_t)c->sc.n);
        rc = c->group ? pdmpc_group_fetch_records_at(c->group, c->sc.n, want.data(), c->out.data()) : pdmpc_fetch_records_at(c->h, c->sc.n, want.data(), c->out.data());
        if (rc) return cfail(c, rc, pdmpc_last_error());
    } else {
        c->x.out.resize((size_t)N);
        rc = plan(pdmpc_plan_step, c->x.out.data());
        if (rc) return rc;
        rc = choose_from_records(c, how, c->x.out.data(), N, follow_own);
        if (rc) return rc;
        gather_kept_records(c, follow_own);
    }
    c->timing[4] = ms_since(t);  // (from the backend call's return on)
    return apply_and_account(c);
}

// the parts of the last pdmpc_plan_joint on h (pdmpc_last_call_timing) into timing[1..3]
void joint_call_timing(pdmpc_handle* h, double* timing) {
    double us[3] = {0, 0, 0};
    if (pdmpc_last_call_timing(h, us) == PDMPC_OK)
        for (int i = 0; i < 3; ++i) timing[1 + i] = us[i] * 1e-3;
}

}  // namespace

extern "C" {

const char* pdmpc_controller_last_error(void) { return g_cerr.c_str(); }

int pdmpc_controller_create(pdmpc_handle* handle, const pdmpc_controller_config* cfg, const pdmpc_scenario* sc, pdmpc_controller** out) {
    if (!cfg || !sc || !out) return cfail(nullptr, PDMPC_ERR_INVALID, "null argument");
    if (sc->n_vehicles < 1 || cfg->Hp < 1 || cfg->Hp > PDMPC_HP_MAX || sc->n_trims < 1) return cfail(nullptr, PDMPC_ERR_INVALID, "bad sizes");
    if (cfg->priority_strategy < PDMPC_PRIORITY_CONSTANT || cfg->priority_strategy > PDMPC_PRIORITY_FCA) return cfail(nullptr, PDMPC_ERR_INVALID, "unknown priority strategy");
    if (cfg->weight_strategy < PDMPC_WEIGHT_DISTANCE || cfg->weight_strategy > PDMPC_WEIGHT_RANDOM) return cfail(nullptr, PDMPC_ERR_INVALID, "unknown weight strategy");
    if (handle) {
        // the backend reads Hp entries of every reference and writes one record per vehicle: a handle created for another
        // horizon or a smaller batch must not be driven by this controller
        pdmpc_config hc{};
        int32_t has_mpa = 0;
        if (pdmpc_get_config(handle, &hc, &has_mpa) != PDMPC_OK) return cfail(nullptr, PDMPC_ERR_INVALID, "bad backend handle");
        if (hc.Hp != cfg->Hp) return cfail(nullptr, PDMPC_ERR_INVALID, "the handle was created for another horizon (config.Hp) than the controller");
        if (hc.max_vehicles < sc->n_vehicles) return cfail(nullptr, PDMPC_ERR_CAPACITY, "the handle's max_vehicles is smaller than the scenario");
        if (!has_mpa) return cfail(nullptr, PDMPC_ERR_NO_MPA, "pdmpc_upload_mpa has not been called on the handle");
    }
    pdmpc_controller* c = new pdmpc_controller();
    c->h = handle;
    c->sc.cfg = *cfg;
    c->sc.n = sc->n_vehicles;
    c->sc.Hp = cfg->Hp;
    c->sc.trim_speed.assign(sc->trim_speed, sc->trim_speed + sc->n_trims);
    c->sc.trim_steering.assign(sc->trim_steering, sc->trim_steering + sc->n_trims);
    for (int v = 0; v < c->sc.n; ++v) {
        VehicleDef d;
        d.x_start = sc->x_start[v];
        d.y_start = sc->y_start[v];
        d.yaw_start = sc->yaw_start[v];
        d.reference_speed = sc->reference_speed[v];
        d.px.assign(sc->path_x + sc->path_offset[v], sc->path_x + sc->path_offset[v + 1]);
        d.py.assign(sc->path_y + sc->path_offset[v], sc->path_y + sc->path_offset[v + 1]);
        if (d.px.size() < 2) {
            delete c;
            return cfail(nullptr, PDMPC_ERR_INVALID, "a reference path needs at least two points");
        }
        if (sc->lanelets_offset) {
            d.lanelets_index.assign(sc->lanelets_index + sc->lanelets_offset[v], sc->lanelets_index + sc->lanelets_offset[v + 1]);
            d.points_index.assign(sc->points_index + sc->lanelets_offset[v], sc->points_index + sc->lanelets_offset[v + 1]);
        }
        d.is_loop = sc->is_loop ? sc->is_loop[v] != 0 : true;
        d.tile_dx = sc->tile_dx ? sc->tile_dx[v] : 0.0;
        d.tile_dy = sc->tile_dy ? sc->tile_dy[v] : 0.0;
        c->sc.veh.push_back(std::move(d));
    }
    for (int l = 0; l < sc->n_lanelets; ++l) {
        Poly a, b;
        a.x.assign(sc->left_x + sc->left_offset[l], sc->left_x + sc->left_offset[l + 1]);
        a.y.assign(sc->left_y + sc->left_offset[l], sc->left_y + sc->left_offset[l + 1]);
        b.x.assign(sc->right_x + sc->right_offset[l], sc->right_x + sc->right_offset[l + 1]);
        b.y.assign(sc->right_y + sc->right_offset[l], sc->right_y + sc->right_offset[l + 1]);
        c->sc.bl_left.push_back(std::move(a));
        c->sc.bl_right.push_back(std::move(b));
    }
    for (int p = 0; p < sc->obstacles.n_polygons; ++p) {
        Poly o;
        o.x.assign(sc->obstacles.x + sc->obstacles.offset[p], sc->obstacles.x + sc->obstacles.offset[p + 1]);
        o.y.assign(sc->obstacles.y + sc->obstacles.offset[p], sc->obstacles.y + sc->obstacles.offset[p + 1]);
        c->sc.static_obstacles.push_back(std::move(o));
    }
    c->fca.obst_off.assign(1, 0);
    for (const Poly& o : c->sc.static_obstacles) {
        c->fca.obst_x.insert(c->fca.obst_x.end(), o.x.begin(), o.x.end());
        c->fca.obst_y.insert(c->fca.obst_y.end(), o.y.begin(), o.y.end());
        c->fca.obst_off.push_back((int32_t)c->fca.obst_x.size());
    }
    // Simulation.setup: initial speed = steering = 0 (Simulation.m:52-65)
    c->tr.mx.resize(c->sc.n);
    c->tr.my.resize(c->sc.n);
    c->tr.myaw.resize(c->sc.n);
    c->tr.mspeed.assign(c->sc.n, 0.0);
    c->tr.msteer.assign(c->sc.n, 0.0);
    for (int v = 0; v < c->sc.n; ++v) {
        c->tr.mx[v] = c->sc.veh[v].x_start;
        c->tr.my[v] = c->sc.veh[v].y_start;
        c->tr.myaw[v] = c->sc.veh[v].yaw_start;
    }
    c->tr.info_old.assign(c->sc.n, Plan());
    c->tr.infos.assign(c->sc.n, Plan());
    *out = c;
    return PDMPC_OK;
}

int pdmpc_controller_set_parallel_coupling(pdmpc_controller* c, int32_t mode) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    if (mode != PDMPC_PARALLEL_PREVIOUS_TRAJECTORY && mode != PDMPC_PARALLEL_REACHABLE_SETS) return cfail(c, PDMPC_ERR_INVALID, "unknown parallel coupling mode");
    c->reach.parallel_mode = mode;
    return PDMPC_OK;
}

int pdmpc_controller_set_optimizer(pdmpc_controller* c, int32_t which) {
    if (!c) return cfail(c, PDMPC_ERR_INVALID, "null controller");
    if (which != PDMPC_OPTIMIZER_GRAPH_SEARCH && which != PDMPC_OPTIMIZER_SAMPLED) return cfail(c, PDMPC_ERR_INVALID, "optimizer must be PDMPC_OPTIMIZER_GRAPH_SEARCH or PDMPC_OPTIMIZER_SAMPLED");
    c->optimizer = which;
    return PDMPC_OK;
}

int pdmpc_controller_priorities(pdmpc_controller* c, int32_t* n_priorities, const int32_t** priorities, int32_t* n_collisions, const int32_t** collisions) {
    if (!c || !n_priorities || !priorities || !n_collisions || !collisions) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    const bool has = c->sc.cfg.priority_strategy != PDMPC_PRIORITY_COLORING, fca = c->sc.cfg.priority_strategy == PDMPC_PRIORITY_FCA;
    *n_priorities = has ? (int32_t)c->fca.prio.size() : 0;
    *priorities = c->fca.prio.data();
    *n_collisions = fca ? (int32_t)c->fca.count.size() : 0;
    *collisions = c->fca.count.data();
    return PDMPC_OK;
}

int pdmpc_controller_seeds(pdmpc_controller* c, int32_t* n, const uint32_t** seeds) {
    if (!c || !n || !seeds) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    const std::vector<uint32_t>& last = (c->x.built_last ? c->x.prob : c->prob).seeds;
    *n = (int32_t)last.size();
    *seeds = last.data();
    return PDMPC_OK;
}

int pdmpc_controller_set_lanelet_bounding(pdmpc_controller* c, int32_t on) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    c->reach.lanelet_bounding = on != 0;
    return PDMPC_OK;
}

int pdmpc_controller_set_reachability(pdmpc_controller* c, const pdmpc_mpa* mpa) {
    if (!c || !mpa) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    if (mpa->Hp != c->sc.Hp) return cfail(c, PDMPC_ERR_INVALID, "the automaton's Hp differs from the controller's");
    if (mpa->n_trims != (int32_t)c->sc.trim_speed.size()) return cfail(c, PDMPC_ERR_INVALID, "the automaton's trims differ from the scenario's");
    c->reach.has = false;
    std::vector<int32_t> off((size_t)mpa->n_trims * mpa->Hp + 1, 0);
    int rc = pdmpc_local_reachable_sets(mpa, 0, off.data(), nullptr, nullptr);
    if (rc != PDMPC_OK && rc != PDMPC_ERR_CAPACITY) return cfail(c, rc, "pdmpc_local_reachable_sets failed");
    std::vector<double> x((size_t)off.back() + 1), y((size_t)off.back() + 1);
    rc = pdmpc_local_reachable_sets(mpa, off.back(), off.data(), x.data(), y.data());
    if (rc) return cfail(c, rc, "pdmpc_local_reachable_sets failed");
    if (c->h) {
        const pdmpc_polygon_set ps = view_polygons(off, x, y);
        rc = pdmpc_upload_reachable_sets(c->h, mpa->n_trims, mpa->Hp, &ps);
        if (rc) return cfail(c, rc, std::string("pdmpc_upload_reachable_sets: ") + pdmpc_last_error());
    }
    c->sc.reach_off = std::move(off);
    c->sc.reach_x = std::move(x);
    c->sc.reach_y = std::move(y);
    c->reach.has = true;
    return PDMPC_OK;
}

// ---- human-driven vehicles
int pdmpc_controller_set_hdvs(pdmpc_controller* c, int32_t n_hdv, const pdmpc_mpa* hdv_mpa, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                              const double* tile_dx, const double* tile_dy) {
    if (!c || n_hdv < 1 || !hdv_mpa || !succ_offset || !relationship) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdvs: bad argument");
    const int n_lan = (int)c->sc.bl_left.size();
    bool lanelets = n_lan > 0;
    for (const VehicleDef& V : c->sc.veh) lanelets = lanelets && !V.lanelets_index.empty();
    if (!lanelets) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdvs: HDVs need a scenario with lanelets");
    if (c->h) {  // the HDV soup is the InterX checker's (edge_checks.hpp); the separating-axis checker has no test against it
        pdmpc_config hc{};
        int32_t has_mpa = 0;
        if (pdmpc_get_config(c->h, &hc, &has_mpa) != PDMPC_OK) return cfail(c, PDMPC_ERR_INVALID, "bad backend handle");
        if (hc.checker == PDMPC_CHECK_SAT) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdvs: the separating-axis checker does not check HDV sets");
    }
    if (hdv_mpa->Hp != c->sc.Hp) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdvs: the HDV automaton's Hp differs from the controller's");
    HdvTraffic H;
    H.lan_off.assign((size_t)n_lan + 1, 0);
    for (int i = 0; i < n_lan; ++i) {
        const Poly &L = c->sc.bl_left[(size_t)i], &R = c->sc.bl_right[(size_t)i];
        H.left_x.insert(H.left_x.end(), L.x.begin(), L.x.end());
        H.left_y.insert(H.left_y.end(), L.y.begin(), L.y.end());
        H.right_x.insert(H.right_x.end(), R.x.begin(), R.x.end());
        H.right_y.insert(H.right_y.end(), R.y.begin(), R.y.end());
        if (L.x.size() != R.x.size()) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdvs: a lanelet needs as many left as right points");
        H.lan_off[(size_t)i + 1] = (int32_t)H.left_x.size();
    }
    if (succ_offset[0] != 0 || succ_offset[n_lan] < 0 || (succ_offset[n_lan] > 0 && !succ_index)) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdvs: bad successor lists");
    H.succ_off.assign(succ_offset, succ_offset + n_lan + 1);
    H.succ_idx.assign(succ_index, succ_index + succ_offset[n_lan]);
    H.succ_idx.push_back(0);
    H.rel.assign(relationship, relationship + (size_t)n_lan * n_lan);
    H.n_trims = hdv_mpa->n_trims;
    H.local_off.assign((size_t)hdv_mpa->n_trims * hdv_mpa->Hp + 1, 0);
    int rc = pdmpc_local_reachable_sets(hdv_mpa, 0, H.local_off.data(), nullptr, nullptr);
    if (rc != PDMPC_OK && rc != PDMPC_ERR_CAPACITY) return cfail(c, rc, "pdmpc_local_reachable_sets failed");
    H.local_x.resize((size_t)H.local_off.back() + 1);
    H.local_y.resize((size_t)H.local_off.back() + 1);
    rc = pdmpc_local_reachable_sets(hdv_mpa, H.local_off.back(), H.local_off.data(), H.local_x.data(), H.local_y.data());
    if (rc) return cfail(c, rc, "pdmpc_local_reachable_sets failed");
    H.n = n_hdv;
    H.tile_dx.assign((size_t)n_hdv, 0.0);
    H.tile_dy.assign((size_t)n_hdv, 0.0);
    if (tile_dx) H.tile_dx.assign(tile_dx, tile_dx + n_hdv);
    if (tile_dy) H.tile_dy.assign(tile_dy, tile_dy + n_hdv);
    H.trim.assign((size_t)n_hdv, 1);  // ManualVehicle.m:33: local_reachable_sets(1, :)
    for (const VehicleDef& V : c->sc.veh) {
        H.cav_tile_dx.push_back(V.tile_dx);
        H.cav_tile_dy.push_back(V.tile_dy);
    }
    if (c->h) {  // (the map's own refusals -- limits, successor ids -- come from the one place that checks them; the upload is the first step's)
        const pdmpc_polygon_set local = view_polygons(H.local_off, H.local_x, H.local_y);
        rc = pdmpc_hdv_check_map_host(n_lan, H.lan_off.data(), H.lan_off.data(), H.left_x.data(), H.left_y.data(), H.right_x.data(), H.right_y.data(), H.succ_off.data(),
                                      H.succ_idx.data(), H.rel.data(), H.n_trims, c->sc.Hp, &local);
        if (rc) return cfail(c, rc, std::string("pdmpc_controller_set_hdvs: ") + pdmpc_last_error());
    }
    c->hdv = std::move(H);  // (with no map slot noted: the next step looks for the map on the handle)
    return PDMPC_OK;
}

int pdmpc_controller_set_hdv_drivers(pdmpc_controller* c, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const double* start_distance,
                                     const double* v_des, const double* params) {
    const std::string who = "pdmpc_controller_set_hdv_drivers: ";
    if (!c || !route_offset || !route_lanelet || !closed || !start_distance || !v_des || !params) return cfail(c, PDMPC_ERR_INVALID, who + "null argument");
    HdvTraffic& H = c->hdv;
    if (H.n == 0) return cfail(c, PDMPC_ERR_INVALID, who + "before pdmpc_controller_set_hdvs");
    if (H.rec_T > 0) return cfail(c, PDMPC_ERR_INVALID, who + "the HDVs replay a recording (pdmpc_controller_set_hdv_recording)");
    if (route_offset[0] != 0) return cfail(c, PDMPC_ERR_INVALID, who + "route offsets that do not start at 0");
    for (int q = 0; q < H.n; ++q)
        if (route_offset[q + 1] < route_offset[q]) return cfail(c, PDMPC_ERR_INVALID, who + "route offsets decrease");
    std::string why;
    if (const int rc = hdv_check_drive(params, c->sc.cfg.dt_seconds, H.n, v_des, &why)) return cfail(c, rc, who + why);
    // the routes against the controller's map, and the placement: the "measurement" of the first step
    std::vector<int32_t> seg((size_t)2 * H.n);
    std::vector<double> u((size_t)H.n), x((size_t)H.n), y((size_t)H.n), cs((size_t)H.n), sn((size_t)H.n);
    const int rc = pdmpc_hdv_place_host((int32_t)H.lan_off.size() - 1, H.lan_off.data(), H.lan_off.data(), H.left_x.data(), H.left_y.data(), H.right_x.data(), H.right_y.data(),
                                        H.succ_off.data(), H.succ_idx.data(), H.rel.data(), H.n, route_offset, route_lanelet, closed, start_distance, H.tile_dx.data(),
                                        H.tile_dy.data(), seg.data(), u.data(), x.data(), y.data(), cs.data(), sn.data());
    if (rc) return cfail(c, rc, who + pdmpc_last_error());
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

int pdmpc_controller_hdv_driver_state(pdmpc_controller* c, int32_t* state_seg, double* state_u, double* x, double* y, double* yaw, double* speed, double* gap) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    const HdvTraffic& H = c->hdv;
    if (!H.driven) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_hdv_driver_state before pdmpc_controller_set_hdv_drivers");
    if (state_seg) std::copy(H.seg.begin(), H.seg.end(), state_seg);
    if (state_u) std::copy(H.u.begin(), H.u.end(), state_u);
    if (x) std::copy(H.x.begin(), H.x.end(), x);
    if (y) std::copy(H.y.begin(), H.y.end(), y);
    if (yaw) std::copy(H.yaw.begin(), H.yaw.end(), yaw);
    if (speed) std::copy(H.speed.begin(), H.speed.end(), speed);
    if (gap) std::copy(H.gap.begin(), H.gap.end(), gap);
    return PDMPC_OK;
}

int pdmpc_controller_set_hdv_recording(pdmpc_controller* c, int32_t T, const double* x, const double* y, const double* yaw) {
    const std::string who = "pdmpc_controller_set_hdv_recording: ";
    if (!c || T < 1 || !x || !y || !yaw) return cfail(c, PDMPC_ERR_INVALID, who + "bad argument");
    HdvTraffic& H = c->hdv;
    if (H.n == 0) return cfail(c, PDMPC_ERR_INVALID, who + "before pdmpc_controller_set_hdvs");
    if (H.driven) return cfail(c, PDMPC_ERR_INVALID, who + "the HDVs have drivers (pdmpc_controller_set_hdv_drivers)");
    H.rec_T = T;
    H.rec_builds = 0;
    H.rec_x.assign(x, x + (size_t)T * H.n);
    H.rec_y.assign(y, y + (size_t)T * H.n);
    H.rec_yaw.assign(yaw, yaw + (size_t)T * H.n);
    return PDMPC_OK;
}

int pdmpc_controller_set_hdv_poses(pdmpc_controller* c, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw) {
    if (!c || !x || !y || !cos_yaw || !sin_yaw) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_poses: null argument");
    HdvTraffic& H = c->hdv;
    if (H.n == 0) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_poses before pdmpc_controller_set_hdvs");
    if (H.driven || H.rec_T > 0)
        return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_poses: the HDVs move themselves (pdmpc_controller_set_hdv_drivers / _set_hdv_recording); their poses are not set");
    H.x.assign(x, x + H.n);
    H.y.assign(y, y + H.n);
    H.cos_yaw.assign(cos_yaw, cos_yaw + H.n);
    H.sin_yaw.assign(sin_yaw, sin_yaw + H.n);
    hdv_driven_yaw(H);
    H.measured = true;
    return PDMPC_OK;
}

int pdmpc_controller_set_hdv_measurements(pdmpc_controller* c, const double* x, const double* y, const double* yaw) {
    if (!c || !x || !y || !yaw) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_measurements: null argument");
    HdvTraffic& H = c->hdv;
    if (H.n == 0) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_measurements before pdmpc_controller_set_hdvs");
    if (H.driven || H.rec_T > 0)
        return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_measurements: the HDVs move themselves (pdmpc_controller_set_hdv_drivers / _set_hdv_recording); their poses are not measured");
    H.x.assign(x, x + H.n);
    H.y.assign(y, y + H.n);
    H.yaw.assign(yaw, yaw + H.n);
    H.cos_yaw.resize((size_t)H.n);
    H.sin_yaw.resize((size_t)H.n);
    for (int q = 0; q < H.n; ++q) {
        H.cos_yaw[(size_t)q] = std::cos(yaw[q]);
        H.sin_yaw[(size_t)q] = std::sin(yaw[q]);
    }
    H.measured = true;
    return PDMPC_OK;
}

int pdmpc_controller_hdv_info(pdmpc_controller* c, int32_t* n_hdv, const int32_t** closest_offset, const int32_t** closest_index, int32_t* n_rows, const int32_t** row_hdv,
                              const int32_t** set_offset, const double** set_x, const double** set_y, const uint8_t** set_flags, const uint8_t** adjacency) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    const HdvTraffic& H = c->hdv;
    if (H.n == 0 || H.closest_off.empty()) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_hdv_info before a step was built with HDVs");
    if (n_hdv) *n_hdv = H.n;
    if (closest_offset) *closest_offset = H.closest_off.data();
    if (closest_index) *closest_index = H.closest_idx.data();
    if (n_rows) *n_rows = H.n_rows;
    if (row_hdv) *row_hdv = H.row_hdv.data();
    if (set_offset) *set_offset = H.set_off.data();
    if (set_x) *set_x = H.set_x.data();
    if (set_y) *set_y = H.set_y.data();
    if (set_flags) *set_flags = H.set_flags.data();
    if (adjacency) *adjacency = H.adjacency.data();
    return PDMPC_OK;
}

int pdmpc_controller_destroy(pdmpc_controller* c) {
    delete c;
    return PDMPC_OK;
}

// records of the step in slot order -> plans, exhaustion handling, fallbacks of coupled vehicles, plant update
int pdmpc_controller_apply(pdmpc_controller* c, const pdmpc_vehicle_out* recs) {
    if (!c || !recs) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    const int n = c->sc.n, Hp = c->sc.Hp;
    auto fallback_plan = [&](int i, Plan& p) -> bool {  // plan_fallback (:678-718): the previous plan shifted by one step
        const Plan& old = c->tr.info_old[i];
        if (!old.present) return false;
        p.present = true;
        const size_t m = old.shapes.size();
        p.resize(m);
        for (size_t q = 0; q < m; ++q) {
            const size_t from = std::min(q + 1, m - 1);
            p.shapes[q] = old.shapes[from];
            p.trims[q] = old.trims[from];
            p.yx[q] = old.yx[from];
            p.yy[q] = old.yy[from];
            p.yyaw[q] = old.yyaw[from];
        }
        return true;
    };
    // The step's plans are built in c->tr.infos — nothing else reads it — and swapped with c->tr.info_old at the end: an error status or a
    // fallback in the first step leaves the controller's plans as they were, and the vectors of a plan keep their capacity from
    // step to step (they are overwritten entry by entry, not re-created).
    std::vector<Plan>& infos = c->tr.infos;
    infos.resize((size_t)n);
    if (c->tr.last_pops.size() != (size_t)n) c->tr.last_pops.assign((size_t)n, 0.0);
    for (int s = 0; s < n; ++s) {
        const int i = c->pri.order[s];
        const pdmpc_vehicle_out& r = recs[s];
        if (r.status != PDMPC_OK && r.status != PDMPC_EXHAUSTED) return cfail(c, PDMPC_ERR_HIP, "a result record carries an error status: not a planning result");
        Plan& p = infos[i];
        p.present = p.needs_fallback = p.exhausted = false;
        p.n_expanded = r.n_expanded;
        c->tr.last_pops[(size_t)i] = (double)r.n_popped;
        if (r.status == PDMPC_OK) {
            p.present = true;
            p.resize((size_t)Hp);
            for (int q = 0; q < Hp; ++q) {
                Poly& sh = p.shapes[q];
                sh.x.assign(r.shapes[q][0], r.shapes[q][0] + r.shape_cols[q]);
                sh.y.assign(r.shapes[q][1], r.shapes[q][1] + r.shape_cols[q]);
                p.trims[q] = r.predicted_trims[q];
                p.yx[q] = r.y_predicted[q][0];
                p.yy[q] = r.y_predicted[q][1];
                p.yyaw[q] = r.y_predicted[q][2];
            }
        } else {  // PrioritizedController.m:344-352
            p.exhausted = true;
            const bool standstill = c->sc.trim_speed[c->in.trims[i] - 1] == 0;
            if (standstill && c->sc.cfg.constraint_from_successor != PDMPC_SUCCESSOR_NONE) {  // handle_graph_search_exhaustion (:568-616)
                p.present = true;
                p.shapes.assign((size_t)Hp, c->in.occ_plain[i]);
                p.trims.assign((size_t)Hp, c->in.trims[i]);
                p.yx.assign((size_t)Hp, c->tr.mx[i]);
                p.yy.assign((size_t)Hp, c->tr.my[i]);
                p.yyaw.assign((size_t)Hp, c->tr.myaw[i]);
            } else {
                if (!fallback_plan(i, p)) return cfail(c, PDMPC_ERR_INVALID, "a vehicle needs a fallback in its first step");
                p.needs_fallback = true;
            }
        }
    }
    // handle_others_fallback / check_others_fallback
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || infos[i].needs_fallback;
    if (any) {
        std::vector<int> fm((size_t)n * n, 0);
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                int v = at(c->in.adjacency, n, a, b);
                if (infos[a].needs_fallback && at(c->pri.directed_seq, n, a, b)) v -= 1;
                if (infos[b].needs_fallback && at(c->pri.directed_seq, n, b, a)) v -= 1;
                fm[(size_t)a * n + b] = v;
            }
        std::vector<uint8_t> reached(n, 0);
        for (int f = 0; f < n; ++f) {
            if (!infos[f].needs_fallback) continue;
            std::vector<uint8_t> seen(n, 0);
            std::vector<int> stack{f};
            seen[f] = 1;
            while (!stack.empty()) {
                const int a = stack.back();
                stack.pop_back();
                for (int b = 0; b < n; ++b)
                    if (fm[(size_t)a * n + b] != 0 && !seen[b]) {
                        seen[b] = 1;
                        stack.push_back(b);
                    }
            }
            for (int v = 0; v < n; ++v) reached[v] |= seen[v];
        }
        for (int i = 0; i < n; ++i)
            if (reached[i] && !infos[i].needs_fallback) {
                Plan& p = infos[i];  // (keeps its search's n_expanded and exhausted)
                if (!fallback_plan(i, p)) return cfail(c, PDMPC_ERR_INVALID, "a vehicle needs a fallback in its first step");
                p.needs_fallback = false;  // plan_fallback(is_fallback_while_planning = false)
            }
    }
    std::swap(c->tr.info_old, c->tr.infos);
    // Simulation.apply (Simulation.m:86-100)
    for (int i = 0; i < n; ++i) {
        const Plan& p = c->tr.info_old[i];
        c->tr.mx[i] = p.yx[0];
        c->tr.my[i] = p.yy[0];
        c->tr.myaw[i] = p.yyaw[0];
        c->tr.mspeed[i] = c->sc.trim_speed[p.trims[0] - 1];
        c->tr.msteer[i] = c->sc.trim_steering[p.trims[0] - 1];
    }
    return PDMPC_OK;
}

// One pass of HighLevelController.main_control_loop (:334-373) in simulation: build, plan on the GPU (one launch), apply.
int pdmpc_controller_last_timing(pdmpc_controller* c, double* ms6) {
    if (!c || !ms6) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    for (int i = 0; i < 6; ++i) ms6[i] = c->timing[i];
    return PDMPC_OK;
}

int pdmpc_controller_timing_sum(pdmpc_controller* c, double* ms6, int64_t* n_steps, int32_t reset) {
    if (!c) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    if (ms6)
        for (int i = 0; i < 6; ++i) ms6[i] = c->timing_sum[i];
    if (n_steps) *n_steps = c->timing_steps;
    if (reset) {
        for (int i = 0; i < 6; ++i) c->timing_sum[i] = 0;
        c->timing_steps = 0;
    }
    return PDMPC_OK;
}

int pdmpc_controller_step(pdmpc_controller* c) {
    if (!c || !c->h) return cfail(c, PDMPC_ERR_INVALID, "controller has no backend handle");
    auto t = std::chrono::steady_clock::now();
    int rc = pdmpc_controller_build_step(c);
    if (rc) return rc;
    c->timing[0] = ms_since(t);
    c->timing[4] = 0;
    c->out.resize(c->sc.n);
    rc = plan_built(target_of(c), c->prob, c->tr.last_pops.size() == (size_t)c->sc.n, [&](int s) { return c->tr.last_pops[(size_t)c->pri.order[(size_t)s]]; }, c->optimizer, c->timing,
                    pdmpc_plan_step, c->out.data());
    if (rc) return own(c, rc);
    return apply_and_account(c);
}

int pdmpc_controller_run(pdmpc_controller* c, int32_t n_steps, double* ms) {
    return timed_steps(n_steps, ms, [&] { return pdmpc_controller_step(c); });
}

int pdmpc_controller_problem(pdmpc_controller* c, int32_t* n, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                             const pdmpc_polygon_set** fallback, const int32_t** order, const int32_t** levels) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    expose(c->prob, n, in, pred_offset, pred_index, fallback);
    if (n) *n = c->sc.n;  // (also before the first build)
    if (order) *order = c->pri.order.data();
    if (levels) *levels = c->pri.levels.data();
    return PDMPC_OK;
}

int pdmpc_controller_state(pdmpc_controller* c, double* x, double* y, double* yaw, double* speed, double* steering, int32_t* needs_fallback, int32_t* time_step) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    for (int i = 0; i < c->sc.n; ++i) {
        if (x) x[i] = c->tr.mx[i];
        if (y) y[i] = c->tr.my[i];
        if (yaw) yaw[i] = c->tr.myaw[i];
        if (speed) speed[i] = c->tr.mspeed[i];
        if (steering) steering[i] = c->tr.msteer[i];
        if (needs_fallback) needs_fallback[i] = c->tr.info_old[i].present && c->tr.info_old[i].needs_fallback;
    }
    if (time_step) *time_step = c->tr.k;
    return PDMPC_OK;
}

int pdmpc_exploration_permutations(int32_t n_levels, int32_t n_perm, uint32_t seed, int32_t* out) {
    if (n_levels < 1 || n_perm < 1 || !out) return cfail(nullptr, PDMPC_ERR_INVALID, "bad argument");
    exploration_permutations(n_levels, n_perm, seed, out);
    return PDMPC_OK;
}

// Everything one launch needs to plan the whole time step (controller.py: build_step_problem): vehicles in level order
// (slot = position), per-slot predecessor slots, per-slot areas to publish on exhaustion.  A step alone is a sweep of one member.
int pdmpc_controller_build_step(pdmpc_controller* c) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    return own(c, build_members(c->h, &c, 1, BatchKind{}, c->prep));
}

// ---- the explorative step (twin of pdmpc.explorative.build_exploration_batch / choose_solution / explore_step)
// PrioritizedExplorativeController.m:25-91: the step's traffic state under n_perm prioritizations, one flattened batch: instance p
// permutes the computation levels of the base prioritization (prepare_permutation :42-58: a vehicle of level L gets the position
// of L in permutation p as its priority), slots ordered by (level, instance, slot).  Advances the time step like build_step.
int pdmpc_controller_explore_build(pdmpc_controller* c, int32_t n_perm, uint32_t seed) {
    if (!c || n_perm < 1) return cfail(c, PDMPC_ERR_INVALID, "bad argument");
    SwitchedOn exploring(c->as.exploring);
    int rc = pdmpc_controller_build_step(c);  // instance 0: the controller's own prioritization
    if (rc) return rc;
    return permute_instances(c, n_perm, seed);
}
int pdmpc_controller_explore_problem(pdmpc_controller* c, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                                     const pdmpc_polygon_set** fallback, const int32_t** instance, const int32_t** vehicle, const int32_t** level) {
    if (!c || c->x.prob.in.empty()) return cfail(c, PDMPC_ERR_INVALID, "no exploration batch has been built");
    expose(c->x.prob, n_slots, in, pred_offset, pred_index, fallback);
    if (instance) *instance = c->x.instance.data();
    if (vehicle) *vehicle = c->x.vehicle.data();
    if (level) *level = c->x.level.data();
    return PDMPC_OK;
}

// compute_solution_cost / choose_solution (:94-176): per weakly connected sub-graph of the coupling graph the instance with the
// smallest sum of the cost-to-come of the vehicles' final nodes after round(., 8); a vehicle whose search was exhausted makes its
// instance infinitely expensive.  chosen[v] = instance of vehicle v's sub-graph; cost (may be NULL): n_perm x n_graphs, graphs
// ordered by their smallest vehicle.  The chosen instances' couplings become the controller's (what apply's fallback handling sees).
int pdmpc_controller_explore_choose(pdmpc_controller* c, const pdmpc_vehicle_out* recs, int32_t* chosen, int32_t* n_graphs, double* cost) {
    if (!c || !recs || c->x.inst.empty()) return cfail(c, PDMPC_ERR_INVALID, "no exploration batch has been built");
    if (const int rc = choose_from_records(c, kExploreChoice, recs, (int)c->x.inst.size() * c->sc.n, false)) return rc;
    if (chosen) std::copy(c->x.chosen.begin(), c->x.chosen.end(), chosen);
    if (n_graphs) *n_graphs = c->x.graphs;
    if (cost) std::copy(c->x.cost.begin(), c->x.cost.end(), cost);
    return PDMPC_OK;
}

// One explorative time step: build the batch, plan all prioritizations with ONE launch, choose per sub-graph, apply the chosen plans.
int pdmpc_controller_explore_step(pdmpc_controller* c, int32_t n_perm) {
    if (!c || !c->h) return cfail(c, PDMPC_ERR_INVALID, "controller has no backend handle");
    const auto t = std::chrono::steady_clock::now();
    const int rc = pdmpc_controller_explore_build(c, n_perm, (uint32_t)(c->tr.k + 1));  // RandStream("mt19937ar", Seed = obj.k) (:249)
    if (rc) return rc;
    return batch_step(c, t, c->follow_own, kExploreChoice);
}

int pdmpc_controller_set_device_choice(pdmpc_controller* c, int32_t on) {
    if (!c) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    c->device_choice = on != 0;
    return PDMPC_OK;
}

int pdmpc_controller_explore_follow_own(pdmpc_controller* c, int32_t on) {
    if (!c) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    c->follow_own = on != 0;
    return PDMPC_OK;
}

int pdmpc_controller_explore_run(pdmpc_controller* c, int32_t n_perm, int32_t n_steps, double* ms) {
    if (!c) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    SwitchedOn lean(c->lean_explore);
    return timed_steps(n_steps, ms, [&] { return pdmpc_controller_explore_step(c, n_perm); });
}

int pdmpc_controller_explore_result(pdmpc_controller* c, int32_t* chosen, int32_t* n_graphs, const double** cost, const pdmpc_vehicle_out** records) {
    if (!c || c->x.chosen.empty()) return cfail(c, PDMPC_ERR_INVALID, "no explorative step has been chosen");
    if (chosen) std::copy(c->x.chosen.begin(), c->x.chosen.end(), chosen);
    if (n_graphs) *n_graphs = c->x.graphs;
    if (cost) *cost = c->x.cost.data();
    if (records) *records = c->x.out.empty() ? nullptr : c->x.out.data();
    return PDMPC_OK;
}

int pdmpc_unique_priorities_host(int32_t n, const uint8_t* adjacency, int64_t max_out, int64_t* n_out, uint32_t* masks, int32_t* priorities) {
    if (n_out) *n_out = -1;
    if (n < 1 || !adjacency || !n_out || max_out < 0 || (max_out > 0 && (!masks || !priorities)))
        return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_unique_priorities_host: bad argument");
    const char* why = "";
    if (const int rc = enumerate_on_host(n, adjacency, max_out, n_out, masks, priorities, &why)) return cfail(nullptr, rc, std::string("pdmpc_unique_priorities_host: ") + why);
    return PDMPC_OK;
}

// ... of several graphs (the twin of pdmpc_unique_priorities_grouped): every graph counted first, and only if every count fits its
// max_out the lists written one after the other
int pdmpc_unique_priorities_grouped_host(int32_t n_groups, const int32_t* group_n, const uint8_t** adjacency, int64_t* max_out, int64_t* n_out, uint32_t* masks,
                                         int32_t* priorities) {
    if (n_groups < 1 || !group_n || !adjacency || !max_out || !n_out) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_unique_priorities_grouped_host: bad argument");
    for (int g = 0; g < n_groups; ++g) {
        n_out[g] = -1;
        if (group_n[g] < 1 || !adjacency[g] || max_out[g] < 0 || (max_out[g] > 0 && (!masks || !priorities)))
            return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_unique_priorities_grouped_host: bad argument for graph " + std::to_string(g));
    }
    int refused = -1;
    const char *why = "", *first_why = "";
    for (int g = 0; g < n_groups; ++g) {  // (max_out 0: nothing is written, the count is reported)
        (void)enumerate_on_host(group_n[g], adjacency[g], 0, &n_out[g], nullptr, nullptr, &why);
        if ((n_out[g] < 0 || n_out[g] > max_out[g]) && refused < 0) {
            refused = g;
            first_why = why;
        }
    }
    if (refused >= 0) return cfail(nullptr, PDMPC_ERR_CAPACITY, "pdmpc_unique_priorities_grouped_host: graph " + std::to_string(refused) + ": " + first_why);
    for (int g = 0; g < n_groups; ++g) {
        int64_t K = 0;
        if (const int rc = enumerate_on_host(group_n[g], adjacency[g], max_out[g], &K, masks, priorities, &why))
            return cfail(nullptr, rc, std::string("pdmpc_unique_priorities_grouped_host: ") + why);
        masks += K;
        priorities += K * group_n[g];
    }
    return PDMPC_OK;
}

// ---- the optimal-priority step (PrioritizedOptimalController.m; twin of pdmpc.optimal.build_optimal_batch / choose_solution / optimal_step)
// :25-53 + controller (:134-152): the step's traffic state under every unique prioritization of its coupling graph, one flattened batch:
// prepare_permutation = prioritize() with constant priorities = prioritization p, then group(); slots ordered by (level, instance, slot).
int pdmpc_controller_optimal_build(pdmpc_controller* c, int32_t max_instances) {
    if (!c || max_instances < 1) return cfail(c, PDMPC_ERR_INVALID, "bad argument");
    // traffic info and coupling of the step (and the controller's own problem, replaced by instance 0), the enumeration, the instances: a
    // sweep of one member
    return own(c, build_members(c->h, &c, 1, BatchKind{0, max_instances}, c->prep));
}

int pdmpc_controller_optimal_choose(pdmpc_controller* c, const pdmpc_vehicle_out* recs, int32_t* chosen, double* cost) {
    if (!c || !recs || c->x.inst.empty() || c->x.o_masks.size() != c->x.inst.size()) return cfail(c, PDMPC_ERR_INVALID, "no optimal-priority batch has been built");
    if (const int rc = choose_from_records(c, kOptimalChoice, recs, (int)c->x.inst.size() * c->sc.n, false)) return rc;
    if (chosen) std::copy(c->x.chosen.begin(), c->x.chosen.end(), chosen);
    if (cost) std::copy(c->x.cost.begin(), c->x.cost.end(), cost);
    return PDMPC_OK;
}

// One optimal-priority time step: every unique prioritization planned with ONE launch, the choice per vehicle, the chosen plans applied.
int pdmpc_controller_optimal_step(pdmpc_controller* c, int32_t max_instances) {
    if (!c || !c->h) return cfail(c, PDMPC_ERR_INVALID, "controller has no backend handle");
    const auto t = std::chrono::steady_clock::now();
    const int rc = pdmpc_controller_optimal_build(c, max_instances);
    if (rc) return rc;
    return batch_step(c, t, false, kOptimalChoice);
}

int pdmpc_controller_optimal_run(pdmpc_controller* c, int32_t max_instances, int32_t n_steps, double* ms) {
    if (!c) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    SwitchedOn lean(c->lean_explore);
    return timed_steps(n_steps, ms, [&] { return pdmpc_controller_optimal_step(c, max_instances); });
}

int pdmpc_controller_optimal_result(pdmpc_controller* c, int32_t* chosen, int32_t* n_instances, const double** cost, const pdmpc_vehicle_out** records) {
    if (!c || c->x.chosen.empty() || c->x.o_masks.size() != c->x.inst.size()) return cfail(c, PDMPC_ERR_INVALID, "no optimal-priority step has been chosen");
    if (chosen) std::copy(c->x.chosen.begin(), c->x.chosen.end(), chosen);
    if (n_instances) *n_instances = (int32_t)c->x.inst.size();
    if (cost) *cost = c->x.cost.data();
    if (records) *records = c->x.out.empty() ? nullptr : c->x.out.data();
    return PDMPC_OK;
}

// ---- centralized control (step_centralized.hpp)
int pdmpc_controller_centralized_build(pdmpc_controller* c) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    if (const int rc = centralized_refusal(c)) return rc;
    centralized_build(c);
    return PDMPC_OK;
}

int pdmpc_controller_centralized_problem(pdmpc_controller* c, int32_t* n, const pdmpc_vehicle_in** in) {
    if (!c || !c->cen.built) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_centralized_problem before pdmpc_controller_centralized_build");
    if (n) *n = c->sc.n;
    if (in) *in = c->cen.in.data();
    return PDMPC_OK;
}

int pdmpc_controller_centralized_apply(pdmpc_controller* c, const pdmpc_vehicle_out* recs) {
    if (!c || !recs) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    if (!c->cen.built) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_centralized_apply before pdmpc_controller_centralized_build");
    return centralized_apply(c, recs);
}

// One pass of the main control loop with CentralizedController.controller: build, ONE joint search of one problem, apply.
int pdmpc_controller_centralized_step(pdmpc_controller* c) {
    if (!c || !c->h) return cfail(c, PDMPC_ERR_INVALID, "controller has no backend handle");
    if (const int rc = centralized_refusal(c)) return rc;
    auto t = std::chrono::steady_clock::now();
    centralized_build(c);
    c->timing[0] = ms_since(t);
    c->timing[4] = 0;
    c->out.resize((size_t)c->sc.n);
    const int32_t problem_offset[2] = {0, c->sc.n};
    if (const int rc = pdmpc_plan_joint(c->h, 1, problem_offset, c->cen.in.data(), c->out.data())) return cfail(c, rc, std::string("pdmpc_plan_joint: ") + pdmpc_last_error());
    joint_call_timing(c->h, c->timing);
    t = std::chrono::steady_clock::now();
    const int rc = centralized_apply(c, c->out.data());
    c->timing[5] = ms_since(t);
    for (int i = 0; i < 6; ++i) c->timing_sum[i] += c->timing[i];
    c->timing_steps += 1;
    return rc;
}

int pdmpc_controller_centralized_run(pdmpc_controller* c, int32_t n_steps, double* ms) {
    return timed_steps(n_steps, ms, [&] { return pdmpc_controller_centralized_step(c); });
}

const pdmpc_vehicle_out* pdmpc_controller_records(pdmpc_controller* c) { return c && !c->out.empty() ? c->out.data() : nullptr; }

}  // extern "C"

// ---- several closed loops in lock-step: the members' own build / apply code around ONE step preparation on the
// device and ONE pdmpc_plan_step for all of them.  Sweep slots are the members' problems one after the other, each in its own slot order.
struct pdmpc_sweep {
    pdmpc_handle* h = nullptr;
    pdmpc_group* group = nullptr;  // pdmpc_sweep_set_group: the concatenated problems are planned over this group (h is its rank 0)
    int32_t group_mode = PDMPC_SHARD_AUTO;
    std::vector<pdmpc_controller*> members;
    std::vector<int32_t> first;  // [M + 1] member m's first sweep slot (= its first vehicle among the concatenated vehicles)
    bool broken = false;         // a step failed half way: the members have advanced unevenly
    bool built = false;
    double timing[6] = {0, 0, 0, 0, 0, 0};
    PrepScratch prep;  // of the members' ONE step preparation (its prep_calls: pdmpc_sweep_last_prep_calls)
    StepProblem prob;                          // the concatenated problem, and per slot of it:
    std::vector<int32_t> member, member_slot;  // whose it is, and which of that member's slots
    std::vector<pdmpc_vehicle_out> out;
    int32_t optimal_calls[2] = {0, 0};  // pdmpc_sweep_optimal_last_calls
    // centralized members (pdmpc_sweep_centralized_*): the live members' joint problems one after the other as ONE pdmpc_plan_joint takes them
    struct Centralized {
        bool built = false;
        std::vector<int32_t> problem_offset, member;  // [n_problems + 1], [n_problems]: whose problem it is
        std::vector<pdmpc_vehicle_in> in;
        std::vector<pdmpc_vehicle_out> out;
        std::vector<int32_t> exhausted_at;  // [M] 0: live; else the time step at which the member's search ran empty
    } cen;
    // the concatenated batch of prioritizations (pdmpc_sweep_explore_*, pdmpc_sweep_optimal_*): the members' flattened batches one after
    // the other, and their choices
    struct Batch {
        int n_perm = 0;              // of the explorative batch that is built (0: none)
        bool optimal = false;        // an optimal-priority batch is built (the members' K differ: first[])
        std::vector<int32_t> first;  // [M + 1] member m's first slot of the batch
        StepProblem prob;
        std::vector<int32_t> member, instance, vehicle, level;  // per slot: whose it is, and the member's own tags of it
        std::vector<ChoiceLists> lists;                           // per member, slots of its own batch
        ChoiceLists all;                                          // ... concatenated, slots of the whole batch
        std::vector<int32_t> first_graph, first_cell, chosen;     // [M + 1] each member's part of `all`; what the graphs chose
        std::vector<double> cell_cost;
        std::vector<pdmpc_vehicle_out> picks;                     // member after member, each in its own slot order
    } x;
};

namespace {
int N_of(const pdmpc_sweep* s) { return s->first.back(); }
PlanTarget target_of(const pdmpc_sweep* s) { return {s->h, s->group, s->group_mode}; }
// what pdmpc_controller_set_group and pdmpc_sweep_set_group refuse: an unknown sharding mode, a group whose rank 0 is another handle
int group_refusal(pdmpc_group* g, int32_t mode, pdmpc_handle* h, const char* who) {
    if (mode != PDMPC_SHARD_AUTO && mode != PDMPC_SHARD_COMPONENTS && mode != PDMPC_SHARD_LEVELS) return cfail(nullptr, PDMPC_ERR_INVALID, std::string(who) + ": unknown sharding mode");
    pdmpc_handle* h0 = nullptr;
    if (pdmpc_group_handle(g, 0, &h0) != PDMPC_OK || !h0 || h0 != h)
        return cfail(nullptr, PDMPC_ERR_INVALID, std::string(who) + ": not created on the handle of the group's rank 0 (pdmpc_group_handle(group, 0))");
    return PDMPC_OK;
}
// more plans than the handle's max_vehicles (without a handle: any number) are refused with `text`
int refuse_beyond_handle(pdmpc_handle* h, int64_t plans, const char* text) {
    pdmpc_config hc{};
    int32_t has_mpa = 0;
    if (h && pdmpc_get_config(h, &hc, &has_mpa) != PDMPC_OK) return cfail(nullptr, PDMPC_ERR_INVALID, "bad backend handle");
    return h && plans > hc.max_vehicles ? cfail(nullptr, PDMPC_ERR_CAPACITY, text) : PDMPC_OK;
}

// A member's problem P as the slots of S from `first` on (first = 0: S starts over; whatever S held from that slot on goes): shallow
// copies, the seeds along with them, predecessor slots shifted by `first`, and behind the last one the entry that keeps pred_index
// from ever being an empty array
void append_problem(StepProblem& S, const StepProblem& P, int32_t first) {
    assert(first == 0 || first == S.n());  // members are appended in order, each at the end of what is there
    const size_t f = (size_t)first, n = (size_t)P.n();
    S.pred_offset.resize(f + 1, 0);
    S.pred_index.resize((size_t)S.pred_offset[f]);
    S.in.resize(f);
    S.fb.resize(f);
    S.seeds.resize(f);
    S.in.insert(S.in.end(), P.in.begin(), P.in.end());
    S.fb.insert(S.fb.end(), P.fb.begin(), P.fb.end());
    S.seeds.insert(S.seeds.end(), P.seeds.begin(), P.seeds.end());
    const int32_t e0 = S.pred_offset[f];
    for (size_t q = 0; q < n; ++q) S.pred_offset.push_back(e0 + P.pred_offset[q + 1]);
    for (int32_t e = 0; e < P.pred_offset[n]; ++e) S.pred_index.push_back(first + P.pred_index[(size_t)e]);
    S.pred_index.push_back(0);
}

int sweep_build(pdmpc_sweep* s) {
    const size_t M = s->members.size();
    if (const int rc = build_members(s->h, s->members.data(), M, BatchKind{}, s->prep)) return rc;
    s->member.clear();
    s->member_slot.clear();
    for (size_t m = 0; m < M; ++m) {
        const pdmpc_controller* c = s->members[m];
        append_problem(s->prob, c->prob, s->first[m]);
        s->member.insert(s->member.end(), (size_t)c->sc.n, (int32_t)m);
        for (int q = 0; q < c->sc.n; ++q) s->member_slot.push_back(q);
    }
    s->built = true;
    return PDMPC_OK;
}

int sweep_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records, bool keep_records) {
    for (size_t m = 0; m < s->members.size(); ++m) {
        pdmpc_controller* c = s->members[m];
        const pdmpc_vehicle_out* r = records + s->first[m];
        if (keep_records) {  // (pdmpc_controller_records: the member's own records, in its own slot order)
            c->out.assign(r, r + c->sc.n);
            r = c->out.data();
        }
        if (const int rc = pdmpc_controller_apply(c, r)) return rc;
    }
    return PDMPC_OK;
}

// a failed step leaves the members unevenly advanced: nothing more is stepped
int sweep_guard(pdmpc_sweep* s, int rc) {
    if (rc) s->broken = true;
    return rc;
}
// ... and what every entry point that steps a sweep refuses first, in this order: an argument that is missing (its text), an earlier
// failure, and (before: its text) a step whose build has not run
int sweep_refusal(const pdmpc_sweep* s, bool missing, const char* missing_text, bool unbuilt = false, const char* before = nullptr) {
    if (missing) return cfail(nullptr, PDMPC_ERR_INVALID, missing_text);
    if (s->broken) return cfail(nullptr, PDMPC_ERR_INVALID, "an earlier step of the sweep failed: its members have advanced unevenly");
    if (unbuilt) return cfail(nullptr, PDMPC_ERR_INVALID, before);
    return PDMPC_OK;
}
// ... of a step over a batch of prioritizations
int batch_refusal(const pdmpc_sweep* s, bool needs_handle) {
    if (!s) return cfail(nullptr, PDMPC_ERR_INVALID, "null sweep");
    return sweep_refusal(s, needs_handle && !s->h, "the sweep has no backend handle");
}

// ---- the explorative step of a sweep

// what pdmpc_sweep_explore_* refuse before any member advances
int explore_refusal(pdmpc_sweep* s, int32_t n_perm, bool needs_handle) {
    if (const int rc = batch_refusal(s, needs_handle)) return rc;
    if (n_perm < 1) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_explore: n_perm < 1");
    return refuse_beyond_handle(s->h, (int64_t)N_of(s) * n_perm, "pdmpc_sweep_explore: the members' prioritizations are more plans than the handle's max_vehicles");
}

// what pdmpc_sweep_optimal_* refuse before any member advances
int optimal_refusal(pdmpc_sweep* s, int32_t max_instances, bool needs_handle) {
    if (const int rc = batch_refusal(s, needs_handle)) return rc;
    if (max_instances < 1) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_optimal: max_instances < 1");
    for (const pdmpc_controller* c : s->members)
        if (c->sc.n > 64) return cfail(nullptr, PDMPC_ERR_CAPACITY, "pdmpc_sweep_optimal: a member has more than 64 vehicles");
    return PDMPC_OK;
}

// every member's batch of prioritizations (explorative or optimal-priority), and the batches one after the other
int sweep_batch_build(pdmpc_sweep* s, BatchKind kind) {
    pdmpc_sweep::Batch& X = s->x;
    X.n_perm = 0;
    X.optimal = false;
    const size_t M = s->members.size();
    if (const int rc = build_members(s->h, s->members.data(), M, kind, s->prep)) return rc;
    X.first.assign(1, 0);
    X.member.clear();
    X.instance.clear();
    X.vehicle.clear();
    X.level.clear();
    for (size_t m = 0; m < M; ++m) {
        const pdmpc_controller* c = s->members[m];
        append_problem(X.prob, c->x.prob, X.first[m]);
        X.first.push_back(X.prob.n());
        X.member.insert(X.member.end(), (size_t)c->x.prob.n(), (int32_t)m);
        X.instance.insert(X.instance.end(), c->x.instance.begin(), c->x.instance.end());
        X.vehicle.insert(X.vehicle.end(), c->x.vehicle.begin(), c->x.vehicle.end());
        X.level.insert(X.level.end(), c->x.level.begin(), c->x.level.end());
    }
    X.n_perm = kind.n_perm;
    X.optimal = kind.max_instances > 0;
    return PDMPC_OK;
}

// the optimal-priority batches: what is known only once the couplings exist is refused here (the enumeration refuses a member with more
// than 32 coupling edges or more than max_instances prioritizations)
int sweep_optimal_build(pdmpc_sweep* s, int max_instances) {
    s->optimal_calls[0] = s->optimal_calls[1] = 0;
    const int rc = sweep_batch_build(s, BatchKind{0, max_instances});
    s->optimal_calls[0] = s->prep.prio.calls;
    if (rc) return rc;
    return refuse_beyond_handle(s->h, s->x.prob.n(), "pdmpc_sweep_optimal: the members' unique prioritizations are more plans than the handle's max_vehicles");
}

// the concatenated batch as pdmpc_sweep_explore_problem / pdmpc_sweep_optimal_problem hand it out
int expose_batch(const pdmpc_sweep::Batch& X, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                 const pdmpc_polygon_set** fallback, const int32_t** member, const int32_t** instance, const int32_t** vehicle, const int32_t** level) {
    expose(X.prob, n_slots, in, pred_offset, pred_index, fallback);
    if (member) *member = X.member.data();
    if (instance) *instance = X.instance.data();
    if (vehicle) *vehicle = X.vehicle.data();
    if (level) *level = X.level.data();
    return PDMPC_OK;
}

// does every vehicle of member c follow the controller's own prioritization whatever is chosen? (the explorative step's measurement
// switch; never the optimal-priority step)
inline bool follows_own(const pdmpc_controller* c, const BatchChoice& how) { return &how == &kExploreChoice && c->follow_own; }

// the records of the whole batch: every member chooses on the host and applies its chosen plans
int sweep_batch_apply(pdmpc_sweep* s, const BatchChoice& how, const pdmpc_vehicle_out* records) {
    const pdmpc_sweep::Batch& X = s->x;
    for (size_t m = 0; m < s->members.size(); ++m) {
        pdmpc_controller* c = s->members[m];
        c->x.out.assign(records + X.first[m], records + X.first[m + 1]);
        if (const int rc = choose_from_records(c, how, c->x.out.data(), X.first[m + 1] - X.first[m], follows_own(c, how))) return rc;
        gather_kept_records(c, follows_own(c, how));
        if (const int rc = pdmpc_controller_apply(c, c->out.data())) return rc;
    }
    return PDMPC_OK;
}

// the members' choices, each described by `how`, as ONE pdmpc_choice over the slots of the whole batch
void concatenate_choices(pdmpc_sweep* s, const BatchChoice& how) {
    pdmpc_sweep::Batch& X = s->x;
    const size_t M = s->members.size();
    X.lists.resize(M);
    ChoiceLists& A = X.all;
    A.cell_offset.assign(1, 0);
    A.cell_slot.clear();
    A.graph_offset.assign(1, 0);
    A.clear_picks();
    X.first_graph.assign(1, 0);
    X.first_cell.assign(1, 0);
    for (size_t m = 0; m < M; ++m) {
        pdmpc_controller* c = s->members[m];
        ChoiceLists& D = X.lists[m];
        how.describe(c, D);
        pick_chosen_plans(c, D, follows_own(c, how), how.graph_per_vehicle);
        const int32_t f = X.first[m], g0 = X.first_graph[m], c0 = X.first_cell[m], s0 = (int32_t)A.cell_slot.size(), p0 = (int32_t)A.pick_slot.size();
        for (int q = 1; q <= D.n_cells(); ++q) A.cell_offset.push_back(s0 + D.cell_offset[(size_t)q]);
        for (int32_t slot : D.cell_slot) A.cell_slot.push_back(f + slot);
        for (int g = 1; g <= D.n_graphs(); ++g) A.graph_offset.push_back(c0 + D.graph_offset[(size_t)g]);
        for (int32_t g : D.pick_graph) A.pick_graph.push_back(g < 0 ? -1 : g0 + g);
        for (int i = 1; i <= D.n_picks(); ++i) A.pick_offset.push_back(p0 + D.pick_offset[(size_t)i]);
        for (int32_t slot : D.pick_slot) A.pick_slot.push_back(f + slot);
        X.first_graph.push_back(g0 + D.n_graphs());
        X.first_cell.push_back(c0 + D.n_cells());
    }
    X.chosen.resize((size_t)X.first_graph.back());
    X.cell_cost.resize((size_t)X.first_cell.back());
    X.picks.resize((size_t)N_of(s));
}
// The lock-step behind a built batch (explorative or optimal-priority; t: when its build began): ONE pdmpc_plan_step_chosen for the
// concatenated batch with the members' choices concatenated, every member adopts its part -- as its own step that keeps the chosen
// plans only leaves it -- and applies it.
int sweep_batch_step(pdmpc_sweep* s, std::chrono::steady_clock::time_point t, const BatchChoice& how) {
    pdmpc_sweep::Batch& X = s->x;
    s->timing[0] = ms_since(t);
    const size_t M = s->members.size();
    // (the work of the last step as the members' own steps over a batch hand it over)
    auto pops_of = [&](int q) {
        const pdmpc_controller* c = s->members[(size_t)X.member[(size_t)q]];
        return c->tr.last_pops.size() == (size_t)c->sc.n ? c->tr.last_pops[(size_t)X.vehicle[(size_t)q]] : 0.0;
    };
    concatenate_choices(s, how);
    const pdmpc_choice ch = X.all.view();
    int rc = plan_built(target_of(s), X.prob, true, pops_of, s->members[0]->optimizer, s->timing, pdmpc_plan_step_chosen, &ch, X.chosen.data(), X.cell_cost.data(), X.picks.data());
    if (rc) return rc;
    t = std::chrono::steady_clock::now();
    for (size_t m = 0; m < M; ++m) {
        pdmpc_controller* c = s->members[m];
        how.adopt(c, X.lists[m], X.chosen.data() + X.first_graph[m], X.cell_cost.data() + X.first_cell[m], follows_own(c, how));
        c->x.out.clear();
        c->out.assign(X.picks.begin() + s->first[m], X.picks.begin() + s->first[m + 1]);
    }
    s->timing[4] = ms_since(t);
    t = std::chrono::steady_clock::now();
    for (size_t m = 0; m < M && !rc; ++m) rc = pdmpc_controller_apply(s->members[m], s->members[m]->out.data());
    s->timing[5] = ms_since(t);
    return rc;
}

// ---- centralized members
// what pdmpc_sweep_centralized_* refuse before any member advances
int sweep_centralized_refusal(pdmpc_sweep* s, bool needs_handle) {
    if (const int rc = batch_refusal(s, needs_handle)) return rc;
    for (pdmpc_controller* c : s->members)
        if (const int rc = centralized_refusal(c)) return rc;
    return PDMPC_OK;
}
// every live member's joint problem, one after the other
void sweep_centralized_build(pdmpc_sweep* s) {
    pdmpc_sweep::Centralized& X = s->cen;
    X.problem_offset.assign(1, 0);
    X.member.clear();
    X.in.clear();
    for (size_t m = 0; m < s->members.size(); ++m) {
        if (X.exhausted_at[m]) continue;
        pdmpc_controller* c = s->members[m];
        centralized_build(c);
        X.in.insert(X.in.end(), c->cen.in.begin(), c->cen.in.end());
        X.problem_offset.push_back((int32_t)X.in.size());
        X.member.push_back((int32_t)m);
    }
    X.built = true;
}
// the records of the built problems: every member's apply; a member whose search ran empty is retired, the others go on
int sweep_centralized_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records, bool keep_records) {
    pdmpc_sweep::Centralized& X = s->cen;
    for (size_t p = 0; p < X.member.size(); ++p) {
        const size_t m = (size_t)X.member[p];
        pdmpc_controller* c = s->members[m];
        const pdmpc_vehicle_out* r = records + X.problem_offset[p];
        if (keep_records) {  // (pdmpc_controller_records, as the member's own step leaves them)
            c->out.assign(r, r + c->sc.n);
            r = c->out.data();
        }
        const int rc = centralized_apply(c, r);
        if (rc == PDMPC_EXHAUSTED)
            X.exhausted_at[m] = c->tr.k;
        else if (rc)
            return rc;
    }
    X.built = false;  // (one apply per build: a retired member's problem is not applied again)
    return PDMPC_OK;
}
bool any_live(const pdmpc_sweep* s) {
    for (int32_t k : s->cen.exhausted_at)
        if (!k) return true;
    return false;
}
}  // namespace

extern "C" {

int pdmpc_sweep_create(pdmpc_handle* h, int32_t n_members, pdmpc_controller* const* members, pdmpc_sweep** out) {
    if (!out || n_members < 1 || !members) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_create: bad argument");
    *out = nullptr;
    int64_t total = 0;
    for (int m = 0; m < n_members; ++m) {
        const pdmpc_controller* c = members[m];
        if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_create: null member");
        if (c->h != h) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_create: a member was not created on the sweep's handle");
        if (c->sc.Hp != members[0]->sc.Hp) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_create: the members differ in Hp");
        if (c->optimizer != members[0]->optimizer) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_create: the members select different optimizers");
        for (int q = 0; q < m; ++q)
            if (members[q] == c) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_create: a member is listed twice");
        total += c->sc.n;
    }
    if (const int rc = refuse_beyond_handle(h, total, "pdmpc_sweep_create: the members have more vehicles than the handle's max_vehicles")) return rc;
    pdmpc_sweep* s = new pdmpc_sweep();
    s->h = h;
    s->members.assign(members, members + n_members);
    s->first.assign(1, 0);
    for (int m = 0; m < n_members; ++m) s->first.push_back(s->first.back() + members[m]->sc.n);
    s->cen.exhausted_at.assign((size_t)n_members, 0);
    *out = s;
    return PDMPC_OK;
}

int pdmpc_sweep_destroy(pdmpc_sweep* s) {
    delete s;
    return PDMPC_OK;
}

int pdmpc_sweep_build(pdmpc_sweep* s) {
    if (const int rc = sweep_refusal(s, !s, "null sweep")) return rc;
    return sweep_guard(s, sweep_build(s));
}

int pdmpc_sweep_problem(pdmpc_sweep* s, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                        const pdmpc_polygon_set** fallback, const int32_t** member, const int32_t** member_slot) {
    if (!s || !s->built) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_problem before pdmpc_sweep_build");
    expose(s->prob, n_slots, in, pred_offset, pred_index, fallback);
    if (member) *member = s->member.data();
    if (member_slot) *member_slot = s->member_slot.data();
    return PDMPC_OK;
}

int pdmpc_sweep_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records) {
    if (const int rc = sweep_refusal(s, !s || !records, "null argument", s && !s->built, "pdmpc_sweep_apply before pdmpc_sweep_build")) return rc;
    return sweep_guard(s, sweep_apply(s, records, false));
}

int pdmpc_sweep_step(pdmpc_sweep* s) {
    if (const int rc = sweep_refusal(s, !s || !s->h, "the sweep has no backend handle")) return rc;
    auto t = std::chrono::steady_clock::now();
    int rc = sweep_build(s);
    if (rc) return sweep_guard(s, rc);
    s->timing[0] = ms_since(t);
    s->timing[4] = 0;
    s->out.resize((size_t)N_of(s));
    // (the work of the last step as pdmpc_controller_step hands it over; a member's first step: 1 for each of its slots)
    auto pops_of = [&](int q) {
        const pdmpc_controller* c = s->members[(size_t)s->member[(size_t)q]];
        return c->tr.last_pops.size() == (size_t)c->sc.n ? c->tr.last_pops[(size_t)c->pri.order[(size_t)s->member_slot[(size_t)q]]] : 0.0;
    };
    rc = plan_built(target_of(s), s->prob, true, pops_of, s->members[0]->optimizer, s->timing, pdmpc_plan_step, s->out.data());
    if (rc) return sweep_guard(s, rc);
    t = std::chrono::steady_clock::now();
    rc = sweep_apply(s, s->out.data(), true);
    s->timing[5] = ms_since(t);
    return sweep_guard(s, rc);
}

int pdmpc_sweep_run(pdmpc_sweep* s, int32_t n_steps, double* ms) {
    return timed_steps(n_steps, ms, [&] { return pdmpc_sweep_step(s); });
}

int pdmpc_controller_set_group(pdmpc_controller* c, pdmpc_group* g, int32_t mode) {
    if (!c) return cfail(c, PDMPC_ERR_INVALID, "null argument");
    if (g)
        if (const int rc = group_refusal(g, mode, c->h, "pdmpc_controller_set_group")) return own(c, rc);
    c->group = g;
    c->group_mode = g ? mode : PDMPC_SHARD_AUTO;
    return PDMPC_OK;
}

int pdmpc_sweep_set_group(pdmpc_sweep* s, pdmpc_group* g, int32_t mode) {
    if (!s) return cfail(nullptr, PDMPC_ERR_INVALID, "null argument");
    if (g) {
        if (const int rc = group_refusal(g, mode, s->h, "pdmpc_sweep_set_group")) return rc;
        for (const pdmpc_controller* c : s->members)
            if (const int rc = group_refusal(g, mode, c->h, "pdmpc_sweep_set_group: a member")) return rc;
    }
    s->group = g;
    s->group_mode = g ? mode : PDMPC_SHARD_AUTO;
    return PDMPC_OK;
}

int pdmpc_sweep_last_timing(pdmpc_sweep* s, double* ms6) {
    if (!s || !ms6) return cfail(nullptr, PDMPC_ERR_INVALID, "null argument");
    for (int i = 0; i < 6; ++i) ms6[i] = s->timing[i];
    return PDMPC_OK;
}

int pdmpc_sweep_last_hdv_calls(pdmpc_sweep* s, int32_t* calls2) {
    if (!s || !calls2) return cfail(nullptr, PDMPC_ERR_INVALID, "null argument");
    std::copy(s->prep.hdv_calls, s->prep.hdv_calls + 2, calls2);
    return PDMPC_OK;
}

int pdmpc_sweep_last_prep_calls(pdmpc_sweep* s, int32_t* calls4) {
    if (!s || !calls4) return cfail(nullptr, PDMPC_ERR_INVALID, "null argument");
    std::copy(s->prep.prep_calls, s->prep.prep_calls + 4, calls4);
    return PDMPC_OK;
}

int pdmpc_sweep_explore_build(pdmpc_sweep* s, int32_t n_perm) {
    if (const int rc = explore_refusal(s, n_perm, false)) return rc;
    return sweep_guard(s, sweep_batch_build(s, BatchKind{n_perm, 0}));
}

int pdmpc_sweep_explore_problem(pdmpc_sweep* s, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                                const pdmpc_polygon_set** fallback, const int32_t** member, const int32_t** instance, const int32_t** vehicle, const int32_t** level) {
    if (!s || s->x.n_perm < 1) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_explore_problem before pdmpc_sweep_explore_build");
    return expose_batch(s->x, n_slots, in, pred_offset, pred_index, fallback, member, instance, vehicle, level);
}

int pdmpc_sweep_explore_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records) {
    if (const int rc = sweep_refusal(s, !s || !records, "null argument", s && s->x.n_perm < 1, "pdmpc_sweep_explore_apply before pdmpc_sweep_explore_build")) return rc;
    return sweep_guard(s, sweep_batch_apply(s, kExploreChoice, records));
}

int pdmpc_sweep_explore_step(pdmpc_sweep* s, int32_t n_perm) {
    if (const int rc = explore_refusal(s, n_perm, true)) return rc;
    const auto t = std::chrono::steady_clock::now();
    if (const int rc = sweep_batch_build(s, BatchKind{n_perm, 0})) return sweep_guard(s, rc);
    return sweep_guard(s, sweep_batch_step(s, t, kExploreChoice));
}

int pdmpc_sweep_explore_run(pdmpc_sweep* s, int32_t n_perm, int32_t n_steps, double* ms) {
    return timed_steps(n_steps, ms, [&] { return pdmpc_sweep_explore_step(s, n_perm); });
}

// ---- the optimal-priority step of a sweep
int pdmpc_sweep_optimal_build(pdmpc_sweep* s, int32_t max_instances) {
    if (const int rc = optimal_refusal(s, max_instances, false)) return rc;
    return sweep_guard(s, sweep_optimal_build(s, max_instances));
}

int pdmpc_sweep_optimal_problem(pdmpc_sweep* s, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index,
                                const pdmpc_polygon_set** fallback, const int32_t** member, const int32_t** instance, const int32_t** vehicle, const int32_t** level) {
    if (!s || !s->x.optimal) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_optimal_problem before pdmpc_sweep_optimal_build");
    return expose_batch(s->x, n_slots, in, pred_offset, pred_index, fallback, member, instance, vehicle, level);
}

int pdmpc_sweep_optimal_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records) {
    if (const int rc = sweep_refusal(s, !s || !records, "null argument", s && !s->x.optimal, "pdmpc_sweep_optimal_apply before pdmpc_sweep_optimal_build")) return rc;
    return sweep_guard(s, sweep_batch_apply(s, kOptimalChoice, records));
}

int pdmpc_sweep_optimal_step(pdmpc_sweep* s, int32_t max_instances) {
    if (const int rc = optimal_refusal(s, max_instances, true)) return rc;
    const auto t = std::chrono::steady_clock::now();
    if (const int rc = sweep_optimal_build(s, max_instances)) return sweep_guard(s, rc);
    const int rc = sweep_batch_step(s, t, kOptimalChoice);
    pdmpc_stats st{};
    if (!rc) s->optimal_calls[1] = pdmpc_get_last_stats(s->h, &st) == PDMPC_OK ? (int32_t)st.n_launches : 1;
    return sweep_guard(s, rc);
}

int pdmpc_sweep_optimal_run(pdmpc_sweep* s, int32_t max_instances, int32_t n_steps, double* ms) {
    return timed_steps(n_steps, ms, [&] { return pdmpc_sweep_optimal_step(s, max_instances); });
}

// ---- centralized members of a sweep
int pdmpc_sweep_centralized_build(pdmpc_sweep* s) {
    if (const int rc = sweep_centralized_refusal(s, false)) return rc;
    sweep_centralized_build(s);
    return PDMPC_OK;
}

int pdmpc_sweep_centralized_problem(pdmpc_sweep* s, int32_t* n_problems, const int32_t** problem_offset, const pdmpc_vehicle_in** in, const int32_t** member) {
    if (!s || !s->cen.built) return cfail(nullptr, PDMPC_ERR_INVALID, "pdmpc_sweep_centralized_problem before pdmpc_sweep_centralized_build");
    if (n_problems) *n_problems = (int32_t)s->cen.member.size();
    if (problem_offset) *problem_offset = s->cen.problem_offset.data();
    if (in) *in = s->cen.in.data();
    if (member) *member = s->cen.member.data();
    return PDMPC_OK;
}

int pdmpc_sweep_centralized_apply(pdmpc_sweep* s, const pdmpc_vehicle_out* records) {
    if (const int rc = sweep_refusal(s, !s || !records, "null argument", s && !s->cen.built, "pdmpc_sweep_centralized_apply before pdmpc_sweep_centralized_build")) return rc;
    return sweep_guard(s, sweep_centralized_apply(s, records, false));
}

int pdmpc_sweep_centralized_step(pdmpc_sweep* s) {
    if (const int rc = sweep_centralized_refusal(s, true)) return rc;
    if (!any_live(s)) return cfail(nullptr, PDMPC_EXHAUSTED, "pdmpc_sweep_centralized_step: every member's search is exhausted");
    auto t = std::chrono::steady_clock::now();
    sweep_centralized_build(s);
    pdmpc_sweep::Centralized& X = s->cen;
    s->timing[0] = ms_since(t);
    s->timing[4] = 0;
    X.out.resize(X.in.size());
    int rc = pdmpc_plan_joint(s->h, (int32_t)X.member.size(), X.problem_offset.data(), X.in.data(), X.out.data());
    if (rc) return sweep_guard(s, cfail(nullptr, rc, std::string("pdmpc_plan_joint: ") + pdmpc_last_error()));
    joint_call_timing(s->h, s->timing);
    t = std::chrono::steady_clock::now();
    rc = sweep_centralized_apply(s, X.out.data(), true);
    s->timing[5] = ms_since(t);
    return sweep_guard(s, rc);
}

int pdmpc_sweep_centralized_run(pdmpc_sweep* s, int32_t n_steps, double* ms) {
    return timed_steps(n_steps, ms, [&] { return pdmpc_sweep_centralized_step(s); });
}

int pdmpc_sweep_centralized_status(pdmpc_sweep* s, int32_t* exhausted_at) {
    if (!s || !exhausted_at) return cfail(nullptr, PDMPC_ERR_INVALID, "null argument");
    std::copy(s->cen.exhausted_at.begin(), s->cen.exhausted_at.end(), exhausted_at);
    return PDMPC_OK;
}

int pdmpc_sweep_optimal_last_calls(pdmpc_sweep* s, int32_t* calls2) {
    if (!s || !calls2) return cfail(nullptr, PDMPC_ERR_INVALID, "null argument");
    std::copy(s->optimal_calls, s->optimal_calls + 2, calls2);
    return PDMPC_OK;
}

}  // extern "C"
