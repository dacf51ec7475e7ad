// step_controller.cpp — the caller's side of the optimizer boundary, natively: one MPC time step of the prioritized
// sequential controller around pdmpc_plan_step.  Host code only (no device code in this file).
//
// What it restates (file:line relative to the reference root), the C++ twin of p-dmpc_amd/pdmpc/controller.py, in stages, each a header
// that names only the ones before it and says at its head what it restates (`make host-parts` compiles each alone):
// step_types.hpp (the records), step_inputs.hpp (what a step reads of the traffic), step_hdv.hpp (human-driven vehicles: a member's HDV
// state, the solo and the batch path of the traffic stage), step_priorities.hpp (couplings -> a prioritization), step_state.hpp (the
// controller as the parts that are written together), step_assembly.hpp (a member's StepProblem), step_batch.hpp (the batches of
// prioritizations and the choice among their plans), step_prepare.hpp (the step preparation over a span of members: build_members),
// step_centralized.hpp (centralized control: the joint problem).  This file: planning a built problem (plan_built), the steps and their
// loops, the sweep, every entry point of the C ABI, and
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
#include "step_types.hpp"  // the stages, in their order
#include "step_inputs.hpp"
#include "step_hdv.hpp"
#include "step_priorities.hpp"
#include "step_state.hpp"
#include "step_assembly.hpp"
#include "step_batch.hpp"
#include "step_prepare.hpp"
#include "step_centralized.hpp"

namespace {
// ---- the shared paths of the steps below (templates: outside the extern "C" block)
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

// ---- how a step ends that the controller takes alone
PlanTarget target_of(const pdmpc_controller* c) { return {c->h, c->group, c->group_mode}; }
// a failure inside a step the controller takes alone is the controller's error too (the global message has it either way)
int own(pdmpc_controller* c, int rc) {
    if (rc) c->err = g_cerr;
    return rc;
}
// what a stage on narrow state refused (its code and its text) as the controller's error
int refused(pdmpc_controller* c, int rc, const std::string& why) { return rc ? cfail(c, rc, why) : (int)PDMPC_OK; }
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
        rc = hdv_with_map(H, c->sc.Hp, pdmpc_hdv_check_map_host);
        if (rc) return cfail(c, rc, std::string("pdmpc_controller_set_hdvs: ") + pdmpc_last_error());
    }
    c->hdv = std::move(H);  // (with no map slot noted: the next step looks for the map on the handle)
    return PDMPC_OK;
}

int pdmpc_controller_set_hdv_drivers(pdmpc_controller* c, const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const double* start_distance,
                                     const double* v_des, const double* params) {
    if (!c || !route_offset || !route_lanelet || !closed || !start_distance || !v_des || !params) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_drivers: null argument");
    std::string why;
    return refused(c, hdv_set_drivers(c->hdv, c->sc.cfg.dt_seconds, route_offset, route_lanelet, closed, start_distance, v_des, params, &why), why);
}

int pdmpc_controller_hdv_driver_state(pdmpc_controller* c, int32_t* state_seg, double* state_u, double* x, double* y, double* yaw, double* speed, double* gap) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    const HdvTraffic& H = c->hdv;
    if (!H.driven) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_hdv_driver_state before pdmpc_controller_set_hdv_drivers");
    auto out = [](const auto& from, auto* to) {  // (any of them may be NULL)
        if (to) std::copy(from.begin(), from.end(), to);
    };
    out(H.seg, state_seg), out(H.u, state_u), out(H.x, x), out(H.y, y), out(H.yaw, yaw), out(H.speed, speed), out(H.gap, gap);
    return PDMPC_OK;
}

int pdmpc_controller_set_hdv_recording(pdmpc_controller* c, int32_t T, const double* x, const double* y, const double* yaw) {
    if (!c || T < 1 || !x || !y || !yaw) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_recording: bad argument");
    std::string why;
    return refused(c, hdv_set_recording(c->hdv, T, x, y, yaw, &why), why);
}

int pdmpc_controller_set_hdv_poses(pdmpc_controller* c, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw) {
    if (!c || !x || !y || !cos_yaw || !sin_yaw) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_poses: null argument");
    std::string why;
    return refused(c, hdv_set_poses(c->hdv, "pdmpc_controller_set_hdv_poses", "set", x, y, nullptr, cos_yaw, sin_yaw, &why), why);
}

int pdmpc_controller_set_hdv_measurements(pdmpc_controller* c, const double* x, const double* y, const double* yaw) {
    if (!c || !x || !y || !yaw) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_set_hdv_measurements: null argument");
    std::string why;
    return refused(c, hdv_set_poses(c->hdv, "pdmpc_controller_set_hdv_measurements", "measured", x, y, yaw, nullptr, nullptr, &why), why);
}

int pdmpc_controller_hdv_info(pdmpc_controller* c, int32_t* n_hdv, const int32_t** closest_offset, const int32_t** closest_index, int32_t* n_rows, const int32_t** row_hdv,
                              const int32_t** set_offset, const double** set_x, const double** set_y, const uint8_t** set_flags, const uint8_t** adjacency) {
    if (!c) return cfail(nullptr, PDMPC_ERR_INVALID, "null controller");
    const HdvTraffic& H = c->hdv;
    if (H.n == 0 || H.closest_off.empty()) return cfail(c, PDMPC_ERR_INVALID, "pdmpc_controller_hdv_info before a step was built with HDVs");
    auto out = [](auto* to, auto value) {  // (any of them may be NULL)
        if (to) *to = value;
    };
    out(n_hdv, H.n), out(closest_offset, H.closest_off.data()), out(closest_index, H.closest_idx.data()), out(n_rows, H.n_rows), out(row_hdv, H.row_hdv.data());
    out(set_offset, H.set_off.data()), out(set_x, H.set_x.data()), out(set_y, H.set_y.data()), out(set_flags, H.set_flags.data()), out(adjacency, H.adjacency.data());
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
