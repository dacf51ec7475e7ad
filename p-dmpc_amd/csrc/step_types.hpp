// step_types.hpp — the records of the native step controller (step_controller.cpp, stage 1 of 9): polygons, matrix lists, plans,
// vehicles, a step problem, a prioritization, a choice, and the parts of the controller's state that a step's inputs are made of.  Names
// nothing but the C ABI.
// (Every stage header compiles alone under -Wunused-function -Wunused-member-function, `make host-parts`: its helpers are inline, and a
// member function that only a later stage calls is [[maybe_unused]].  Those warnings pass over both markers, so that compile checks the
// layering only; the same target compiles all stages and the .cpp as one text with the markers taken out, which is the check for dead helpers.)
#pragma once
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pdmpc.h"

namespace {
struct Poly {  // 2 x V, MATLAB [x; y]
    std::vector<double> x, y;
    [[maybe_unused]] int n() const { return (int)x.size(); }
};

// (offsets, x, y) vectors viewed as a polygon set of off.size() - 1 polygons (no copy: the vectors outlive the view)
inline pdmpc_polygon_set view_polygons(const std::vector<int32_t>& off, const std::vector<double>& x, const std::vector<double>& y) {
    pdmpc_polygon_set ps;
    ps.n_polygons = (int32_t)off.size() - 1;
    ps.offset = off.data();
    ps.x = x.data();
    ps.y = y.data();
    return ps;
}

// the non-zero entries of a matrix as lists: by row (idx[off[i] .. off[i + 1]) = the columns of row i) or by column (the rows of
// column j), ascending in both forms
struct Lists {
    std::vector<int32_t> off, idx, fill;  // (fill: scratch of lists_by_column)
    const int32_t* begin(int i) const { return idx.data() + off[i]; }
    const int32_t* end(int i) const { return idx.data() + off[i + 1]; }
};

struct Plan {  // what the controller keeps of a vehicle's ControlResultsInfo (ControlResultsInfo.m:5-17)
    bool present = false;
    bool needs_fallback = false;
    bool exhausted = false;
    std::vector<Poly> shapes;         // Hp
    std::vector<int32_t> trims;       // Hp
    std::vector<double> yx, yy, yyaw; // Hp
    int32_t n_expanded = 0;
    [[maybe_unused]] void resize(size_t m) { shapes.resize(m), trims.resize(m), yx.resize(m), yy.resize(m), yyaw.resize(m); }
};

struct VehicleDef {
    double x_start, y_start, yaw_start, reference_speed;
    std::vector<double> px, py;             // reference path
    std::vector<int32_t> lanelets_index;    // 1-based lanelet ids along the loop (empty: no lanelets, circle scenario)
    std::vector<int32_t> points_index;      // 1-based index of the last path point of each of those lanelets
    bool is_loop;
    double tile_dx, tile_dy;
};

// A step problem in the C ABI's form (what pdmpc_plan_step takes; the polygon sets its entries point to live in the arena of the
// controller that built them), with the sampled optimizer's seed and the expected work per slot.  One record wherever a problem lives.
struct StepProblem {
    std::vector<pdmpc_vehicle_in> in;
    std::vector<pdmpc_polygon_set> fb;  // per slot: what its vehicle publishes if its search is exhausted
    std::vector<int32_t> pred_offset, pred_index;
    std::vector<uint32_t> seeds;   // time_step + vehicle_index (set_seeds; empty for a kept instance, which is never planned by itself)
    std::vector<double> weights;   // plan_built's scratch
    int n() const { return (int)in.size(); }
    // a backend call on the problem: call(h, n_slots, in, pred_offset, pred_index, fallback, rest ...)
    template <class Call, class... Rest>
    int plan(Call call, pdmpc_handle* h, Rest... rest) const {
        return call(h, n(), in.data(), pred_offset.data(), pred_index.data(), fb.data(), rest...);
    }
    // ... and its twin over a group: call(g, n_slots, in, pred_offset, pred_index, fallback, weights, mode, rest ...)
    template <class Call, class... Rest>
    int plan_on_group(Call call, pdmpc_group* g, const double* expected_work, int32_t mode, Rest... rest) const {
        return call(g, n(), in.data(), pred_offset.data(), pred_index.data(), fb.data(), expected_work, mode, rest...);
    }
};
// ... and the same five as every *_problem entry point hands them out
inline void expose(const StepProblem& P, int32_t* n_slots, const pdmpc_vehicle_in** in, const int32_t** pred_offset, const int32_t** pred_index, const pdmpc_polygon_set** fallback) {
    if (n_slots) *n_slots = P.n();
    if (in) *in = P.in.data();
    if (pred_offset) *pred_offset = P.pred_offset.data();
    if (pred_index) *pred_index = P.pred_index.data();
    if (fallback) *fallback = P.fb.data();
}
// Where a built problem is planned: on the handle, or (g set) over a group whose rank 0 is that handle (pdmpc_controller_set_group,
// pdmpc_sweep_set_group).  The step preparation stays on the handle either way.
struct PlanTarget {
    pdmpc_handle* h = nullptr;
    pdmpc_group* g = nullptr;
    int32_t mode = PDMPC_SHARD_AUTO;
};

// A prioritization of the step's traffic state: the controller's own, and every instance of an explorative or optimal-priority batch
struct Instance {
    std::vector<uint8_t> directed, directed_seq;  // n x n row-major
    std::vector<int32_t> levels, order, slot_of;
    [[maybe_unused]] void take_couplings(const Instance& of) {
        directed = of.directed;
        directed_seq = of.directed_seq;
    }
};

// A choice among the plans of a batch as pdmpc_choose_host / pdmpc_plan_step_chosen take it (pdmpc_choice): the lists, kept from step to step
struct ChoiceLists {
    std::vector<int32_t> cell_offset, cell_slot, graph_offset, pick_graph, pick_offset, pick_slot;
    std::vector<int32_t> graph_of;  // the explorative choice: per vehicle its sub-graph
    int n_cells() const { return cell_offset.empty() ? 0 : (int)cell_offset.size() - 1; }
    int n_graphs() const { return graph_offset.empty() ? 0 : (int)graph_offset.size() - 1; }
    int n_picks() const { return (int)pick_graph.size(); }
    [[maybe_unused]] void clear_picks() {
        pick_graph.clear();
        pick_slot.clear();
        pick_offset.assign(1, 0);
    }
    [[maybe_unused]] pdmpc_choice view() const {
        pdmpc_choice ch{};
        ch.n_cells = n_cells();
        ch.n_graphs = n_graphs();
        ch.n_picks = n_picks();
        ch.cell_offset = cell_offset.data();
        ch.cell_slot = cell_slot.data();
        ch.graph_offset = graph_offset.data();
        ch.pick_graph = pick_graph.data();
        ch.pick_offset = pick_offset.data();
        ch.pick_slot = pick_slot.data();
        return ch;
    }
};

inline uint8_t& at(std::vector<uint8_t>& m, int n, int i, int j) { return m[(size_t)i * n + j]; }
inline uint8_t at(const std::vector<uint8_t>& m, int n, int i, int j) { return m[(size_t)i * n + j]; }

// f(j) for the non-zero entries j of a matrix row, ascending.  Rows of the coupling matrices are mostly zero (a vehicle is coupled with
// the few around it): eight entries per test.
template <class F>
inline void for_each_set(const uint8_t* row, int n, F&& f) {
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        uint64_t w;
        std::memcpy(&w, row + j, 8);
        if (w == 0) continue;
        for (int q = 0; q < 8; ++q)
            if (row[j + q]) f(j + q);
    }
    for (; j < n; ++j)
        if (row[j]) f(j);
}

inline void lists_by_row(const std::vector<uint8_t>& M, int n, Lists& L) {
    L.off.assign((size_t)n + 1, 0);
    L.idx.clear();
    for (int i = 0; i < n; ++i) {
        for_each_set(M.data() + (size_t)i * n, n, [&](int j) { L.idx.push_back(j); });
        L.off[i + 1] = (int32_t)L.idx.size();
    }
}
inline void lists_by_column(int n, const Lists& by_row, Lists& L) {
    L.off.assign((size_t)n + 1, 0);
    for (int32_t j : by_row.idx) ++L.off[j + 1];
    for (int j = 0; j < n; ++j) L.off[j + 1] += L.off[j];
    L.idx.resize(by_row.idx.size());
    L.fill.assign(L.off.begin(), L.off.end() - 1);
    for (int i = 0; i < n; ++i)
        for (const int32_t* q = by_row.begin(i); q != by_row.end(i); ++q) L.idx[L.fill[*q]++] = i;
}

inline double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

// ---- the controller's state that a step's inputs are made of, by who writes it (the rest: step_state.hpp; step_inputs.hpp fills them)
// the scenario and the automaton: written by pdmpc_controller_create / pdmpc_controller_set_reachability only
struct Scenario {
    pdmpc_controller_config cfg{};
    int n = 0, Hp = 0;
    std::vector<VehicleDef> veh;
    std::vector<Poly> bl_left, bl_right;  // per lanelet boundary polylines (RoadDataCommonRoad.get_lanelet_boundary)
    std::vector<Poly> static_obstacles;
    std::vector<double> trim_speed, trim_steering;
    // the automaton's local reachable hulls, polygon trim * Hp + k (pdmpc_controller_set_reachability)
    std::vector<int32_t> reach_off;
    std::vector<double> reach_x, reach_y;
};
// what is carried from step to step: written by pdmpc_controller_apply (k: advanced by begin_step)
struct Traffic {
    int k = 0;
    std::vector<double> mx, my, myaw, mspeed, msteer;  // measurements
    std::vector<Plan> info_old, infos;
    std::vector<double> last_pops;  // per vehicle: nodes its search popped in the last step (the next step's expected work, pdmpc_set_step_weights)
};
// what a step reads of the traffic: rewritten by traffic_info and the coupling every step
struct StepInputs {
    std::vector<int32_t> trims;
    std::vector<Poly> occ_offset, occ_plain;
    std::vector<std::vector<double>> ref_x, ref_y, v_ref;
    std::vector<Poly> bnd_left, bnd_right;
    std::vector<int32_t> current_lanelet;  // the lanelet id every vehicle is on (get_predicted_lanelets.m:44,61); 0 without lanelets
    std::vector<uint8_t> adjacency;  // n x n row-major
};
// Human-driven vehicles (pdmpc_controller_set_hdvs): what the traffic call is made with -- the scenario's lanelets
// flattened, the lanelet graph, the local sets of the HDVs' automaton, tiles and the last measured poses --, what the step's ONE call
// left (pdmpc_controller_hdv_info), and per CAV the rows of the HDVs adjacent to it as the set its searches receive.
struct HdvTraffic {
    int n = 0;  // HDVs; 0: none set, and a step is built as without this struct
    bool measured = false;
    int32_t map_slot = -1;       // the handle's map slot this map was found in or uploaded to by the last step's traffic stage, and
    int64_t map_generation = 0;  // ... the slot's generation then: while it has not moved the map is still there (0: not known)
    std::vector<int32_t> lan_off, succ_off, succ_idx;
    std::vector<double> left_x, left_y, right_x, right_y;
    std::vector<uint8_t> rel;
    int n_trims = 0;
    std::vector<int32_t> local_off;
    std::vector<double> local_x, local_y;
    std::vector<double> tile_dx, tile_dy, x, y, yaw, cos_yaw, sin_yaw;
    std::vector<int32_t> trim;
    std::vector<double> cav_tile_dx, cav_tile_dy;
    int32_t n_rows = 0;
    std::vector<int32_t> closest_off, closest_idx, row_hdv, set_off;
    std::vector<double> set_x, set_y;
    std::vector<uint8_t> set_flags, adjacency;
    std::vector<std::vector<int32_t>> cav_off;
    std::vector<std::vector<double>> cav_x, cav_y;
    // Drivers (pdmpc_controller_set_hdv_drivers; include/pdmpc_hdv.h: the driver model): the HDVs move themselves, one step at every built
    // step but the first after the drivers were set (whose "measurement" is the placement).  seg / u: the state of the last built step.
    bool driven = false;
    int driven_builds = 0;  // built steps since the drivers were set
    std::vector<int32_t> route_off, route_id, seg, new_seg;
    std::vector<uint8_t> route_closed;
    std::vector<double> u, new_u, v_des, speed, gap;
    double drive_params[4] = {0.0, 0.0, 0.0, 0.0};
    // A recording (pdmpc_controller_set_hdv_recording): row min(built steps, T) - 1 of T recorded poses is the measurement of a built step
    int rec_T = 0, rec_builds = 0;
    std::vector<double> rec_x, rec_y, rec_yaw;
    // CAV v's set (valid until the next step's call)
    [[maybe_unused]] pdmpc_polygon_set set_of(int v) const { return view_polygons(cav_off[(size_t)v], cav_x[(size_t)v], cav_y[(size_t)v]); }
    // ... rebuilt from the call's output: the rows of the adjacent HDVs in row order, polygon row * Hp + k (vectorize_all_obstacles.m:33-62)
    [[maybe_unused]] void gather(int n_cav, int Hp) {
        cav_off.resize((size_t)n_cav);
        cav_x.resize((size_t)n_cav);
        cav_y.resize((size_t)n_cav);
        for (int v = 0; v < n_cav; ++v) {
            std::vector<int32_t>& off = cav_off[(size_t)v];
            std::vector<double>&cx = cav_x[(size_t)v], &cy = cav_y[(size_t)v];
            off.assign(1, 0);
            cx.clear();
            cy.clear();
            for (int r = 0; r < n_rows; ++r) {
                if (!adjacency[(size_t)v * n + row_hdv[(size_t)r]]) continue;
                for (int k = 0; k < Hp; ++k) {
                    const int32_t a = set_off[(size_t)r * Hp + k], b = set_off[(size_t)r * Hp + k + 1];
                    cx.insert(cx.end(), set_x.begin() + a, set_x.begin() + b);
                    cy.insert(cy.end(), set_y.begin() + a, set_y.begin() + b);
                    off.push_back((int32_t)cx.size());
                }
            }
            cx.push_back(0.0);  // (never an empty array)
            cy.push_back(0.0);
        }
    }
};
// reachable sets: the switches, and per step every vehicle's Hp sets at its pose, closed (HighLevelController.m:219-263)
struct ReachState {
    int parallel_mode = PDMPC_PARALLEL_PREVIOUS_TRAJECTORY;
    bool has = false;  // the scenario holds the local hulls
    std::vector<std::vector<Poly>> sets;
    std::vector<double> cos_yaw, sin_yaw;
    // lanelet bounding of those sets (pdmpc_controller_set_lanelet_bounding): the raw lanelet polygons and the bounded sets of the step
    bool lanelet_bounding = false;
    std::vector<int32_t> bound_off, lan_off;
    std::vector<double> bound_x, bound_y, lan_x, lan_y;
};
// priorities of the random and FCA strategies (1-based per vehicle) and the FCA inputs of the step: every reference point with the
// cos / sin of its calculate_yaw heading, the coupled pairs a < b, the collision counts, the scenario's obstacles as one polygon set
struct FcaInputs {
    std::vector<int32_t> prio, pairs, count, obst_off;
    std::vector<double> x, y, cos_yaw, sin_yaw, obst_x, obst_y;
};
}  // namespace
