// step_assembly.hpp — a member's step around the step preparation (step_controller.cpp, stage 6 of 9): its seeds, its priorities, and
// the stages begin_step, assemble_step and finish_step that build its StepProblem from the controller's parts.
// What it restates (file:line relative to the reference root):
//   obstacle assembly         PrioritizedController.plan / consider_predecessors / consider_successors (:297-324, 449-566)
//   published on exhaustion   handle_graph_search_exhaustion / plan_fallback (:602-611, 678-718)
#pragma once
#include <cmath>

#include "step_state.hpp"

namespace {
thread_local std::string g_cerr;

struct SetBuilder {  // builds a pdmpc_polygon_set whose arrays live in the controller's arena; one builder at a time
    Assembly& c;
    explicit SetBuilder(Assembly& as) : c(as) {
        c.sb_off.assign(1, 0);
        c.sb_x.clear();
        c.sb_y.clear();
    }
    void add(const Poly& p) {
        c.sb_x.insert(c.sb_x.end(), p.x.begin(), p.x.end());
        c.sb_y.insert(c.sb_y.end(), p.y.begin(), p.y.end());
        c.sb_off.push_back((int32_t)c.sb_x.size());
    }
    pdmpc_polygon_set finish() {
        pdmpc_polygon_set s;
        s.n_polygons = (int32_t)c.sb_off.size() - 1;
        const size_t np = c.sb_x.size();
        int32_t* off = (int32_t*)c.arena.take(c.sb_off.size() * sizeof(int32_t));
        double* x = (double*)c.arena.take((np + 1) * sizeof(double));  // (one entry more: never an empty array)
        double* y = (double*)c.arena.take((np + 1) * sizeof(double));
        std::memcpy(off, c.sb_off.data(), c.sb_off.size() * sizeof(int32_t));
        if (np) {
            std::memcpy(x, c.sb_x.data(), np * sizeof(double));
            std::memcpy(y, c.sb_y.data(), np * sizeof(double));
        }
        x[np] = y[np] = 0.0;
        s.offset = off;
        s.x = x;
        s.y = y;
        return s;
    }
};

inline int cfail(pdmpc_controller* c, int code, const std::string& msg) {
    g_cerr = msg;
    if (c) c->err = msg;
    return code;
}

// ---- a member's step around the step preparation: the seeds, the priorities, and the stages of pdmpc_controller_build_step in its order
// RandStream('mt19937ar', Seed = time_step + vehicle_index) of every slot (MonteCarloTreeSearch.m:31-32; PrioritizedController.m:335-341
// calls run_optimizer with obj.k, so every instance of a batch draws the same stream for the same vehicle)
inline void set_seeds(int time_step, StepProblem& P, const std::vector<int32_t>& vehicle_of_slot) {
    P.seeds.resize(vehicle_of_slot.size());
    for (size_t s = 0; s < vehicle_of_slot.size(); ++s) P.seeds[s] = (uint32_t)(time_step + vehicle_of_slot[s] + 1);
}

// priorities -> c->pri.directed (FCA: the counts and priorities of the member's group in the step preparation's assessment)
inline void direct_by_priorities(pdmpc_controller* c, const int32_t* fca_collisions, const int32_t* fca_priorities) {
    const int n = c->sc.n;
    std::vector<uint8_t>& directed = c->pri.directed;
    if (c->sc.cfg.priority_strategy == PDMPC_PRIORITY_COLORING) {
        coloring_directed(c->in.adjacency, n, directed);
        return;
    }
    // constant priorities = vehicle index (ConstantPrioritizer.m:14-20); random and FCA priorities as below
    c->fca.prio.resize(n);
    for (int v = 0; v < n; ++v) c->fca.prio[v] = v + 1;
    if (c->sc.cfg.priority_strategy == PDMPC_PRIORITY_RANDOM) {
        random_priorities(c->tr.k, n, c->fca.prio);
    } else if (c->sc.cfg.priority_strategy == PDMPC_PRIORITY_FCA) {
        adopt_fca(n, c->fca, fca_collisions, fca_priorities);
    }
    direct_by(c->in.adjacency, n, c->fca.prio.data(), directed);
}

// A member's step in three parts around the step preparation, which runs once for all members that are built together: everything
// before it (advances the time step; P: what the step reads of the reachable sets),
inline int begin_step(pdmpc_controller* c, StepPrep& P) {
    const int n = c->sc.n;
    const bool reach_parallel = c->reach.parallel_mode == PDMPC_PARALLEL_REACHABLE_SETS;
    const bool reach = c->sc.cfg.coupling == PDMPC_COUPLING_REACHABLE_SET || reach_parallel;  // a feature reads the reachable sets
    if (reach && !c->reach.has)
        return cfail(c, PDMPC_ERR_INVALID, "reachable-set coupling / parallel coupling by reachable sets need pdmpc_controller_set_reachability first");
    c->tr.k += 1;
    c->as.arena.reset();
    if (c->as.exploring) {
        c->as.obst_memo.resize((size_t)n);
        c->as.dyn_memo.resize((size_t)n);
        for (int v = 0; v < n; ++v) {
            c->as.obst_memo[(size_t)v].clear();
            c->as.dyn_memo[(size_t)v].clear();
        }
    }
    c->as.fb_of.assign(n, pdmpc_polygon_set());
    c->as.fb_done.assign(n, 0);
    c->as.empty_done = false;
    traffic_info(c->sc, c->tr, c->in);
    if (reach) reachable_sets_at_poses(c->sc, c->tr, c->in, c->reach);
    bool bounded = false;  // (not on scenarios without lanelets)
    if (reach && c->reach.lanelet_bounding)
        for (int v = 0; v < n && !bounded; ++v) bounded = !c->sc.veh[v].lanelets_index.empty();
    P.reach_parallel = reach_parallel;
    P.reach = reach;
    P.bounded = bounded;
    return PDMPC_OK;
}
// c->pri.directed -> sequential couplings, levels, slot order and the per-slot inputs of pdmpc_plan_step (the arena is the caller's
// to clear: the explorative step keeps several problems alive side by side)
inline int assemble_step(pdmpc_controller* c, bool seq_given = false) {
    const int n = c->sc.n, Hp = c->sc.Hp;
    // (seq_given: c->pri.directed_seq is the caller's -- the explorative step swaps single couplings of the base prioritization)
    // who a vehicle is coupled with, as lists: the loops below visit a vehicle's few couplings, not rows and columns of the matrices
    Lists &dir_succ = c->as.ls_dir_succ, &dir_pred = c->as.ls_dir_pred, &seq_succ_own = c->as.ls_seq_succ, &seq_pred_own = c->as.ls_seq_pred;
    lists_by_row(c->pri.directed, n, dir_succ);
    lists_by_column(n, dir_succ, dir_pred);
    bool uncut = false;
    const Grouping how = {c->sc.cfg.max_num_CLs, c->sc.cfg.weight_strategy, c->sc.trim_speed, c->sc.cfg.dt_seconds, c->sc.Hp, c->tr.mx, c->tr.my, c->tr.k};
    if (!seq_given && !group(n, how, c->pri.directed, dir_succ, dir_pred, c->as.kahn, c->pri.directed_seq, c->pri.levels, uncut)) return cfail(c, PDMPC_ERR_INVALID, "coupling graph has a cycle");
    if (!uncut) {  // (uncut: the sequential coupling is `directed` itself, levels and lists included)
        lists_by_row(c->pri.directed_seq, n, seq_succ_own);
        lists_by_column(n, seq_succ_own, seq_pred_own);
        if (!kahn_lists(seq_succ_own, n, c->pri.levels, c->as.kahn)) return cfail(c, PDMPC_ERR_INVALID, "coupling graph has a cycle");
    }
    const Lists& seq_pred = uncut ? dir_pred : seq_pred_own;
    // slot order: by level, vehicles of a level in index order (a counting sort over the levels 1 .. n)
    c->pri.order.resize(n);
    c->pri.slot_of.assign(n, 0);
    {
        std::vector<int>& first = c->as.kahn.cur;  // (scratch) first[l] = slot of level l's first vehicle
        first.assign((size_t)n + 2, 0);
        for (int i = 0; i < n; ++i) ++first[(size_t)c->pri.levels[i] + 1];
        for (int l = 1; l <= n + 1; ++l) first[l] += first[l - 1];
        for (int i = 0; i < n; ++i) {
            const int s = first[(size_t)c->pri.levels[i]]++;
            c->pri.order[s] = i;
            c->pri.slot_of[i] = s;
        }
    }
    // ---- per slot inputs
    c->prob.in.assign(n, pdmpc_vehicle_in());
    c->prob.fb.assign(n, pdmpc_polygon_set());
    c->prob.pred_offset.assign(n + 1, 0);
    c->prob.pred_index.clear();
    for (int s = 0; s < n; ++s) {
        const int i = c->pri.order[s];
        pdmpc_vehicle_in& I = c->prob.in[s];
        std::memset(&I, 0, sizeof I);
        I.x0 = c->tr.mx[i];
        I.y0 = c->tr.my[i];
        I.yaw0 = c->tr.myaw[i];
        I.trim0 = c->in.trims[i];
        I.ref_x = c->in.ref_x[i].data();
        I.ref_y = c->in.ref_y[i].data();
        I.v_ref = c->in.v_ref[i].data();
        I.n_left = c->in.bnd_left[i].n();
        I.n_right = c->in.bnd_right[i].n();
        I.left_x = c->in.bnd_left[i].x.data();
        I.left_y = c->in.bnd_left[i].y.data();
        I.right_x = c->in.bnd_right[i].x.data();
        I.right_y = c->in.bnd_right[i].y.data();
        auto add_shifted = [](SetBuilder& b, const std::vector<Poly>& shapes) {  // del_first_rpt_last without the temporary
            for (size_t q = 1; q < shapes.size(); ++q) b.add(shapes[q]);
            b.add(shapes.back());
        };
        // who contributes (in the order the sets are built in): consider_predecessors (:449-506) — sequential predecessors are handed
        // over on the device; the others contribute their previous plan shifted by one step (parallel_coupling_previous_trajectory,
        // :409-447) —, then consider_successors (:508-566)
        const bool memo = c->as.exploring && n <= 512;  // (one prioritization: every set is built once anyway)
        MemoKey ok, dk;
        if (memo) {
            std::memset(&ok, 0, sizeof ok);
            std::memset(&dk, 0, sizeof dk);
        }
        int ol[512], dpl[512], dsl[512], no = 0, ndp = 0, nds = 0;  // (the contributors in the order the sets are built in)
        std::vector<int> big;  // (n > 512: the lists on the heap)
        int *olp = ol, *dplp = dpl, *dslp = dsl;
        if (n > 512) {
            big.resize((size_t)3 * n);
            olp = big.data();
            dplp = big.data() + n;
            dslp = big.data() + 2 * n;
        }
        for (const int32_t* q = dir_pred.begin(i); q != dir_pred.end(i); ++q) {
            const int j = *q;
            if (at(c->pri.directed_seq, n, j, i)) continue;
            // (parallel_coupling_reachability, :391-407: the predecessor's reachable sets exist from the first step on)
            if (c->reach.parallel_mode == PDMPC_PARALLEL_REACHABLE_SETS || (c->tr.info_old[j].present && c->tr.k > 1)) {
                dplp[ndp++] = j;
                if (memo) dk.w[j >> 6] |= 1ull << (j & 63);
            }
        }
        for (const int32_t* q = dir_succ.begin(i); q != dir_succ.end(i); ++q) {
            const int j = *q;
            if (c->sc.cfg.constraint_from_successor == PDMPC_SUCCESSOR_AREA_OF_STANDSTILL) {
                if (std::fabs(c->tr.mspeed[j]) < 0.01) {  // :536-540
                    olp[no++] = j;
                    if (memo) ok.w[j >> 6] |= 1ull << (j & 63);
                }
            } else if (c->sc.cfg.constraint_from_successor == PDMPC_SUCCESSOR_AREA_OF_PREVIOUS_TRAJECTORY) {
                if (c->tr.info_old[j].present) {
                    dslp[nds++] = j;
                    if (memo) dk.w[8 + (j >> 6)] |= 1ull << (j & 63);
                }
            }
        }
        auto build_obst = [&]() {
            SetBuilder obst(c->as);
            for (const Poly& o : c->sc.static_obstacles) obst.add(o);
            for (int q = 0; q < no; ++q) obst.add(c->in.occ_offset[olp[q]]);
            return obst.finish();
        };
        auto build_dyn = [&]() {
            SetBuilder dyn(c->as);
            for (int q = 0; q < ndp; ++q) {
                if (c->reach.parallel_mode == PDMPC_PARALLEL_REACHABLE_SETS) {
                    for (const Poly& p : c->reach.sets[dplp[q]]) dyn.add(p);
                } else {
                    add_shifted(dyn, c->tr.info_old[dplp[q]].shapes);
                }
            }
            for (int q = 0; q < nds; ++q) add_shifted(dyn, c->tr.info_old[dslp[q]].shapes);
            return dyn.finish();
        };
        if (memo) {
            auto& om = c->as.obst_memo[(size_t)i];
            if (const pdmpc_polygon_set* hit = om.find(ok)) {
                I.obstacles = *hit;
            } else {
                I.obstacles = build_obst();
                om.keys.push_back(ok);
                om.sets.push_back(I.obstacles);
            }
            auto& dm = c->as.dyn_memo[(size_t)i];
            if (const pdmpc_polygon_set* hit = dm.find(dk)) {
                I.dynamic_obstacles = *hit;
            } else {
                I.dynamic_obstacles = build_dyn();
                dm.keys.push_back(dk);
                dm.sets.push_back(I.dynamic_obstacles);
            }
        } else {
            I.obstacles = build_obst();
            I.dynamic_obstacles = build_dyn();
        }
        if (!c->as.empty_done) {
            SetBuilder none(c->as);
            c->as.empty_set = none.finish();
            c->as.empty_done = true;
        }
        // the rows of the HDVs adjacent to i, the same in every prioritization of the step (IterationData.filter :113)
        I.hdv_reachable_sets = c->hdv.n > 0 ? c->hdv.set_of(i) : c->as.empty_set;
        // sequential predecessors as slots
        for (const int32_t* q = seq_pred.begin(i); q != seq_pred.end(i); ++q) c->prob.pred_index.push_back(c->pri.slot_of[*q]);
        c->prob.pred_offset[s + 1] = (int32_t)c->prob.pred_index.size();
        // what the vehicle publishes if its search is exhausted: its standstill rectangle (:602-611) or the previous plan
        // shifted by one step (:678-718)
        if (!c->as.fb_done[i]) {  // (a function of the vehicle alone: shared by the prioritizations of an explorative step)
            SetBuilder fbs(c->as);
            const bool standstill = c->sc.trim_speed[c->in.trims[i] - 1] == 0;
            if (standstill && c->sc.cfg.constraint_from_successor != PDMPC_SUCCESSOR_NONE) {
                for (int q = 0; q < Hp; ++q) fbs.add(c->in.occ_plain[i]);
            } else if (c->tr.info_old[i].present) {
                add_shifted(fbs, c->tr.info_old[i].shapes);
            }
            c->as.fb_of[i] = fbs.finish();
            c->as.fb_done[i] = 1;
        }
        c->prob.fb[s] = c->as.fb_of[i];
    }
    c->prob.pred_index.push_back(0);
    return PDMPC_OK;
}
// ... and everything after the step preparation
inline int finish_step(pdmpc_controller* c, const int32_t* fca_collisions, const int32_t* fca_priorities) {
    direct_by_priorities(c, fca_collisions, fca_priorities);
    if (const int rc = assemble_step(c)) return rc;
    set_seeds(c->tr.k, c->prob, c->pri.order);
    c->x.built_last = false;
    return PDMPC_OK;
}
}  // namespace
