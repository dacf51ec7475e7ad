// step_centralized.hpp — centralized control (step_controller.cpp, stage 9 of 9): the joint problem of a controller's vehicles and the
// plant update from its records.  No coupling, no priorities, no levels: the step preparation (build_members) has no part in it.
// What it restates (file:line relative to the reference root), the C++ twin of p-dmpc_amd/pdmpc/centralized.py:
//   the step                  CentralizedController.controller (hlc/controller/centralized/CentralizedController.m:33-59)
//   no fallback               handle_graph_search_exhaustion of that controller (:61-70): an exhausted search ends the run
//   plant                     Simulation.apply (plant/Simulation.m:86-100)
#pragma once
#include "step_batch.hpp"

namespace {
// what every centralized entry point refuses before anything advances: more vehicles than a joint problem holds, and a handle whose
// checker the joint search does not run
inline int centralized_refusal(pdmpc_controller* c) {
    if (c->hdv.n > 0) return cfail(c, PDMPC_ERR_INVALID, "centralized control: the joint search has no check against HDV sets (pdmpc_controller_set_hdvs)");
    if (c->sc.n > PDMPC_JOINT_MAX) return cfail(c, PDMPC_ERR_CAPACITY, "centralized control: the controller has more than PDMPC_JOINT_MAX vehicles");
    if (c->h) {
        pdmpc_config hc{};
        int32_t has_mpa = 0;
        if (pdmpc_get_config(c->h, &hc, &has_mpa) != PDMPC_OK) return cfail(c, PDMPC_ERR_INVALID, "bad backend handle");
        if (hc.checker != PDMPC_CHECK_SAT) return cfail(c, PDMPC_ERR_INVALID, "centralized control: joint searches use the separating-axis checker (PDMPC_CHECK_SAT)");
    }
    return PDMPC_OK;
}

// CentralizedController.build_iters: advances the time step, the traffic info of the step, then row v of the reference's iter for every
// vehicle.  The scenario's obstacles are ONE set that every entry points to, so the packer and the joint kernel hold it once.
inline void centralized_build(pdmpc_controller* c) {
    const int n = c->sc.n;
    c->tr.k += 1;
    c->as.arena.reset();
    traffic_info(c->sc, c->tr, c->in);
    SetBuilder obst(c->as);
    for (const Poly& o : c->sc.static_obstacles) obst.add(o);
    const pdmpc_polygon_set obstacles = obst.finish();
    SetBuilder none(c->as);
    c->as.empty_set = none.finish();
    c->as.empty_done = true;
    c->cen.in.assign((size_t)n, pdmpc_vehicle_in());
    for (int i = 0; i < n; ++i) {
        pdmpc_vehicle_in& I = c->cen.in[(size_t)i];
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
        I.obstacles = obstacles;
        I.dynamic_obstacles = c->as.empty_set;
        I.hdv_reachable_sets = c->as.empty_set;
    }
    c->cen.built = true;
}

// the records of the joint problem in vehicle order: PDMPC_EXHAUSTED if the search ran empty (nothing is applied), else the plant update
inline int centralized_apply(pdmpc_controller* c, const pdmpc_vehicle_out* recs) {
    const int n = c->sc.n;
    const int n_trims = (int)c->sc.trim_speed.size();
    bool exhausted = false;
    for (int i = 0; i < n; ++i) {
        const pdmpc_vehicle_out& r = recs[i];
        if (r.status != PDMPC_OK && r.status != PDMPC_EXHAUSTED) return cfail(c, PDMPC_ERR_HIP, "a result record carries an error status: not a planning result");
        if (r.status == PDMPC_OK && (r.predicted_trims[0] < 1 || r.predicted_trims[0] > n_trims)) return cfail(c, PDMPC_ERR_INVALID, "a result record's first trim is not a trim of the scenario");
        exhausted = exhausted || r.status == PDMPC_EXHAUSTED;
    }
    if (exhausted)
        return cfail(c, PDMPC_EXHAUSTED, "graph search exhausted at time step " + std::to_string(c->tr.k) + ": the centralized controller has no fallback");
    // Simulation.apply (Simulation.m:86-100)
    for (int i = 0; i < n; ++i) {
        const pdmpc_vehicle_out& r = recs[i];
        c->tr.mx[i] = r.y_predicted[0][0];
        c->tr.my[i] = r.y_predicted[0][1];
        c->tr.myaw[i] = r.y_predicted[0][2];
        c->tr.mspeed[i] = c->sc.trim_speed[r.predicted_trims[0] - 1];
        c->tr.msteer[i] = c->sc.trim_steering[r.predicted_trims[0] - 1];
    }
    return PDMPC_OK;
}
}  // namespace
