// step_inputs.hpp — what a step reads of the traffic (step_controller.cpp, stage 2 of 9): the reference's functions that fill the parts
// of the controller's state a step's inputs are made of (step_types.hpp).  Every function takes the parts it reads and writes; the
// controller is not known here.
// What it restates (file:line relative to the reference root):
//   traffic info per step     HighLevelController.update_controlled_vehicles_traffic_info (hlc/controller/HighLevelController.m:167-270)
//   trim from measurement     MotionPrimitiveAutomaton.trim_from_values (hlc/model/motion_primitive_automaton/MotionPrimitiveAutomaton.m:193-236)
//   occupied areas            hlc/controller/common/get_occupied_areas.m:21-31, utility/translate_global.m:19-22
//   reference trajectory      hlc/controller/common/get_reference_trajectory.m:27-46, sample_reference_trajectory.m:1-99,
//                             get_arc_distance_to_endpoint.m:39-114, projection_2d.m:14-42
//   predicted lanelets        hlc/controller/common/get_predicted_lanelets.m:25-62, get_lanelets_boundary.m:18-68
//   coupling                  Coupler.m:31-32 (full), DistanceCoupler.m:15-50 (distance), ReachableSetCoupler.m:5-56 (reachable sets,
//                             reachable_sets.cpp / reachable_kernel.hip)
//   FCA inputs                FcaPrioritizer.m:11-92 (fca.cpp / fca_kernel.hip)
#pragma once
#include <algorithm>
#include <cmath>

#include "../../include/pdmpc_geometry.h"
#include "step_types.hpp"

namespace {
// MotionPrimitiveAutomaton.trim_from_values (:193-236): 1-based index of the closest trim
inline int trim_from_values(const Scenario& sc, double speed, double steering) {
    const int nt = (int)sc.trim_speed.size();
    if (steering == 0) {
        int best = -1;
        double bd = 0;
        for (int t = 0; t < nt; ++t) {
            if (sc.trim_steering[t] != 0) continue;
            const double d = std::fabs(sc.trim_speed[t] - speed);
            if (best < 0 || d < bd) {
                best = t;
                bd = d;
            }
        }
        return best + 1;
    }
    double sp_min = sc.trim_speed[0], sp_max = sc.trim_speed[0], st_min = sc.trim_steering[0], st_max = sc.trim_steering[0];
    for (int t = 1; t < nt; ++t) {
        sp_min = std::min(sp_min, sc.trim_speed[t]);
        sp_max = std::max(sp_max, sc.trim_speed[t]);
        st_min = std::min(st_min, sc.trim_steering[t]);
        st_max = std::max(st_max, sc.trim_steering[t]);
    }
    const double sp_s = sp_max - sp_min, st_s = st_max - st_min;
    int best = 0;
    double bd = 0;
    for (int t = 0; t < nt; ++t) {
        const double a = (sc.trim_speed[t] - sp_min) / sp_s - (speed - sp_min) / sp_s;
        const double b = (sc.trim_steering[t] - st_min) / st_s - (steering - st_min) / st_s;
        const double d = std::hypot(a, b);
        if (t == 0 || d < bd) {
            best = t;
            bd = d;
        }
    }
    return best + 1;
}

// get_occupied_areas.m:21-31 -> closed rectangles with and without the offset (translate_global.m:19-22)
inline void occupied_areas(double x, double y, double yaw, double length, double width, double offset, Poly& with_offset, Poly& plain) {
    static const double sx[5] = {-1, -1, 1, 1, -1}, sy[5] = {-1, 1, 1, -1, -1};
    const double c = std::cos(yaw), s = std::sin(yaw);
    with_offset.x.resize(5);
    with_offset.y.resize(5);
    plain.x.resize(5);
    plain.y.resize(5);
    for (int q = 0; q < 5; ++q) {
        const double xa = sx[q] * (length / 2 + offset), ya = sy[q] * (width / 2 + offset);
        with_offset.x[q] = c * xa + (-s) * ya + x;
        with_offset.y[q] = s * xa + c * ya + y;
        const double xb = sx[q] * (length / 2), yb = sy[q] * (width / 2);
        plain.x[q] = c * xb + (-s) * yb + x;
        plain.y[q] = s * xb + c * yb + y;
    }
}

inline double norm2(double a, double b) { return std::sqrt(a * a + b * b); }

// projection_2d.m:14-42 -> projected point and lambda
inline void projection_2d(double x1, double y1, double x2, double y2, double x3, double y3, double& xp, double& yp, double& lambda) {
    const double b = std::sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1));
    if (b != 0) {
        const double xn = (x2 - x1) / b, yn = (y2 - y1) / b;
        const double x31 = x3 - x1, y31 = y3 - y1;
        const double dot = xn * x31 + yn * y31;
        xp = x1 + dot * xn;
        yp = y1 + dot * yn;
        lambda = dot / b;
    } else {
        xp = x1;
        yp = y1;
        lambda = 0.0;
    }
}

// get_arc_distance_to_endpoint.m:39-114 (the part the sampler uses): projected point and 1-based idx_next
inline void arc_projection(double px, double py, const std::vector<double>& cx, const std::vector<double>& cy, double& xp, double& yp, int& idx_next) {
    const int np = (int)cx.size();
    int ic = 0;
    double best = 0;
    auto sq_of = [&](int i) { return (cx[i] - px) * (cx[i] - px) + (cy[i] - py) * (cy[i] - py); };
    for (int i = 0; i < np; ++i) {
        const double d = sq_of(i);
        if (i == 0 || d < best) {
            best = d;
            ic = i;
        }
    }
    int f, s;
    if (ic == 0) {
        f = 0;
        s = 1;
    } else if (ic == np - 1) {
        f = np - 2;
        s = np - 1;
    } else if (sq_of(ic - 1) <= sq_of(ic + 1)) {
        f = ic - 1;
        s = ic;
    } else {
        f = ic;
        s = ic + 1;
    }
    double lam;
    projection_2d(cx[f], cy[f], cx[s], cy[s], px, py, xp, yp, lam);
    const int idx_closest = ic + 1;
    idx_next = idx_closest;
    if ((0 <= lam && lam <= 0.5) || lam >= 1) idx_next = idx_closest < np ? idx_closest + 1 : 1;
    idx_next = std::max(2, idx_next);
}

// sample_reference_trajectory.m:1-99 (indices 1-based)
inline void sample_reference(int n_samples, const std::vector<double>& rx, const std::vector<double>& ry, double x_cur, double y_cur, const std::vector<double>& step,
                      std::vector<double>& out_x, std::vector<double>& out_y, std::vector<int32_t>& points_index, int* current_point_index = nullptr) {
    out_x.assign(n_samples, 0.0);
    out_y.assign(n_samples, 0.0);
    points_index.assign(n_samples, 0);
    double cx, cy;
    int point_index;
    arc_projection(x_cur, y_cur, rx, ry, cx, cy, point_index);
    if (current_point_index) *current_point_index = point_index;  // (sample_reference_trajectory.m: before the loop's wrap-around)
    const int n_line = (int)rx.size();
    const bool is_loop = norm2(rx[0] - rx[n_line - 1], ry[0] - ry[n_line - 1]) < 1e-8;
    bool at_end = point_index == n_line;
    int last = point_index - 1;
    if (is_loop && at_end) point_index = 1;
    auto X = [&](int i) { return rx[i - 1]; };
    auto Y = [&](int i) { return ry[i - 1]; };
    for (int i = 0; i < n_samples; ++i) {
        double remaining = norm2(cx - X(point_index), cy - Y(point_index));
        if (remaining > step[i] || point_index == n_line) {
            while (X(point_index) == X(last) && Y(point_index) == Y(last) && last > 1) --last;
            const double dx = X(point_index) - X(last), dy = Y(point_index) - Y(last);
            const double nn = norm2(dx, dy);
            cx = cx + step[i] * (dx / nn);
            cy = cy + step[i] * (dy / nn);
        } else {
            double reflength = remaining;
            while (remaining < step[i]) {
                reflength = remaining;
                cx = X(point_index);
                cy = Y(point_index);
                last = point_index;
                point_index = std::min(point_index + 1, n_line);
                at_end = point_index == n_line;
                if (is_loop && at_end) point_index = 1;
                remaining = remaining + norm2(cx - X(point_index), cy - Y(point_index));
            }
            const double dx = X(point_index) - X(last), dy = Y(point_index) - Y(last);
            const double nn = norm2(dx, dy);
            cx = cx + (step[i] - reflength) * (dx / nn);
            cy = cy + (step[i] - reflength) * (dy / nn);
        }
        out_x[i] = cx;
        out_y[i] = cy;
        points_index[i] = point_index;
    }
}

// get_predicted_lanelets.m:25-62 + get_lanelets_boundary.m:18-68 for vehicle v
inline void lanelet_boundary(const Scenario& sc, int v, const std::vector<int32_t>& ref_points_index, Poly& left, Poly& right) {
    const VehicleDef& V = sc.veh[v];
    left.x.clear();
    left.y.clear();
    right.x.clear();
    right.y.clear();
    if (V.lanelets_index.empty()) return;
    const int n_total = (int)V.px.size(), n_lan = (int)V.lanelets_index.size();
    int rpi[PDMPC_HP_MAX + 1], seen[PDMPC_HP_MAX + 2], predicted[PDMPC_HP_MAX + 2];
    int n_rpi = 0, n_seen = 0, n_pred = 0;
    for (int32_t p : ref_points_index) rpi[n_rpi++] = p;
    int index_add = rpi[n_rpi - 1] + 4;
    if (index_add > n_total) index_add -= n_total;
    rpi[n_rpi++] = index_add;
    for (int t = 0; t < n_rpi; ++t) {
        const int p = rpi[t];
        int q = 1;
        for (int u = 0; u < n_lan; ++u) q += p > V.points_index[u];
        if (std::find(seen, seen + n_seen, q) == seen + n_seen) seen[n_seen++] = q;  // unique(..., 'stable')
    }
    if (n_seen == 1) {
        int nxt = seen[0] + 1;
        if (nxt > n_lan) nxt = 1;
        seen[n_seen++] = nxt;
    }
    for (int t = 0; t < n_seen; ++t) predicted[n_pred++] = V.lanelets_index[std::min(seen[t], n_lan) - 1];
    auto append = [](Poly& dst, const Poly& src, int from, int to) {
        dst.x.insert(dst.x.end(), src.x.begin() + from, src.x.begin() + to);
        dst.y.insert(dst.y.end(), src.y.begin() + from, src.y.begin() + to);
    };
    // up to four points of the predecessor lanelet in front   :39-65
    int pos = (int)(std::find(V.lanelets_index.begin(), V.lanelets_index.end(), predicted[0]) - V.lanelets_index.begin());
    int pred = -1;
    if (pos != 0)
        pred = V.lanelets_index[pos - 1];
    else if (V.is_loop)
        pred = V.lanelets_index.back();
    if (pred >= 0) {
        const Poly& pl = sc.bl_left[pred - 1];
        const Poly& pr = sc.bl_right[pred - 1];
        const int num_added = std::min(4, std::min(pr.n() - 1, pl.n() - 1));
        append(left, pl, pl.n() - 1 - num_added, pl.n() - 1);
        append(right, pr, pr.n() - 1 - num_added, pr.n() - 1);
    }
    // then the boundaries of the predicted lanelets back to back, each without its last point but the final one   :26-32
    for (int q = 0; q < n_pred; ++q) {
        const Poly& bl = sc.bl_left[predicted[q] - 1];
        const Poly& br = sc.bl_right[predicted[q] - 1];
        const bool final_one = q + 1 == n_pred;
        append(left, bl, 0, final_one ? bl.n() : bl.n() - 1);
        append(right, br, 0, final_one ? br.n() : br.n() - 1);
    }
    for (int i = 0; i < left.n(); ++i) {
        left.x[i] = left.x[i] + V.tile_dx;
        left.y[i] = left.y[i] + V.tile_dy;
    }
    for (int i = 0; i < right.n(); ++i) {
        right.x[i] = right.x[i] + V.tile_dx;
        right.y[i] = right.y[i] + V.tile_dy;
    }
}

// FcaPrioritizer.m:11-92 on the step's reference points and the scenario's obstacles: the two per-member halves around the ONE
// grouped assessment of all FCA members of a step preparation (build_members) -- the reference points, their headings and the
// coupled pairs in `fca`, and the counts and priorities taken over (false, nothing written: Hp < 2, calculate_yaw needs two reference points)
inline bool fca_inputs(const Scenario& sc, const StepInputs& in, FcaInputs& fca) {
    const int n = sc.n, Hp = sc.Hp;
    if (Hp < 2) return false;
    fca.x.resize((size_t)n * Hp);
    fca.y.resize((size_t)n * Hp);
    fca.cos_yaw.resize((size_t)n * Hp);
    fca.sin_yaw.resize((size_t)n * Hp);
    for (int v = 0; v < n; ++v) {
        const double *px = in.ref_x[v].data(), *py = in.ref_y[v].data();
        for (int q = 0; q < Hp; ++q) {
            // calculate_yaw.m: central differences, one-sided at the ends (prioritizer.calculate_yaw)
            const int a = q == 0 ? 0 : (q == Hp - 1 ? Hp - 2 : q - 1), b = q == 0 ? 1 : (q == Hp - 1 ? Hp - 1 : q + 1);
            const double yaw = std::atan2(py[b] - py[a], px[b] - px[a]);
            const size_t i = (size_t)v * Hp + q;
            fca.x[i] = px[q];
            fca.y[i] = py[q];
            fca.cos_yaw[i] = std::cos(yaw);
            fca.sin_yaw[i] = std::sin(yaw);
        }
    }
    fca.pairs.clear();
    for (int a = 0; a < n; ++a)
        for_each_set(in.adjacency.data() + (size_t)a * n + a + 1, n - a - 1, [&](int q) {
            fca.pairs.push_back(a);
            fca.pairs.push_back(a + 1 + q);
        });
    fca.count.resize(n);
    return true;
}
inline void adopt_fca(int n, FcaInputs& fca, const int32_t* collisions, const int32_t* priorities) {
    std::copy(collisions, collisions + n, fca.count.begin());
    std::copy(priorities, priorities + n, fca.prio.begin());
}

// get_predicted_lanelets.m:44,61: the lanelet vehicle v is on, from the path point it is at (0: a scenario without lanelets)
inline int32_t current_lanelet(const Scenario& sc, int v, int current_point_index) {
    const VehicleDef& V = sc.veh[v];
    const int n_lan = (int)V.lanelets_index.size();
    if (n_lan == 0) return 0;
    int q = 1;
    for (int u = 0; u < n_lan; ++u) q += current_point_index > V.points_index[u];
    return V.lanelets_index[std::min(q, n_lan) - 1];
}

// ---- the stages of a step before its priorities, in their order
inline void traffic_info(const Scenario& sc, const Traffic& tr, StepInputs& in) {
    const int n = sc.n, Hp = sc.Hp;
    in.trims.assign(n, 0);
    // (resized, not re-created: the per-vehicle vectors keep their capacity from step to step; every one of them is rewritten below)
    in.occ_offset.resize(n);
    in.occ_plain.resize(n);
    in.ref_x.resize(n);
    in.ref_y.resize(n);
    in.v_ref.resize(n);
    in.bnd_left.resize(n);
    in.bnd_right.resize(n);
    in.current_lanelet.assign(n, 0);
    std::vector<double> step(Hp);
    std::vector<int32_t> pidx;
    for (int v = 0; v < n; ++v) {
        in.trims[v] = trim_from_values(sc, tr.mspeed[v], tr.msteer[v]);
        occupied_areas(tr.mx[v], tr.my[v], tr.myaw[v], sc.cfg.vehicle_length, sc.cfg.vehicle_width, sc.cfg.offset, in.occ_offset[v], in.occ_plain[v]);
        // get_reference_trajectory.m:27-46
        std::vector<double>& vref = in.v_ref[v];
        vref.assign(Hp, sc.veh[v].reference_speed);
        const double v_current = sc.trim_speed[in.trims[v] - 1];
        for (int q = 0; q < Hp; ++q) step[q] = (((q == 0 ? v_current : vref[q - 1]) + vref[q]) / 2) * sc.cfg.dt_seconds;
        int cpi = 0;
        sample_reference(Hp, sc.veh[v].px, sc.veh[v].py, tr.mx[v], tr.my[v], step, in.ref_x[v], in.ref_y[v], pidx, &cpi);
        lanelet_boundary(sc, v, pidx, in.bnd_left[v], in.bnd_right[v]);
        in.current_lanelet[v] = current_lanelet(sc, v, cpi);
    }
}

// reachable sets at the vehicles' poses (reachable_sets_at_pose, MotionPrimitiveAutomaton.m:649-687), closed by repeating the first
// vertex (HighLevelController.m:258-263)
inline void reachable_sets_at_poses(const Scenario& sc, const Traffic& tr, const StepInputs& in, ReachState& reach) {
    const int n = sc.n, Hp = sc.Hp;
    reach.sets.resize(n);
    reach.cos_yaw.resize(n);
    reach.sin_yaw.resize(n);
    for (int v = 0; v < n; ++v) {
        const double cy = std::cos(tr.myaw[v]), sy = std::sin(tr.myaw[v]);
        reach.cos_yaw[v] = cy;
        reach.sin_yaw[v] = sy;
        std::vector<Poly>& sets = reach.sets[v];
        sets.resize(Hp);
        for (int q = 0; q < Hp; ++q) {
            const int p = (in.trims[v] - 1) * Hp + q, a = sc.reach_off[p], m = sc.reach_off[p + 1] - a;
            Poly& P = sets[q];
            P.x.resize(m + 1);
            P.y.resize(m + 1);
            for (int r = 0; r < m; ++r) pdmpc_move_point(cy, sy, tr.mx[v], tr.my[v], sc.reach_x[a + r], sc.reach_y[a + r], &P.x[r], &P.y[r]);
            P.x[m] = P.x[0];
            P.y[m] = P.y[0];
        }
    }
}

// lanelet bounding of those sets (bound_reachable_sets.m, HighLevelController.m:241-246): every step's sets when parallel
// predecessors read them (all_steps), else step Hp only (the coupler's)
// ... its two per-member halves around the bounding call of a step preparation (build_members): the raw lanelet polygons in
// reach.lan_*, and the bounded sets in reach.bound_* taken over as the parallel predecessors' obstacles
inline void lanelet_polygons(const Scenario& sc, const StepInputs& in, ReachState& reach) {
    const int n = sc.n;
    reach.lan_off.assign((size_t)n + 1, 0);
    reach.lan_x.clear();
    reach.lan_y.clear();
    for (int v = 0; v < n; ++v) {  // the left boundary, then the reversed right boundary (get_lanelets_boundary.m:69-74)
        const Poly &L = in.bnd_left[v], &R = in.bnd_right[v];
        reach.lan_x.insert(reach.lan_x.end(), L.x.begin(), L.x.end());
        reach.lan_y.insert(reach.lan_y.end(), L.y.begin(), L.y.end());
        reach.lan_x.insert(reach.lan_x.end(), R.x.rbegin(), R.x.rend());
        reach.lan_y.insert(reach.lan_y.end(), R.y.rbegin(), R.y.rend());
        reach.lan_off[v + 1] = (int32_t)reach.lan_x.size();
    }
    reach.lan_x.push_back(0.0);  // (never empty)
    reach.lan_y.push_back(0.0);
}
inline void adopt_bounded_sets(const Scenario& sc, ReachState& reach, bool all_steps) {
    if (!all_steps) return;  // (else the parallel predecessors' obstacles are the bounded sets)
    for (int v = 0; v < sc.n; ++v)
        for (int q = 0; q < sc.Hp; ++q) {
            const int o = v * sc.Hp + q, a = reach.bound_off[o], m = reach.bound_off[o + 1] - a;
            Poly& P = reach.sets[v][q];
            P.x.assign(reach.bound_x.begin() + a, reach.bound_x.begin() + a + m);
            P.y.assign(reach.bound_y.begin() + a, reach.bound_y.begin() + a + m);
        }
}

// in.adjacency by the host rules: full and distance coupling (ReachableSetCoupler.m:5-56 is a call of the step preparation, which has
// written the member's block into in.adjacency already)
inline void couple(const Scenario& sc, const Traffic& tr, StepInputs& in) {
    const int n = sc.n;
    if (sc.cfg.coupling == PDMPC_COUPLING_REACHABLE_SET) return;
    in.adjacency.assign((size_t)n * n, 0);
    if (sc.cfg.coupling == PDMPC_COUPLING_FULL) {
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) at(in.adjacency, n, a, b) = a != b;
    } else if (sc.cfg.coupling == PDMPC_COUPLING_DISTANCE) {
        const double vmax = *std::max_element(sc.trim_speed.begin(), sc.trim_speed.end());
        const double max_distance = 2 * vmax * sc.cfg.dt_seconds * sc.Hp;
        // (hypot(dx, dy) >= max(|dx|, |dy|), also as rounded: a pair farther apart along one axis alone is not coupled — most pairs of
        // a tiled network.  That test runs over the whole row, the distance itself over the survivors.)
        for (int a = 0; a < n; ++a) {
            uint8_t* row = in.adjacency.data() + (size_t)a * n;
            const double xa = tr.mx[a], ya = tr.my[a];
            const double *px = tr.mx.data(), *py = tr.my.data();
            for (int b = a + 1; b < n; ++b) row[b] = (uint8_t)(!(std::fabs(xa - px[b]) > max_distance) & !(std::fabs(ya - py[b]) > max_distance));
            for_each_set(row + a + 1, n - a - 1, [&](int q) {
                const int b = a + 1 + q;
                row[b] = std::hypot(xa - px[b], ya - py[b]) <= max_distance;
                at(in.adjacency, n, b, a) = row[b];
            });
        }
    }
}
}  // namespace
