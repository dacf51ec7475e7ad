// sampled_ensemble_kernel.hip — the sampled optimizer (MonteCarloTreeSearch.m:40-249) planned as a seed ensemble
// (pdmpc_set_sampled_ensemble): E members per vehicle, one wavefront each, the cheapest collision-free plan wins on
// the device.
//
// The grid is count * E workgroups; block b is member b % E of slot b / E (reverse_dispatch turns the slots round as in the other
// sampled kernels), so all members of a slot lie below the blocks of its successors.  A member is sampled_budget_kernel.hip's search,
// statement for statement (a third copy: the two existing files keep their device code bit for bit), at any budget, with three
// things of its own: its seed PDMPC_SAMPLED_MEMBER_SEED(seed, e), its record member_out[slot * E + e] in place of out[slot], and its
// tree (LDS, or tree slot * E + e of the HBM buffer).  Every member reads the same soups: the literal ones and the areas its
// predecessors published in out[].
//
// The protocol of a slot (split-K's "last block reduces"):
//   every member   writes its record, its tree size and its 16-byte entry (status, expansions, final cost) with vector stores, drains
//                  them, then lane 0: release fence (agent), s_waitcnt vmcnt(0), relaxed agent-scope fetch_add on the slot's ticket.
//   ticket E - 1   (the member that arrives last, whichever it is) one agent-scope acquire; reads the E entries with vector loads
//                  (lane e reads entry e: never through the scalar cache); picks the winner -- the smallest cost among the members
//                  with PDMPC_OK, compared with <, members in ascending order, so the lowest index wins a tie --; copies the
//                  chosen record to out[slot] with vector loads and stores; drains; releases and stores the done flag like the
//                  other sampled kernels.  No member OK: member 0's record (PDMPC_EXHAUSTED, with the fallback areas its search
//                  published in it).  A member that timed out waiting for a predecessor: that member's record (PDMPC_ERR_HIP).
//   No member waits for a member, and a member that does not draw the last ticket is finished: a workgroup depends only on the done
//   flags of predecessor slots, whose blocks all lie below it.
// Tickets: the host clears the tickets of the launched slots on the stream ahead of every launch (api.cpp: launch_range) -- also right
// after a launch that failed half-way, which a last arriver that restores them is not.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_math.h"
#include "sampled_ensemble.h"

namespace {

#include "wave_primitives.hpp"
#include "search_state.hpp"
#include "edge_checks.hpp"
#include "mt19937_device.hpp"

// the j-th (0-based) set bit of the successor mask of (trim, step), as a 0-based trim index; -1 if there is none
__device__ __forceinline__ int nth_successor(const lds_mask64* row, int nw, int j) {
    for (int w = 0; w < nw; ++w) {
        uint64_t m = row[w];
        const int c = __builtin_popcountll(m);
        if (j < c) {
            for (int q = 0; q < j; ++q) m &= m - 1;
            return w * 64 + __builtin_ctzll(m);
        }
        j -= c;
    }
    return -1;
}
__device__ __forceinline__ int successor_count(const lds_mask64* row, int nw) {
    int c = 0;
    for (int w = 0; w < nw; ++w) c += __builtin_popcountll(row[w]);
    return c;
}

// ---- mt19937ar one twist at a time (sampled_budget_kernel.hip's)
__device__ __forceinline__ void mt_seed_wave(uint32_t seed, lds_u32* mt, int lane) {
    if (lane == 0) {
        uint32_t x = seed ? seed : 5489u;  // (Seed = 0 is the generator's default seed)
        mt[0] = x;
        for (int i = 1; i < 624; ++i) {
            x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
            mt[i] = x;
        }
    }
    wave_sync();
}
__device__ __forceinline__ void mt_twist_wave(lds_u32* mt, int lane) {
    for (int c = 0; c < 624; c += PDMPC_WAVE) {
        const int k = c + lane;
        uint32_t v = 0;
        if (k < 624) {
            const uint32_t y = (mt[k] & 0x80000000u) | (mt[k == 623 ? 0 : k + 1] & 0x7fffffffu);
            v = mt[k < 227 ? k + 397 : k - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        wave_sync();
        if (k < 624) mt[k] = v;
        wave_sync();
    }
}
__device__ __forceinline__ double mt_double(const lds_u32* mt, int q) {
    const uint32_t a = mt_temper(mt[2 * q]) >> 5, b = mt_temper(mt[2 * q + 1]) >> 6;
    return (a * 67108864.0 + b) * (1.0 / 9007199254740992.0);
}

// ---- the tree's rows, in LDS or in HBM (sampled_budget_kernel.hip's)
template <bool IN_LDS>
struct Tree;
template <>
struct Tree<true> {
    LDS_AS uint16_t* p;
    __device__ __forceinline__ uint32_t get(int i) const { return (uint32_t)p[i]; }
    __device__ __forceinline__ void put(int i, uint32_t v) const { p[i] = (uint16_t)v; }
    __device__ __forceinline__ static void sync() { wave_sync(); }
};
template <>
struct Tree<false> {
    uint16_t* p;  // (neither const nor __restrict__: nothing of it may be read through the scalar cache)
    __device__ __forceinline__ uint32_t get(int i) const { return (uint32_t)__hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
    __device__ __forceinline__ void put(int i, uint32_t v) const { p[i] = (uint16_t)v; }
    __device__ __forceinline__ static void sync() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        wave_sync();
    }
};

// what a member's search leaves besides its record
struct MemberResult {
    int status, n_expanded, n_nodes;
    double cost;
};

// One member's search: sampled_budget_body with the record, the seed and the tree as arguments.  It returns instead of publishing.
template <bool IN_LDS>
__device__ __forceinline__ MemberResult member_search(const SampledBudgetArgs& A, LDS_AS unsigned char* lsm, int slot, uint32_t seed, pdmpc_vehicle_out* __restrict__ O,
                                                      uint16_t* hbm_tree) {
    const int lane = threadIdx.x;
    const int Hp = A.Hp, n = A.n_trims, nw = A.n_words;
    const int budget = A.budget, node_cap = A.node_cap;
    const DevVehicle* __restrict__ V = A.veh + slot;
    const int n_random = Hp * budget;  // rand(stream, 1, Hp * n_expansions_max)                                 :53
    const double inf = __longlong_as_double(0x7ff0000000000000LL);

    // ---- LDS carve (layout_sampled_budget)
    lds_mask64* l_mask = (lds_mask64*)(lsm + A.lds.mask);
    lds_i16* l_mi = (lds_i16*)(lsm + A.lds.man_index);
    lds_pose* l_pose = (lds_pose*)(lsm + A.lds.pose);
    lds_f64* l_rx = (lds_f64*)(lsm + A.lds.ref);
    lds_f64* l_ry = l_rx + PDMPC_HP_MAX;
    lds_u32* l_path = (lds_u32*)(lsm + A.lds.path);
    lds_i32* l_soff = (lds_i32*)(l_path + PDMPC_HP_MAX + 2);
    lds_i32* l_hoff = l_soff + PDMPC_HP_MAX + 1;
    lds_i32* l_lit = l_hoff + PDMPC_HP_MAX + 1;  // literal soup length per step
    lds_d2* l_soup = (lds_d2*)(lsm + A.lds.soup);
    lds_u32* l_mt = (lds_u32*)(lsm + A.lds.rand);  // the generator's state
    Tree<IN_LDS> T;
    if constexpr (IN_LDS)
        T.p = (LDS_AS uint16_t*)(lsm + A.lds.tree16);
    else
        T.p = hbm_tree;

    CheckCtx C;
    C.l_area = (const lds_d2*)(lsm + A.lds.area);
    C.g_area = (const d2*)A.man_area;
    C.l_soup = l_soup;
    C.l_soff = l_soff;
    C.l_hoff = l_hoff;
    C.areas_in_lds = A.areas_in_lds;
    C.Hp = Hp;
    C.checker = A.checker;
    C.sh = (lds_d2*)(lsm + A.lds.shape);
    C.cand = (lds_u32*)(lsm + A.lds.cand);
    C.tally = (LDS_AS unsigned long long*)(C.sh + 2 * PDMPC_VMAX);
    if (lane == 0) {
        C.tally[0] = 0;
        C.tally[1] = 0;
    }

    // ---- prologue: tables, reference points, record defaults, the first twist, obstacle soups, predecessors
    {
        const int mask_bytes = Hp * n * nw * 8;
        stage16(l_mask, A.succ_mask, (mask_bytes + 15) / 16, lane);
        stage16(l_mi, A.man_index, (n * n * 2 + 15) / 16, lane);
        stage16(l_pose, A.man_pose, A.n_man * 2, lane);
        if (A.areas_in_lds) stage16(lsm + A.lds.area, A.man_area, A.n_man * 3 * PDMPC_VMAX, lane);
    }
    if (lane < Hp) {
        l_rx[lane] = V->ref_x[lane];
        l_ry[lane] = V->ref_y[lane];
    }
    {
        double* od = (double*)O;
        const int nd = (int)(sizeof(pdmpc_vehicle_out) / 8);
        const int y0 = (int)(offsetof(pdmpc_vehicle_out, y_predicted) / 8);
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        for (int i = lane; i < nd; i += PDMPC_WAVE) od[i] = (i >= y0 && i < y0 + PDMPC_HP_MAX * 3) ? qnan : 0.0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    mt_seed_wave(seed, l_mt, lane);
    mt_twist_wave(l_mt, lane);
    int twist = 0;  // the state holds doubles [312 * twist, 312 * (twist + 1)) of the stream
    const int n_pred = V->n_pred;
    const int pred_cols = n_pred * PDMPC_VMAX;
    {
        int off = 0;
        for (int k = 0; k < Hp; ++k) {
            const int a = V->lit_off[k], b = V->lit_off[k + 1];
            if (lane == 0) {
                l_soff[k] = off;
                l_lit[k] = b - a;
            }
            stage16(l_soup + off, (const d2*)A.points + a, b - a, lane);
            off += (b - a) + pred_cols;
        }
        if (lane == 0) l_soff[Hp] = off;
        for (int k = 0; k < Hp; ++k) {
            const int a = V->hdv_off[k], b = V->hdv_off[k + 1];
            if (lane == 0) l_hoff[k] = off;
            stage16(l_soup + off, (const d2*)A.points + a, b - a, lane);
            off += (b - a);
        }
        if (lane == 0) l_hoff[Hp] = off;
        stage16(l_soup + off, (const d2*)A.points + V->ll_off, V->ll_len, lane);
        C.ll_base = off;
    }
    C.ll_len = uni_i(V->ll_len);
    wave_sync();
    if (n_pred > 0) {
        // predecessors of this step (PrioritizedController.m:476-491): wait for every done flag, then their areas into the soups
        const int32_t* pred = A.pred + V->pred_off;
        bool dep_timeout = false;
        for (int p = 0; p < n_pred && !dep_timeout; ++p) {
            uint32_t spins = 0;
            while (__hip_atomic_load(A.done_flag + pred[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != A.epoch) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > A.spin_limit) {
                    dep_timeout = true;
                    break;
                }
            }
        }
        if (dep_timeout) {
            // the watchdog: the slot gets this status and the host plans the call again in resident slices (api.cpp: plan_packed_growing)
            if (lane == 0) {
                O->status = PDMPC_ERR_HIP;
                O->n_hp = Hp;
            }
            return {PDMPC_ERR_HIP, 0, 0, inf};
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wave_sync();
        // (lane-dependent indices: the records are read with vector loads, after the acquire — never through the scalar cache)
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        for (int idx = lane; idx < Hp * pred_cols; idx += PDMPC_WAVE) {
            const int k = idx / pred_cols;
            const int r = idx - k * pred_cols;
            const int p = r / PDMPC_VMAX;
            const int v = r - p * PDMPC_VMAX;
            const pdmpc_vehicle_out* PO = A.out + pred[p];
            const int cols = PO->shape_cols[k];
            const double sx = PO->shapes[k][0][v], sy = PO->shapes[k][1][v];
            d2 pt;
            pt.x = v < cols ? sx : qnan;
            pt.y = v < cols ? sy : qnan;
            l_soup[l_soff[k] + l_lit[k] + r] = pt;
        }
    }
    wave_sync();

    // ---- tree with root node (MonteCarloTreeSearch.m:60-74); node ids are 1-based, row 0 is unused.  The root's whole row:
    //      children(1:size(root_successor_trims, 2), 1) = 1, the others 0, no parent, its trim
    const double root_x = V->x0, root_y = V->y0, root_yaw = V->yaw0;
    {
        const int rc = successor_count(l_mask + ((size_t)0 * n + (V->trim0 - 1)) * nw, nw);
        if (lane < PDMPC_SB_ROW) T.put(1 * PDMPC_SB_ROW + lane, lane < PDMPC_SB_FANOUT ? (lane < rc ? 1u : 0u) : (lane == PDMPC_SB_TRIM ? (uint32_t)V->trim0 : 0u));
    }
    T.sync();
    int n_nodes = 1, n_expansions = 0, n_traversals = 0;
    bool is_finished = false, have_best = false;
    double best_cost = 0.0;
    int best_node = 0;

    while (n_expansions < budget && !is_finished && n_nodes + Hp < node_cap) {  // :89 (the last condition never binds: sampled_budget.h)
        int node_id = 1;
        double solution_cost = 0.0;
        double px = root_x, py = root_y, pyaw = root_yaw;
        bool is_valid = false;
        int child_position = 0, node_parent = 0;
        for (int i_step = 1; i_step <= Hp; ++i_step) {  // :95
            is_valid = false;
            ++n_traversals;
            // the node's row: children in lanes 0 .. 15, its parent and its trim behind them
            const uint32_t row = lane < PDMPC_SB_ROW ? T.get(node_id * PDMPC_SB_ROW + lane) : 0u;
            // trim_positions = find(children(:, node_id))                                              :100
            const unsigned long long nz = __ballot(lane < PDMPC_SB_FANOUT && row != 0u);
            const int n_trims = __builtin_popcountll(nz);
            if (n_trims != 0) {
                // child_position = trim_positions(ceil(random_numbers(n_traversals) * n_trims))          :105
                // (the reference draws Hp * n_expansions_max numbers and would fail beyond them; the index stays inside the slot's numbers)
                const int ri = (n_traversals <= n_random ? n_traversals : n_random) - 1;
                while (ri >= (twist + 1) * PDMPC_SB_TWIST) {
                    mt_twist_wave(l_mt, lane);
                    ++twist;
                }
                const double r = uni_d(mt_double(l_mt, ri - twist * PDMPC_SB_TWIST));
                int pick = (int)ceil(r * (double)n_trims) - 1;
                if (pick < 0) pick = 0;  // (r == 0 would index element 0 in the reference: an error there)
                unsigned long long m = nz;
                for (int q = 0; q < pick; ++q) m &= m - 1;
                child_position = __builtin_ctzll(m);
            } else {
                if (node_id != 1) {  // remove edge to node without children                              :108-112
                    const int parent_id = (int)lane_u(row, PDMPC_SB_PARENT);
                    if (lane < PDMPC_SB_FANOUT && T.get(parent_id * PDMPC_SB_ROW + lane) == (uint32_t)node_id) T.put(parent_id * PDMPC_SB_ROW + lane, 0u);
                    T.sync();
                    break;
                }
                is_finished = true;  // :114-115
                break;
            }
            // ---- expand node                                                                       :120-138
            const int parent_trim = (int)lane_u(row, PDMPC_SB_TRIM);
            const int goal_trim = nth_successor(l_mask + ((size_t)(i_step - 1) * n + (parent_trim - 1)) * nw, nw, child_position) + 1;
            const int m = (int)l_mi[(parent_trim - 1) * n + (goal_trim - 1)];
            const double dx = l_pose[m].dx, dy = l_pose[m].dy, dyaw = l_pose[m].dyaw;
            const int ncols = l_pose[m].n_cols;
            double s, c;
            pdmpc_sincos(pyaw, &s, &c);
            const double sx0 = px, sy0 = py;  // start_pose
            {
                // node_pose = node_pose + transform * maneuver.dpose: rows accumulated left to right, zeros included
                const double t0 = c * dx + (-s) * dy + 0.0 * dyaw;
                const double t1 = s * dx + c * dy + 0.0 * dyaw;
                const double t2 = 0.0 * dx + 0.0 * dy + 1.0 * dyaw;
                px = px + t0;
                py = py + t1;
                pyaw = pyaw + t2;
            }
            {
                // solution_cost += norm(node_pose(1:2) - reference_trajectory_points(:, i_step))^2          :143
                const double ddx = px - l_rx[i_step - 1], ddy = py - l_ry[i_step - 1];
                const double nrm = sqrt(ddx * ddx + ddy * ddy);
                solution_cost = solution_cost + nrm * nrm;
            }
            const int cval = (int)lane_u(row, child_position);
            if (cval != 1) {  // is_expanded                                                              :145-150
                node_id = cval;
                continue;
            }
            ++n_expansions;  // :152
            node_parent = node_id;
            // shapes = transform(1:2,1:2) * area + start_pose(1:2)                                        :159-166
            if (lane < ncols) {
                const size_t ai = (size_t)m * 3 * PDMPC_VMAX + lane;
                const size_t bi = ai + (size_t)((i_step == Hp) ? 2 : 1) * PDMPC_VMAX;
                d2 a, b;
                if (C.areas_in_lds) {
                    a = C.l_area[ai];
                    b = C.l_area[bi];
                } else {
                    a = C.g_area[ai];
                    b = C.g_area[bi];
                }
                d2 sa, sb;
                sa.x = (c * a.x + (-s) * a.y) + sx0;
                sa.y = (s * a.x + c * a.y) + sy0;
                sb.x = (c * b.x + (-s) * b.y) + sx0;
                sb.y = (s * b.x + c * b.y) + sy0;
                C.sh[lane] = sa;
                C.sh[PDMPC_VMAX + lane] = sb;
            }
            wave_sync();
            {
                // are_constraints_satisfied(iter, iVeh, shapes, shapes_for_boundary_check, i_step, ...)      :170-179
                const int so = uni_i(C.l_soff[i_step - 1]);
                const int M_k = uni_i(C.l_soff[i_step]) - so;
                bool hit;
                if (lane == 0) C.tally[0] += 1;
                if (A.checker == PDMPC_CHECK_INTERX) {
                    const int ho = uni_i(C.l_hoff[i_step - 1]);
                    const int Hk = uni_i(C.l_hoff[i_step]) - ho;
                    if (lane == 0) C.tally[1] += (unsigned long long)(ncols - 1) * (unsigned long long)((M_k > 1 ? M_k - 1 : 0) + (Hk > 1 ? Hk - 1 : 0) + (C.ll_len > 1 ? C.ll_len - 1 : 0));
                    hit = interx_check(C.sh, ncols, C.l_soup, so, M_k, ho, Hk, C.ll_base, C.ll_len, lane);
                } else {
                    hit = sat_soup_wave(C.sh, ncols, C.l_soup + so, M_k, lane);
                    if (!hit) hit = sat_boundary_wave(C.sh + PDMPC_VMAX, ncols, C.l_soup + C.ll_base, C.ll_len, lane);
                }
                wave_sync();
                is_valid = !hit;
            }
            if (!is_valid) {
                if (lane == 0) T.put(node_parent * PDMPC_SB_ROW + child_position, 0u);  // remove edge     :183
                T.sync();
                break;
            }
            ++n_nodes;  // add node: its whole row, then the parent's entry                                 :186-193
            {
                const int cc = (i_step != Hp) ? successor_count(l_mask + ((size_t)i_step * n + (goal_trim - 1)) * nw, nw) : 0;
                if (lane < PDMPC_SB_ROW)
                    T.put(n_nodes * PDMPC_SB_ROW + lane, lane < PDMPC_SB_FANOUT ? (lane < cc ? 1u : 0u) : (lane == PDMPC_SB_PARENT ? (uint32_t)node_parent : (uint32_t)goal_trim));
                if (lane == 0) T.put(node_parent * PDMPC_SB_ROW + child_position, (uint32_t)n_nodes);
            }
            T.sync();
            node_id = n_nodes;
        }
        if (is_valid) {  // valid_nodes_at_hp.push(node_id, solution_cost); only the queue's top is ever read         :199-203
            if (!have_best || solution_cost < best_cost) {
                have_best = true;
                best_cost = solution_cost;
                best_node = node_id;
            }
            if (lane == 0) T.put(node_parent * PDMPC_SB_ROW + child_position, 0u);  // avoid double exploration
            T.sync();
        }
    }

    // ---- results                                                                                       :207-248
    if (lane == 0) {
        O->n_expanded = n_expansions;
        O->n_popped = n_traversals;
        O->n_hp = Hp;
    }
    if (have_best) {
        {
            int nd = best_node;  // (every lane walks the same rows: uniform vector loads)
            for (int i = Hp; i >= 0; --i) {
                if (lane == 0) l_path[i] = (uint32_t)nd;
                nd = (int)T.get(nd * PDMPC_SB_ROW + PDMPC_SB_PARENT);
            }
        }
        wave_sync();
        // poses along the path, recomputed like the reference does (:228-239), then the swept areas with the descent's
        // arithmetic (the reference kept them from the descent that created each node: same inputs, same bits)
        double px = root_x, py = root_y, pyaw = root_yaw;
        int prev_trim = 0;
        for (int i = 0; i <= Hp; ++i) {
            const int nd = (int)l_path[i];
            const int nd_trim = (int)T.get(nd * PDMPC_SB_ROW + PDMPC_SB_TRIM);
            if (i >= 1) {
                const int m = (int)l_mi[(prev_trim - 1) * n + (nd_trim - 1)];
                const double dx = l_pose[m].dx, dy = l_pose[m].dy, dyaw = l_pose[m].dyaw;
                const int ncols = l_pose[m].n_cols;
                double s, c;
                pdmpc_sincos(pyaw, &s, &c);
                if (lane < ncols) {
                    const d2 a = C.g_area[(size_t)m * 3 * PDMPC_VMAX + lane];
                    O->shapes[i - 1][0][lane] = (c * a.x + (-s) * a.y) + px;
                    O->shapes[i - 1][1][lane] = (s * a.x + c * a.y) + py;
                }
                if (lane == 0) O->shape_cols[i - 1] = ncols;
                const double t0 = c * dx + (-s) * dy + 0.0 * dyaw;
                const double u1 = s * dx + c * dy + 0.0 * dyaw;
                const double u2 = 0.0 * dx + 0.0 * dy + 1.0 * dyaw;
                px = px + t0;
                py = py + u1;
                pyaw = pyaw + u2;
            }
            prev_trim = nd_trim;
            if (lane == 0) {
                O->tree_path[i] = nd;
                double* row = O->path_nodes[i];  // NodeInfo order; g/h stay -1 except g of the chosen node (:223-225, 244)
                row[0] = px;
                row[1] = py;
                row[2] = pyaw;
                row[3] = (double)nd_trim;
                row[4] = (nd == best_node) ? best_cost : -1.0;
                row[5] = -1.0;
                row[6] = (double)(i + 1);
                row[7] = 1.0;
                if (i >= 1) {
                    O->y_predicted[i - 1][0] = px;
                    O->y_predicted[i - 1][1] = py;
                    O->y_predicted[i - 1][2] = pyaw;
                    O->predicted_trims[i - 1] = (int32_t)nd_trim;
                }
            }
        }
        if (lane == 0) O->status = PDMPC_OK;
    } else {
        if (lane == 0) O->status = PDMPC_EXHAUSTED;  // :212-215
        if (V->fb_off[0] >= 0) {
            // the caller-supplied fallback areas (PrioritizedController.m:568-616, 678-718): in every member's record, so that member 0's
            // is the slot's record as the other sampled kernels write it if no member is OK
            for (int idx = lane; idx < Hp * PDMPC_VMAX; idx += PDMPC_WAVE) {
                const int k = idx / PDMPC_VMAX;
                const int v = idx - k * PDMPC_VMAX;
                const int a = V->fb_off[k], b = V->fb_off[k + 1];
                const int cols = (b - a < PDMPC_VMAX) ? (b - a) : PDMPC_VMAX;
                if (v == 0) O->shape_cols[k] = cols;
                if (v < cols) {
                    O->shapes[k][0][v] = A.points[2 * (size_t)(a + v)];
                    O->shapes[k][1][v] = A.points[2 * (size_t)(a + v) + 1];
                }
            }
        }
    }
    if (lane == 0) {
        atomicAdd(A.work_count + 0, C.tally[0]);  // (the checks of all members)
        atomicAdd(A.work_count + 1, C.tally[1]);
    }
    return {have_best ? PDMPC_OK : PDMPC_EXHAUSTED, n_expansions, n_nodes, have_best ? best_cost : inf};
}

template <bool IN_LDS>
__device__ __forceinline__ void sampled_ensemble_body(const SampledEnsembleArgs& G, LDS_AS unsigned char* lsm) {
    const SampledBudgetArgs& A = G.s;
    const int lane = threadIdx.x;
    const int E = G.n_members;
    const int b_slot = (int)blockIdx.x / E;
    const int e = (int)blockIdx.x - b_slot * E;
    const int slot = A.first + (A.reverse_dispatch ? A.n_searches - 1 - b_slot : b_slot);
    const size_t base = (size_t)slot * (size_t)E;
    pdmpc_vehicle_out* const mine = G.member_out + base + e;

    const MemberResult R = member_search<IN_LDS>(A, lsm, slot, PDMPC_SAMPLED_MEMBER_SEED(A.veh[slot].seed, e), mine,
                                                 IN_LDS ? nullptr : A.tree + (base + e) * (size_t)A.node_cap * PDMPC_SB_ROW);

    // ---- arrive: the entry and the tree size behind the record, everything drained, then the ticket
    if (lane == 0) {
        EnsembleEntry en;
        en.status = R.status;
        en.n_expanded = R.n_expanded;
        en.cost = R.cost;
        G.entries[base + e] = en;
        G.member_nodes[base + e] = R.n_nodes;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    uint32_t ticket = 0;
    if (lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(G.tickets + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ticket = uni_u(ticket);
    if (ticket != (uint32_t)(E - 1)) return;  // (not the last: finished, without waiting for anybody)

    // ---- the member that arrived last acts for the slot
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    int st = PDMPC_EXHAUSTED;
    double cost = 0.0;
    if (lane < E) {  // (lane-dependent index: vector loads)
        const EnsembleEntry* en = G.entries + base + lane;
        st = en->status;
        cost = en->cost;
    }
    const unsigned long long timed = __ballot(lane < E && st == PDMPC_ERR_HIP);
    unsigned long long ok = __ballot(lane < E && st == PDMPC_OK);
    int chosen = 0;
    if (timed != 0ull) {
        chosen = uni_i(__builtin_ctzll(timed));
    } else if (ok != 0ull) {
        chosen = uni_i(__builtin_ctzll(ok));
        double best = lane_d(cost, chosen);
        for (ok &= ok - 1; ok != 0ull; ok &= ok - 1) {  // ascending members, <: the lowest index wins a tie
            const int q = uni_i(__builtin_ctzll(ok));
            const double cq = lane_d(cost, q);
            if (cq < best) {
                best = cq;
                chosen = q;
            }
        }
    }
    {
        const double* src = (const double*)(G.member_out + base + chosen);
        double* dst = (double*)(A.out + slot);
        const int nd = (int)(sizeof(pdmpc_vehicle_out) / 8);
        for (int i = lane; i < nd; i += PDMPC_WAVE) dst[i] = src[i];
        if (lane == 0) {
            A.tree_size[slot] = __hip_atomic_load(G.member_nodes + base + chosen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            G.chosen[slot] = chosen;
        }
    }
    // publish like the other sampled kernels: successors of this launch, or of a later launch of the same step, wait on the flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    if (lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(A.done_flag + slot, A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_sampled_ensemble_kernel(const SampledEnsembleArgs G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sampled_ensemble_body<true>(G, (LDS_AS unsigned char*)smem);
}

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_sampled_ensemble_kernel_hbm(const SampledEnsembleArgs G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sampled_ensemble_body<false>(G, (LDS_AS unsigned char*)smem);
}

extern "C" int pdmpc_launch_sampled_ensemble(const SampledEnsembleArgs* args, int count, void* stream) {
    if (count <= 0) return 0;
    if (args->n_members < 2 || args->n_members > PDMPC_SAMPLED_ENSEMBLE_MAX) return (int)hipErrorInvalidValue;
    const bool in_lds = args->s.tree == nullptr;
    const void* fn = in_lds ? (const void*)pdmpc_sampled_ensemble_kernel : (const void*)pdmpc_sampled_ensemble_kernel_hbm;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)args->s.lds.total);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)count * (unsigned)args->n_members);
    if (in_lds)
        hipLaunchKernelGGL(pdmpc_sampled_ensemble_kernel, grid, dim3(PDMPC_WAVE), args->s.lds.total, (hipStream_t)stream, *args);
    else
        hipLaunchKernelGGL(pdmpc_sampled_ensemble_kernel_hbm, grid, dim3(PDMPC_WAVE), args->s.lds.total, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
