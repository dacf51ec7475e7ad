// sampled_search.hpp — the sampled optimizer's search (MonteCarloTreeSearch.m:40-249), the one body of pdmpc_sampled_kernel, the
// pdmpc_sampled_budget kernels and the pdmpc_sampled_ensemble kernels.  Device code, included inside a kernel file's
// anonymous namespace after wave_primitives.hpp, search_state.hpp, edge_checks.hpp and mt19937_device.hpp, like edge_checks.hpp.
//
// Up to `budget` expansions of a tree that is grown by random descents from the root (the successor at every step is drawn with a
// number of mt19937ar(seed), :53,105); an edge is checked when its node is created (:170-179), a colliding edge is cut (:183), a node
// without successors is cut from its parent (:108-112); descents that reach the horizon collision-free are candidates, the cheapest
// one (cost = sum of squared distances to the reference points, :143) wins (:197).  The descents are a dependent chain by
// construction, so one wavefront runs a search: the scalar bookkeeping is executed uniformly by all lanes, the edge check -- the only
// data-parallel part -- is the wave-wide InterX / SAT code of the optimal search (edge_checks.hpp).
//
// A slot with predecessors waits for their done flags with the blocking protocol of the graph search's non-speculative path
// (search_common.hpp): a relaxed agent-scope poll with s_sleep bounded by spin_limit, one agent-scope acquire, then vector loads of
// their records' areas into the step-k soups behind the literal polygons ([literal + NaN][n_pred x VMAX NaN-padded] per step, the bulk
// kernel's layout).  On time-out the record gets PDMPC_ERR_HIP and the search returns at once.  An exhausted search leaves the
// caller's fallback areas in its record.  Floating point: the reference's expression order (3x3 transform times dpose, rows
// accumulated left to right), -ffp-contract=off, sin/cos from pdmpc_math.h: bit-identical to the oracle's restatement.
//
// What varies between the kernels is a template parameter, never a run-time switch:
//   the tree      rows of PDMPC_SB_ROW 16-bit words (sampled_budget.h), every row written whole when its node is created, the root's
//                 too: nothing is cleared.  Tree<true>: in LDS.  Tree<false>: in HBM, private to the wave; read with relaxed atomic
//                 vector loads (never through the scalar cache), every group of stores drained and followed by an agent-scope
//                 acquire before the rows are read again -- joint_kernel.hip's discipline for its node records.
//   the numbers   DrawnAhead: the whole stream of Hp * budget doubles into LDS before the predecessor wait, with the tree's region as
//                 the generator's state (the tree is set up after the wait).  TwistByTwist: the generator's 624 state words stay
//                 in LDS and the stream is produced 312 doubles at a time as n_traversals consumes it; the first twist is made
//                 before the wait.  Either way number i is double i of mt19937ar(seed), and an index beyond the stream reads its
//                 last number.
//   the limits    ReferenceLimits: 250 expansions, 288 rows, compile-time.  ArgumentLimits: the arguments' budget and node_cap.
// The search writes the record O and returns what else its caller publishes; it stores no done flag.
#pragma once

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

// ---- the tree's rows, in LDS or in HBM
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
    // the stores drained to L2, this CU's L1 dropped: no later load meets a line cached before they were written
    __device__ __forceinline__ static void sync() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        wave_sync();
    }
};

// ---- the random numbers: start() where the prologue draws, at(i) = number i of the stream (i never decreases)
struct DrawnAhead {
    lds_f64* r;
    __device__ __forceinline__ void start(uint32_t seed, int n, LDS_AS unsigned char* lsm, const LdsLayout& L, int lane) {
        r = (lds_f64*)(lsm + L.rand);
        mt19937_doubles_wave(seed, n, (lds_u32*)(lsm + L.tree16), r, lane);
    }
    __device__ __forceinline__ double at(int i, int) const { return r[i]; }
};
struct TwistByTwist {
    lds_u32* mt;
    int twist;  // the state holds doubles [312 * twist, 312 * (twist + 1)) of the stream
    __device__ __forceinline__ void start(uint32_t seed, int, LDS_AS unsigned char* lsm, const LdsLayout& L, int lane) {
        mt = (lds_u32*)(lsm + L.rand);
        mt_seed_wave(seed, mt, lane);
        mt_twist_wave(mt, lane);
        twist = 0;
    }
    __device__ __forceinline__ double at(int i, int lane) {
        while (i >= (twist + 1) * PDMPC_SB_TWIST) {
            mt_twist_wave(mt, lane);
            ++twist;
        }
        return mt_double(mt, i - twist * PDMPC_SB_TWIST);
    }
};

// ---- n_expansions_max and the tree's rows
struct ReferenceLimits {
    template <class Args>
    __device__ __forceinline__ static int budget(const Args&) { return PDMPC_SAMPLED_BUDGET_DEFAULT; }
    template <class Args>
    __device__ __forceinline__ static int node_cap(const Args&) { return PDMPC_SB_DEFAULT_ROWS; }
};
struct ArgumentLimits {
    template <class Args>
    __device__ __forceinline__ static int budget(const Args& A) { return A.budget; }
    template <class Args>
    __device__ __forceinline__ static int node_cap(const Args& A) { return A.node_cap; }
};

// what a search leaves besides its record
struct SearchResult {
    int status, n_expanded, n_nodes;
    double cost;  // of the plan if status == PDMPC_OK, +inf otherwise
};

// The search of `slot` with `seed`, its record in O, its tree in the layout's tree16 region or at hbm_tree.
template <bool IN_LDS, class Rand, class Limits, class Args>
__device__ __forceinline__ SearchResult sampled_search(const Args& A, LDS_AS unsigned char* lsm, int slot, uint32_t seed, pdmpc_vehicle_out* __restrict__ O, uint16_t* hbm_tree) {
    const int lane = threadIdx.x;
    const int Hp = A.Hp, n = A.n_trims, nw = A.n_words;
    const int budget = Limits::budget(A), node_cap = Limits::node_cap(A);
    const DevVehicle* __restrict__ V = A.veh + slot;
    const int n_random = Hp * budget;  // rand(stream, 1, Hp * n_expansions_max)                                 :53
    const double inf = __longlong_as_double(0x7ff0000000000000LL);

    // ---- LDS carve (launch_plan.hpp: layout_sampled)
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
    Tree<IN_LDS> T;
    if constexpr (IN_LDS)
        T.p = (LDS_AS uint16_t*)(lsm + A.lds.tree16);
    else
        T.p = hbm_tree;
    Rand R;

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

    // ---- prologue: tables, reference points, record defaults, random numbers, obstacle soups, predecessors
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
    R.start(seed, n_random, lsm, A.lds, lane);
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
                const double r = uni_d(R.at((n_traversals <= n_random ? n_traversals : n_random) - 1, lane));
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
            // the caller-supplied fallback areas (PrioritizedController.m:568-616, 678-718; the graph search's record, bulk_search.hpp):
            // published with the record, so that successors of this launch avoid them
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
        atomicAdd(A.work_count + 0, C.tally[0]);
        atomicAdd(A.work_count + 1, C.tally[1]);
    }
    return {have_best ? PDMPC_OK : PDMPC_EXHAUSTED, n_expansions, n_nodes, have_best ? best_cost : inf};
}

// The slot's done flag, behind everything the wave has stored: successors of this launch, or of a later launch of the same step, wait
// on it (like the optimal search's).
template <class Args>
__device__ __forceinline__ void sampled_release_slot(const Args& A, int slot) {
    const int lane = threadIdx.x;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    if (lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(A.done_flag + slot, A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One search per slot (blockIdx.x, turned round with reverse_dispatch), its record the slot's: search, tree size, done flag.  A search
// that timed out on a predecessor leaves no tree size.
template <bool IN_LDS, class Rand, class Limits, class Args>
__device__ __forceinline__ void sampled_slot_body(const Args& A, LDS_AS unsigned char* lsm, uint16_t* hbm_trees) {
    const int slot = A.first + (A.reverse_dispatch ? A.n_searches - 1 - (int)blockIdx.x : (int)blockIdx.x);
    const SearchResult S = sampled_search<IN_LDS, Rand, Limits>(A, lsm, slot, A.veh[slot].seed, A.out + slot,
                                                                IN_LDS ? nullptr : hbm_trees + (size_t)slot * (size_t)Limits::node_cap(A) * PDMPC_SB_ROW);
    if (threadIdx.x == 0 && S.status != PDMPC_ERR_HIP) A.tree_size[slot] = S.n_nodes;
    sampled_release_slot(A, slot);
}
