// joint_kernel.hip — centralized control: ONE graph search over the joint state of N vehicles (GraphSearch.do_graph_search with
// iter.amount = N, GraphSearch.m:23-107 + eval_edge_exact :111-196 + expand_node.m, separating-axis checker).
//
// One workgroup of one wavefront per joint problem; problems are independent (no waits between workgroups, no dispatch order assumed).
//   pop      the libstdc++-faithful binary heap of heap_queue.hpp (keys in LDS, spilling to the problem's far list in HBM), run by
//            the whole wavefront, as in pdmpc_heap_script_kernel: the pop chain is serial by contract
//   check    per vehicle v: its area against every polygon of its step-k soup (static, then dynamic obstacles), against the area of
//            every vehicle u < v of the same node, and its boundary-check area against its lanelet boundary (the wave-wide forms of
//            edge_checks.hpp, one lane per separating axis / boundary segment).  The reference returns at the first hit; the result is
//            a plain AND of side-effect-free tests, so the order of the tests does not matter
//   expand   one lane per child: the children are the Cartesian product of the vehicles' successor trims, vehicle 1 varying fastest
//            (expand_node.m:15-29, cartprod.m, ind2subVect.m), in chunks of 64; each lane writes its child's N records and key,
//            then the chunk is pushed in child order
// The tree: joint node i (0-based) of a problem whose first slot is o is the N records nodes[(o + v) * max_nodes + i]: vehicle v's
// x, y, yaw and trim, the node's k and parent, and its joint g and h.  Areas are recomputed from the parent, never stored.
// Floating point: -ffp-contract=off, pdmpc_sincos, norm as sqrt(dx*dx + dy*dy), expressions in the reference's order — the oracle's
// arithmetic of the single-vehicle searches, so N = 1 reproduces the single-vehicle search bit for bit.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_math.h"
#include "pdmpc_device.h"

namespace {

#include "wave_primitives.hpp"
#include "search_state.hpp"
#include "heap_queue.hpp"
#include "edge_checks.hpp"

// the j-th (0-based) set bit of a successor mask row, as a 1-based trim
__device__ __forceinline__ int joint_nth_successor(const lds_mask64* row, int nw, int j) {
    for (int w = 0; w < nw; ++w) {
        uint64_t m = row[w];
        const int c = __builtin_popcountll(m);
        if (j < c) {
            for (int q = 0; q < j; ++q) m &= m - 1;
            return w * 64 + __builtin_ctzll(m) + 1;
        }
        j -= c;
    }
    return 0;
}

// c * area(1, :) - s * area(2, :) + pX; s * area(1, :) + c * area(2, :) + pY          GraphSearch.m:158-159 (also :162-169)
__device__ __forceinline__ d2 joint_place(d2 a, double c, double s, double px, double py) {
    d2 r;
    r.x = c * a.x - s * a.y + px;
    r.y = s * a.x + c * a.y + py;
    return r;
}

}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_joint_kernel(const JointArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int p = blockIdx.x;
    const int first = A.problem_off[p];
    const int N = A.problem_off[p + 1] - first;
    const int Hp = A.Hp, n = A.n_trims, nw = A.n_words;
    const uint32_t max_nodes = A.max_nodes;

    LDS_AS unsigned char* lsm = (LDS_AS unsigned char*)smem;
    lds_mask64* l_mask = (lds_mask64*)(lsm + A.lds.mask);
    lds_i16* l_mi = (lds_i16*)(lsm + A.lds.man_index);
    lds_pose* l_pose = (lds_pose*)(lsm + A.lds.pose);
    const lds_d2* l_area = (const lds_d2*)(lsm + A.lds.area);
    const d2* g_area = (const d2*)A.man_area;
    lds_f64* l_ref = (lds_f64*)(lsm + A.lds.ref);  // [v][0: x, 1: y, 2: v_ref][k]
    lds_d2* l_shape = (lds_d2*)(lsm + A.lds.shape);  // [v][0: area, 1: boundary-check area][VMAX]
    lds_i32* l_soff = (lds_i32*)(lsm + A.lds.ints);  // [v][k]: soup offset of step k + 1 (k = Hp: end)
    lds_i32* l_llb = l_soff + PDMPC_JOINT_MAX * (PDMPC_HP_MAX + 1);
    lds_i32* l_lll = l_llb + PDMPC_JOINT_MAX;
    lds_i32* l_cols = l_lll + PDMPC_JOINT_MAX;
    lds_i32* l_path = l_cols + PDMPC_JOINT_MAX;
    lds_i32* l_succ = (lds_i32*)(lsm + A.lds.succ);  // [v][n]
    lds_d2* l_soup = (lds_d2*)(lsm + A.lds.soup);

    // ---- prologue: MPA tables, reference points, soups, record defaults
    stage16(l_mask, A.succ_mask, (Hp * n * nw * 8 + 15) / 16, lane);
    stage16(l_mi, A.man_index, (n * n * 2 + 15) / 16, lane);
    stage16(l_pose, A.man_pose, A.n_man * 2, lane);
    if (A.areas_in_lds) stage16(lsm + A.lds.area, A.man_area, A.n_man * 3 * PDMPC_VMAX, lane);
    {
        int off = 0;
        for (int v = 0; v < N; ++v) {
            const DevVehicle* V = A.veh + first + v;
            if (lane < Hp) {
                l_ref[(v * 3 + 0) * PDMPC_HP_MAX + lane] = V->ref_x[lane];
                l_ref[(v * 3 + 1) * PDMPC_HP_MAX + lane] = V->ref_y[lane];
                l_ref[(v * 3 + 2) * PDMPC_HP_MAX + lane] = V->v_ref[lane];
            }
            // one LDS copy per distinct soup of the problem (pdmpc_device.h: the rule layout_joint budgets by).  A row that is taken over
            // is read by the lanes that wrote it: LDS accesses of a wavefront complete in order
            const int su = uni_i(pdmpc_joint_soup_owner(A.veh + first, v, Hp));
            if (su >= 0) {
                if (lane <= Hp) l_soff[v * (PDMPC_HP_MAX + 1) + lane] = l_soff[su * (PDMPC_HP_MAX + 1) + lane];
            } else {
                const int a0 = uni_i(V->lit_off[0]);
                const int a1 = uni_i(V->lit_off[Hp]);
                if (lane <= Hp) l_soff[v * (PDMPC_HP_MAX + 1) + lane] = off + (V->lit_off[lane] - a0);
                stage16(l_soup + off, (const d2*)A.points + a0, a1 - a0, lane);
                off += a1 - a0;
            }
            const int bu = uni_i(pdmpc_joint_boundary_owner(A.veh + first, v));
            const int ll = uni_i(V->ll_len);
            if (bu >= 0) {
                if (lane == 0) {
                    l_llb[v] = l_llb[bu];
                    l_lll[v] = ll;
                }
            } else {
                stage16(l_soup + off, (const d2*)A.points + uni_i(V->ll_off), ll, lane);
                if (lane == 0) {
                    l_llb[v] = off;
                    l_lll[v] = ll;
                }
                off += ll;
            }
        }
    }
    for (int v = 0; v < N; ++v) {
        double* od = (double*)(A.out + first + v);
        const int nd = (int)(sizeof(pdmpc_vehicle_out) / 8);
        const int y0 = (int)(offsetof(pdmpc_vehicle_out, y_predicted) / 8);
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        for (int i = lane; i < nd; i += PDMPC_WAVE) od[i] = (i >= y0 && i < y0 + PDMPC_HP_MAX * 3) ? qnan : 0.0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();

    Search S;
    S.lkey = (lds_f64*)(lsm + A.lds.heap_key);
    S.lid = (lds_u32*)(lsm + A.lds.heap_id);
    S.gkey = A.far_key + (size_t)first * max_nodes;
    S.gid = A.far_id + (size_t)first * max_nodes;
    S.HL = A.heap_lds;
    S.heap_len = 0;
    S.lane = lane;
    S.pl = make_pop_lane(lane);
    S.ln = nullptr;
    S.gn = nullptr;
    S.NL = 0;
    S.max_nodes = max_nodes;

    NodeRec* __restrict__ T = A.nodes + (size_t)first * max_nodes;  // vehicle v, node i: T[v * max_nodes + i]

    // ---- root: every vehicle's pose and trim, k = g = h = 0; pq.push(1, 0)                            GraphSearch.m:29-46
    if (lane < N) {
        const DevVehicle* V = A.veh + first + lane;
        NodeRec r;
        r.x = V->x0;
        r.y = V->y0;
        r.yaw = V->yaw0;
        r.g = 0.0;
        r.cs = 0.0;
        r.sn = 0.0;
        r.h = 0.0;
        r.parent = 0;
        r.packed = (uint32_t)V->trim0;
        T[(size_t)lane * max_nodes] = r;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    heap_push(S, 1u, 0.0);
    uint32_t tree_size = 1;
    int n_popped = 0, n_checks = 0;
    int status = PDMPC_EXHAUSTED;
    uint32_t goal = 0;

    while (S.heap_len > 0) {
        // cur_node_id = pq.pop()                                                                        :55
        double k0;
        uint32_t i0;
        heap_load<false>(S, 0, true, k0, i0);
        const uint32_t cur = uni_u(i0);
        heap_pop(S);
        ++n_popped;
        const uint32_t c0 = cur - 1;
        const uint32_t par = uni_u(T[c0].parent);
        const int cK = (int)(uni_u(T[c0].packed) >> 10);

        // ---- eval_edge_exact                                                                           :111-196
        bool valid = true;
        if (par) {
            ++n_checks;
            // areas of every vehicle: lane = (vehicle, column)
            for (int t = lane; t < N * PDMPC_VMAX; t += PDMPC_WAVE) {
                const int v = t / PDMPC_VMAX, col = t % PDMPC_VMAX;
                const NodeRec pr = T[(size_t)v * max_nodes + (par - 1)];
                const int t1 = (int)(pr.packed & 1023u), t2 = (int)(T[(size_t)v * max_nodes + c0].packed & 1023u);
                const int m = (int)l_mi[(t1 - 1) * n + (t2 - 1)];
                const int ncols = l_pose[m].n_cols;
                if (col == 0) l_cols[v] = ncols;
                if (col < ncols) {
                    double s, c;
                    pdmpc_sincos(pr.yaw, &s, &c);  // c = cos(pYaw); s = sin(pYaw)                        :155-156
                    const size_t ai = (size_t)m * 3 * PDMPC_VMAX + col;
                    const size_t bi = ai + (size_t)((cK == Hp) ? 2 : 1) * PDMPC_VMAX;  // large offset at k == Hp (:166-174)
                    d2 a, b;
                    if (A.areas_in_lds) {
                        a = l_area[ai];
                        b = l_area[bi];
                    } else {
                        a = g_area[ai];
                        b = g_area[bi];
                    }
                    l_shape[(v * 2 + 0) * PDMPC_VMAX + col] = joint_place(a, c, s, pr.x, pr.y);
                    l_shape[(v * 2 + 1) * PDMPC_VMAX + col] = joint_place(b, c, s, pr.x, pr.y);
                }
            }
            wave_sync();
            // are_constraints_satisfied_sat.m:15-53 for every vehicle (the hdv loop :55-66 is unreachable)
            for (int v = 0; v < N && valid; ++v) {
                const lds_d2* sv = l_shape + (v * 2) * PDMPC_VMAX;
                const int cv = uni_i(l_cols[v]);
                const int so = uni_i(l_soff[v * (PDMPC_HP_MAX + 1) + cK - 1]);
                const int M = uni_i(l_soff[v * (PDMPC_HP_MAX + 1) + cK]) - so;
                bool hit = sat_soup_wave(sv, cv, l_soup + so, M, lane);
                for (int u = 0; u < v && !hit; ++u) hit = sat_pair_wave(l_shape + (u * 2) * PDMPC_VMAX, uni_i(l_cols[u]), sv, cv, lane);
                if (!hit) hit = sat_boundary_wave(sv + PDMPC_VMAX, cv, l_soup + uni_i(l_llb[v]), uni_i(l_lll[v]), lane);
                valid = !hit;
            }
            wave_sync();
        }
        if (!valid) continue;  // :75-77
        if (cK == Hp) {        // :81-90
            status = PDMPC_OK;
            goal = cur;
            break;
        }

        // ---- expand_node.m: successors of every vehicle (find(transition_matrix_single(trim_v, :, k + 1)), ascending)
        const int k_exp = cK + 1;
        uint64_t n_prod = 1;
        int cnt[PDMPC_JOINT_MAX];
#pragma unroll
        for (int v = 0; v < PDMPC_JOINT_MAX; ++v) cnt[v] = 1;
#pragma unroll
        for (int v = 0; v < PDMPC_JOINT_MAX; ++v) {
            if (v < N) {
                const int tv = (int)(uni_u(T[(size_t)v * max_nodes + c0].packed) & 1023u);
                const lds_mask64* row = l_mask + ((size_t)(k_exp - 1) * n + (tv - 1)) * nw;
                int c = 0;
                for (int w = 0; w < nw; ++w) c += __builtin_popcountll(row[w]);
                for (int j = lane; j < c; j += PDMPC_WAVE) l_succ[v * n + j] = joint_nth_successor(row, nw, j);
                cnt[v] = c;
                n_prod *= (uint64_t)c;
            }
        }
        wave_sync();
        if (n_prod == 0) continue;
        if ((uint64_t)tree_size + n_prod > (uint64_t)max_nodes) {  // the reference's tree is unbounded; the arena is not
            status = PDMPC_ARENA_OVERFLOW;
            break;
        }
        const uint32_t n_child = (uint32_t)n_prod;
        const int steps_to_go = Hp - k_exp;  // :37
        const double curG = uni_d(T[c0].g);
        for (uint32_t base = 0; base < n_child; base += PDMPC_WAVE) {
            const uint32_t t = base + (uint32_t)lane;
            double key = 0.0;
            if (t < n_child) {
                double g = curG, h = 0.0;  // :34-35
                double ex[PDMPC_JOINT_MAX], ey[PDMPC_JOINT_MAX], eyaw[PDMPC_JOINT_MAX];
                int etrim[PDMPC_JOINT_MAX];
                uint32_t rest = t;  // ind2subVect: vehicle 1 varies fastest
#pragma unroll
                for (int v = 0; v < PDMPC_JOINT_MAX; ++v) {
                    ex[v] = ey[v] = eyaw[v] = 0.0;
                    etrim[v] = 0;
                    if (v < N) {
                        const uint32_t cv = (uint32_t)cnt[v];
                        const uint32_t iv = rest % cv;
                        rest /= cv;
                        const NodeRec cr = T[(size_t)v * max_nodes + c0];
                        const int t1 = (int)(cr.packed & 1023u), t2 = l_succ[v * n + iv];
                        const int mi = (int)l_mi[(t1 - 1) * n + (t2 - 1)];
                        const double mdx = l_pose[mi].dx, mdy = l_pose[mi].dy, mdyaw = l_pose[mi].dyaw;
                        double s, c;
                        pdmpc_sincos(cr.yaw, &s, &c);                 // :50-51
                        ex[v] = c * mdx - s * mdy + cr.x;           // :53
                        ey[v] = s * mdx + c * mdy + cr.y;           // :54
                        eyaw[v] = cr.yaw + mdyaw;                     // :55
                        etrim[v] = t2;
                        const lds_f64* rx = l_ref + (v * 3 + 0) * PDMPC_HP_MAX;
                        const lds_f64* ry = l_ref + (v * 3 + 1) * PDMPC_HP_MAX;
                        const lds_f64* vr = l_ref + (v * 3 + 2) * PDMPC_HP_MAX;
                        {
                            const double ddx = ex[v] - rx[k_exp - 1], ddy = ey[v] - ry[k_exp - 1];
                            const double nrm = sqrt(ddx * ddx + ddy * ddy);
                            g = g + nrm * nrm;  // :61
                        }
                        double dmax = 0.0;  // :66
                        for (int it = 1; it <= steps_to_go; ++it) {  // :68-73
                            dmax = dmax + A.dt * vr[k_exp + it - 1];
                            const double ddx = ex[v] - rx[k_exp + it - 1], ddy = ey[v] - ry[k_exp + it - 1];
                            const double nrm = sqrt(ddx * ddx + ddy * ddy);
                            const double diff = nrm - dmax;
                            const double m0 = (diff > 0) ? diff : 0.0;
                            h = h + m0 * m0;
                        }
                    }
                }
#pragma unroll
                for (int v = 0; v < PDMPC_JOINT_MAX; ++v) {
                    if (v < N) {  // add_nodes (Tree.m:54-70): the joint g and h in every vehicle's record
                        NodeRec r;
                        r.x = ex[v];
                        r.y = ey[v];
                        r.yaw = eyaw[v];
                        r.g = g;
                        r.cs = 0.0;
                        r.sn = 0.0;
                        r.h = h;
                        r.parent = cur;
                        r.packed = (uint32_t)etrim[v] | ((uint32_t)k_exp << 10);
                        T[(size_t)v * max_nodes + tree_size + t] = r;
                    }
                }
                key = g * 1.0 + h * 1.0;  // GraphSearch.m:100-102
            }
            // pq.push(new_open_nodes, new_open_values): in child order                                  mex.cpp:67-72
            const int in_chunk = (int)((n_child - base) < (uint32_t)PDMPC_WAVE ? (n_child - base) : (uint32_t)PDMPC_WAVE);
            for (int j = 0; j < in_chunk; ++j) heap_push(S, tree_size + base + (uint32_t)j + 1u, lane_d(key, j));
        }
        tree_size += n_child;
        // the children's records are read by the next pops: drained to L2, and this CU's L1 dropped so no plain load meets a line
        // it cached before they were written
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }

    // ---- results (GraphSearch.m:57-61, 81-90)
    wave_sync();
    if (status == PDMPC_OK) {
        if (lane == 0) {
            uint32_t nd = goal;
            for (int i = Hp; i >= 0; --i) {  // fliplr(path_to_root(tree, goal))
                l_path[i] = (int32_t)nd;
                nd = T[nd - 1].parent;
            }
        }
        wave_sync();
        // lane = (vehicle, step): the node's row, its pose and trim, and the area of the edge into it
        for (int t = lane; t < N * (Hp + 1); t += PDMPC_WAVE) {
            const int v = t / (Hp + 1), i = t % (Hp + 1);
            const uint32_t nd = (uint32_t)l_path[i];
            const NodeRec r = T[(size_t)v * max_nodes + nd - 1];
            pdmpc_vehicle_out* O = A.out + first + v;
            O->tree_path[i] = (int32_t)nd;
            double* row = O->path_nodes[i];  // NodeInfo.m:5-13
            row[0] = r.x;
            row[1] = r.y;
            row[2] = r.yaw;
            row[3] = (double)(r.packed & 1023u);
            row[4] = r.g;
            row[5] = r.h;
            row[6] = (double)(r.packed >> 10);
            row[7] = 1.0;
            if (i >= 1) {
                O->y_predicted[i - 1][0] = r.x;  // return_path_to.m:14-23
                O->y_predicted[i - 1][1] = r.y;
                O->y_predicted[i - 1][2] = r.yaw;
                O->predicted_trims[i - 1] = (int32_t)(r.packed & 1023u);  // GraphSearch.m:86
                const NodeRec pr = T[(size_t)v * max_nodes + (uint32_t)l_path[i - 1] - 1];
                const int m = (int)l_mi[(int)((pr.packed & 1023u) - 1) * n + (int)((r.packed & 1023u) - 1)];
                const int ncols = l_pose[m].n_cols;
                double s, c;
                pdmpc_sincos(pr.yaw, &s, &c);
                O->shape_cols[i - 1] = ncols;  // return_path_area.m:4-7
                for (int col = 0; col < ncols; ++col) {
                    const d2 a = g_area[(size_t)m * 3 * PDMPC_VMAX + col];
                    const d2 q = joint_place(a, c, s, pr.x, pr.y);
                    O->shapes[i - 1][0][col] = q.x;
                    O->shapes[i - 1][1][col] = q.y;
                }
            }
        }
    }
    if (lane < N) {
        pdmpc_vehicle_out* O = A.out + first + lane;
        O->status = status;
        O->n_expanded = (int32_t)tree_size;  // info.n_expanded = info.tree.size()                          :58, :89
        O->n_popped = n_popped;
        O->n_hp = Hp;
        A.tree_size[first + lane] = (int32_t)tree_size;
    }
    if (lane == 0) {
        atomicAdd(A.work_count + 0, (unsigned long long)n_checks);
        atomicAdd(A.work_count + 2, (unsigned long long)n_popped);
    }
}

extern "C" int pdmpc_launch_joint(const JointArgs* args, int n_problems, void* stream) {
    if (n_problems <= 0) return 0;
    hipError_t e = hipFuncSetAttribute((const void*)pdmpc_joint_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)args->lds.total);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pdmpc_joint_kernel, dim3(n_problems), dim3(PDMPC_WAVE), args->lds.total, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
