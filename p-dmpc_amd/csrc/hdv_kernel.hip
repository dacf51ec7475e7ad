// hdv_kernel.hip — human-driven vehicles on the device (HighLevelController.update_hdv_traffic_info, HighLevelController.m:394-447, with
// the semantics of DESIGN.md §3.24), f64 throughout.  One call is four launches on one stream:
//
//   closest    one wavefront per HDV: lanes over the lanelets (pdmpc_hdv_lanelet_distance, the distances in LDS), then lane 0 runs the
//              order-dependent scan (pdmpc_hdv_closest_scan) and lists the chains (pdmpc_hdv_list_chains)
//   lane       one wavefront per (HDV, chain, step): K (the trim's step hull moved to the HDV's pose) and the raw chain polygon in LDS,
//              lane 0 normalizes it, lanes clip its edges against K (pdmpc_clip_edge_t), lane 0 builds the kept region in the slot
//              (pdmpc_bound_region: the rule of bounded_kernel.hip, not a copy of it); an empty K ∩ L is a polygon of 0 vertices
//   pack       one wavefront per slot: where its polygon starts in the caller's layout is the sum of the vertex counts of the slots in
//              front of it (integers, summed across the lanes), then the lanes copy the vertices, none at or beyond the capacity
//   adjacency  one lane per (CAV, HDV) pair (pdmpc_hdv_is_behind)
// The host twin (hdv.cpp) runs the same header functions, so lists, rows, vertices, flags and adjacency are bit-identical.  Every
// output entry is written by exactly one lane.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_geometry.h"
#include "pdmpc_device.h"

namespace {
// the chains of HDV h that exist and fit: 0 for an HDV whose lists ran over (the call fails; nothing of it is computed)
__device__ inline int hdv_chains(const HdvArgs& A, int h) {
    const int nc = A.n_chains[h];
    return A.n_closest[h] > PDMPC_HDV_MAX_CHAINS || nc > PDMPC_HDV_MAX_CHAINS ? 0 : nc;
}
// the sum of v over the wavefront's 64 lanes, in every lane
__device__ inline int wave_sum(int v) {
    for (int o = PDMPC_HDV_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_closest_kernel(const HdvArgs A) {
    __shared__ double d[PDMPC_HDV_MAX_LANELETS];
    const int h = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int n = A.n_hdv, nl = A.map.n_lanelets;
    const double px = A.in[h] - A.in[4 * n + h], py = A.in[n + h] - A.in[5 * n + h];
    for (int i = lane; i < nl; i += PDMPC_HDV_WAVE) d[i] = pdmpc_hdv_lanelet_distance(&A.map, i, px, py);
    __syncthreads();
    if (lane != 0) return;
    int32_t* list = A.closest + (size_t)h * PDMPC_HDV_MAX_CHAINS;
    const int n_list = pdmpc_hdv_closest_scan(d, nl, list, PDMPC_HDV_MAX_CHAINS);
    A.n_closest[h] = n_list;
    const int kept = n_list < PDMPC_HDV_MAX_CHAINS ? n_list : PDMPC_HDV_MAX_CHAINS;
    A.n_chains[h] = pdmpc_hdv_list_chains(&A.map, list, kept, A.chain_id + (size_t)h * PDMPC_HDV_MAX_CHAINS, A.chain_succ + (size_t)h * PDMPC_HDV_MAX_CHAINS,
                                          PDMPC_HDV_MAX_CHAINS);
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_lane_kernel(const HdvArgs A) {
    __shared__ double kx[PDMPC_REACH_MAX_COLS], ky[PDMPC_REACH_MAX_COLS];
    __shared__ double rawx[PDMPC_BOUND_LANELET_MAX], rawy[PDMPC_BOUND_LANELET_MAX];
    __shared__ double lx[PDMPC_BOUND_LANELET_MAX], ly[PDMPC_BOUND_LANELET_MAX], tmn[PDMPC_BOUND_LANELET_MAX], tmx[PDMPC_BOUND_LANELET_MAX];
    __shared__ int ci[6 * PDMPC_BOUND_LANELET_MAX];
    __shared__ double cd[2 * PDMPC_BOUND_LANELET_MAX];
    __shared__ int nl_shared;
    const int slot = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int n = A.n_hdv, Hp = A.Hp;
    const int hc = slot / Hp, k = slot - hc * Hp;
    const int h = hc / PDMPC_HDV_MAX_CHAINS, c = hc - h * PDMPC_HDV_MAX_CHAINS;
    if (c >= hdv_chains(A, h)) return;  // (the whole wavefront: no barrier is left behind)
    const int id = A.chain_id[hc], succ = A.chain_succ[hc];
    const int nr = pdmpc_hdv_chain_vertices(&A.map, id, succ);  // (<= PDMPC_BOUND_LANELET_MAX: checked at the upload)
    const double dx = A.in[4 * n + h], dy = A.in[5 * n + h];
    for (int r = lane; r < nr; r += PDMPC_HDV_WAVE) pdmpc_hdv_chain_vertex(&A.map, id, succ, dx, dy, r, &rawx[r], &rawy[r]);
    const int p = A.trim[h] * Hp + k;
    const int a = A.local_off[p], m = A.local_off[p + 1] - a;  // (<= PDMPC_REACH_MAX_COLS: checked at the upload)
    const double x0 = A.in[h], y0 = A.in[n + h], cs = A.in[2 * n + h], sn = A.in[3 * n + h];
    for (int r = lane; r < m; r += PDMPC_HDV_WAVE) pdmpc_move_point(cs, sn, x0, y0, A.local_x[a + r], A.local_y[a + r], &kx[r], &ky[r]);
    __syncthreads();
    if (lane == 0) nl_shared = pdmpc_lanelet_polygon_normalize(rawx, rawy, nr, lx, ly);
    __syncthreads();
    const int nl = nl_shared;
    if (nl >= 3 && m >= 3)
        for (int e = lane; e < nl; e += PDMPC_HDV_WAVE) {
            const int e1 = e + 1 == nl ? 0 : e + 1;
            pdmpc_clip_edge_t(lx[e], ly[e], lx[e1], ly[e1], kx, ky, m, &tmn[e], &tmx[e]);
        }
    __syncthreads();
    if (lane != 0) return;
    pdmpc_bound_chains C;
    C.start = ci;
    C.end = ci + PDMPC_BOUND_LANELET_MAX;
    C.kin = ci + 2 * PDMPC_BOUND_LANELET_MAX;
    C.kout = ci + 3 * PDMPC_BOUND_LANELET_MAX;
    C.next = ci + 4 * PDMPC_BOUND_LANELET_MAX;
    C.region = ci + 5 * PDMPC_BOUND_LANELET_MAX;
    C.sin = cd;
    C.sout = cd + PDMPC_BOUND_LANELET_MAX;
    int cnt = 0;
    unsigned fl = 0u;
    const int over = pdmpc_bound_region(kx, ky, m, lx, ly, nl, tmn, tmx, &C, A.slot_x + (size_t)slot * PDMPC_BOUND_SLOT, A.slot_y + (size_t)slot * PDMPC_BOUND_SLOT, PDMPC_BOUND_SLOT, &cnt, &fl);
    const int empty = (fl & PDMPC_BOUND_RESTORED) != 0u;  // K ∩ L is empty: 0 vertices (HighLevelController.m:416-419), not K
    A.slot_n[slot] = empty ? 0 : cnt;
    A.slot_flags[slot] = (uint8_t)(fl | (over && !empty ? PDMPC_BOUND_OVERFLOW : 0u));
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_pack_kernel(const HdvArgs A) {
    const int slot = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int n = A.n_hdv, Hp = A.Hp, per_hdv = PDMPC_HDV_MAX_CHAINS * Hp;
    const int hc = slot / Hp, k = slot - hc * Hp;
    const int h = hc / PDMPC_HDV_MAX_CHAINS, c = hc - h * PDMPC_HDV_MAX_CHAINS;
    const bool mine = c < hdv_chains(A, h);
    if (!mine && slot != 0) return;
    // the rows and vertices in front of this slot; workgroup 0 also adds up all of them and the status of the call.  Every workgroup sums
    // for itself, so the pass reads S (S - 1) / 2 counts for S slots: S <= PDMPC_HDV_MAX_VEHICLES * PDMPC_HDV_MAX_CHAINS * Hp, 256 at
    // 2 HDVs and Hp 8 (32 640 reads), 16 384 at the limits (1.3e8 reads of 64 KB that stay in L2) -- a single scan workgroup
    // is the change to make before anyone calls this with hundreds of HDVs.
    const int end = slot == 0 ? n * per_hdv : slot;
    int rows = 0, before = 0, all_rows = 0, all = 0, status = 0;
    for (int g = lane; g < n; g += PDMPC_HDV_WAVE) {
        const int nc = hdv_chains(A, g);
        if (g < h) rows += nc;
        all_rows += nc;
        if (A.n_closest[g] > PDMPC_HDV_MAX_CHAINS || A.n_chains[g] > PDMPC_HDV_MAX_CHAINS) status |= PDMPC_HDV_OVER_LISTS;
    }
    for (int j = lane; j < end; j += PDMPC_HDV_WAVE) {
        const int jhc = j / Hp, jh = jhc / PDMPC_HDV_MAX_CHAINS, jc = jhc - jh * PDMPC_HDV_MAX_CHAINS;
        if (jc >= hdv_chains(A, jh)) continue;
        const int cnt = A.slot_n[j];
        if (j < slot) before += cnt;
        all += cnt;
        if (A.slot_flags[j] & PDMPC_BOUND_OVERFLOW) status |= PDMPC_HDV_OVER_SLOT;
    }
    rows = wave_sum(rows);
    before = wave_sum(before);
    if (slot == 0) {
        all_rows = wave_sum(all_rows);
        all = wave_sum(all);
        const int lists = wave_sum(status & PDMPC_HDV_OVER_LISTS ? 1 : 0), slots = wave_sum(status & PDMPC_HDV_OVER_SLOT ? 1 : 0);
        if (lane == 0) {
            A.status[0] = all_rows;
            A.status[1] = (lists ? PDMPC_HDV_OVER_LISTS : 0) | (slots ? PDMPC_HDV_OVER_SLOT : 0);
            A.set_off[all_rows * Hp] = all;
        }
    }
    if (!mine) return;
    const int row = rows + c, set = row * Hp + k;
    const int cnt = A.slot_n[slot];
    if (lane == 0) {
        A.set_off[set] = before;
        A.set_flags[set] = (uint8_t)(A.slot_flags[slot] & (PDMPC_BOUND_RESTORED | PDMPC_BOUND_MULTIPLE));
        if (k == 0) A.row_hdv[row] = h;
    }
    const int fits = cnt < PDMPC_BOUND_SLOT ? cnt : PDMPC_BOUND_SLOT;  // (an overflowed slot holds no more; the call fails)
    const double* sx = A.slot_x + (size_t)slot * PDMPC_BOUND_SLOT;
    const double* sy = A.slot_y + (size_t)slot * PDMPC_BOUND_SLOT;
    for (int r = lane; r < fits; r += PDMPC_HDV_WAVE)
        if (before + r < A.capacity) {
            A.set_x[before + r] = sx[r];
            A.set_y[before + r] = sy[r];
        }
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_adjacency_kernel(const HdvArgs A) {
    const int n = A.n_hdv, nc = A.n_cav;
    const int item = (int)blockIdx.x * PDMPC_HDV_WAVE + (int)threadIdx.x;
    if (item >= nc * n) return;
    const int v = item / n, h = item - v * n;
    int adjacent = 0;
    if (A.cav[2 * nc + v] == A.in[4 * n + h] && A.cav[3 * nc + v] == A.in[5 * n + h]) {
        const int n_list = A.n_closest[h] < PDMPC_HDV_MAX_CHAINS ? A.n_closest[h] : PDMPC_HDV_MAX_CHAINS;
        adjacent = !pdmpc_hdv_is_behind(&A.map, A.cav_lanelet[v], A.cav[v], A.cav[nc + v], A.closest + (size_t)h * PDMPC_HDV_MAX_CHAINS, n_list, A.in[h], A.in[n + h],
                                        A.in[2 * n + h], A.in[3 * n + h]);
    }
    A.adjacency[item] = (uint8_t)adjacent;
}

extern "C" int pdmpc_launch_hdv_traffic(const HdvArgs* args, void* stream) {
    const int n = args->n_hdv;
    if (n <= 0) return 0;
    const uint32_t slots = (uint32_t)n * PDMPC_HDV_MAX_CHAINS * (uint32_t)args->Hp;
    hipLaunchKernelGGL(pdmpc_hdv_closest_kernel, dim3((uint32_t)n), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    hipLaunchKernelGGL(pdmpc_hdv_lane_kernel, dim3(slots), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    hipLaunchKernelGGL(pdmpc_hdv_pack_kernel, dim3(slots), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    if (args->n_cav > 0) {
        const uint32_t blocks = (uint32_t)(((long long)args->n_cav * n + PDMPC_HDV_WAVE - 1) / PDMPC_HDV_WAVE);
        hipLaunchKernelGGL(pdmpc_hdv_adjacency_kernel, dim3(blocks), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    }
    return (int)hipGetLastError();
}
