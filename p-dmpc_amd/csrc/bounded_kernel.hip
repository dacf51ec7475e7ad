// bounded_kernel.hip — the lanelet bounding of the reachable sets (bound_reachable_sets.m, HighLevelController.m:241-246) and the
// reachable-set coupler on the bounded step-Hp sets (ReachableSetCoupler.m:5-56), f64 throughout.  DESIGN.md §3.17.
//
//   bound   one wavefront per (vehicle, step): K (the trim's local hull moved to the pose) and the vehicle's normalized lanelet polygon L
//           in LDS, lanes over L's edges (strict Cyrus–Beck against K, pdmpc_clip_edge_t), then lane 0 builds the chains, links them
//           along ∂K and writes the kept region into the set's slot (pdmpc_bound_region) — the host twin (reachable_sets.cpp) runs the
//           same header functions, so the sets are bit-identical.  A set that does not fit its slot is flagged, never written past it.
//   box     one lane per pair i < j on the step-Hp sets' boxes (boxes that only touch are not coupled); a failing pair is written as 0,
//           a passing one appended to the pair list (a counter: the list's order is the dispatch order, which no result depends on)
//   pairs   PDMPC_BOUND_PAIR_BLOCKS wavefronts take the listed pairs grid-stride, one pair per wavefront at a time: lanes over the
//           edges of both sets (pdmpc_edge_overlap_term), and lane 0 sums them in edge order — the host twin's additions.
// Every output entry is written by exactly one lane, and a pair's area does not depend on where it landed in the list.
//
// The grouped coupler (pdmpc_bounded_set_coupling_grouped) runs box and pairs over consecutive groups of the bounded
// vehicles: the box pass enumerates (row i, columns of i's own group) only and appends to the same list, and the pairs pass writes a
// listed pair into its group's own n_g x n_g block.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_geometry.h"
#include "pair_groups.hpp"
#include "pdmpc_device.h"

#define BOUND_WAVE 64

extern "C" __global__ __launch_bounds__(BOUND_WAVE) void pdmpc_bound_sets_kernel(const BoundArgs A) {
    __shared__ double kx[PDMPC_REACH_MAX_COLS], ky[PDMPC_REACH_MAX_COLS];
    __shared__ double lx[PDMPC_BOUND_LANELET_MAX], ly[PDMPC_BOUND_LANELET_MAX], tmn[PDMPC_BOUND_LANELET_MAX], tmx[PDMPC_BOUND_LANELET_MAX];
    __shared__ int ci[6 * PDMPC_BOUND_LANELET_MAX];
    __shared__ double cd[2 * PDMPC_BOUND_LANELET_MAX];
    const int set = (int)blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int n = A.n, S = A.S, Hp = A.Hp;
    const int v = set / S, q = set - v * S;
    const int p = A.trim[v] * Hp + (A.all_steps ? q : Hp - 1);
    const int a = A.local_off[p], m = A.local_off[p + 1] - a;
    const double x0 = A.in[v], y0 = A.in[n + v], c = A.in[2 * n + v], s = A.in[3 * n + v];
    for (int r = lane; r < m; r += BOUND_WAVE) pdmpc_move_point(c, s, x0, y0, A.local_x[a + r], A.local_y[a + r], &kx[r], &ky[r]);
    const int la = A.lan_off[v], nl = A.lan_off[v + 1] - la;
    for (int r = lane; r < nl; r += BOUND_WAVE) {
        lx[r] = A.lan_x[la + r];
        ly[r] = A.lan_y[la + r];
    }
    __syncthreads();
    if (nl >= 3 && m >= 3)
        for (int e = lane; e < nl; e += BOUND_WAVE) {
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
    double* ox = A.set_x + (size_t)set * PDMPC_BOUND_SLOT;
    double* oy = A.set_y + (size_t)set * PDMPC_BOUND_SLOT;
    int cnt = 0;
    unsigned fl = 0u;
    const int over = pdmpc_bound_region(kx, ky, m, lx, ly, nl, tmn, tmx, &C, ox, oy, PDMPC_BOUND_SLOT, &cnt, &fl);
    A.set_n[set] = cnt;
    A.set_flags[set] = (uint8_t)(fl | (over ? PDMPC_BOUND_OVERFLOW : 0u));
    if (q == S - 1) {
        double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
        const int lim = over ? 0 : cnt;
        for (int r = 0; r < lim; ++r) {
            const double px = ox[r], py = oy[r];
            if (r == 0 || px < b0) b0 = px;
            if (r == 0 || px > b1) b1 = px;
            if (r == 0 || py < b2) b2 = py;
            if (r == 0 || py > b3) b3 = py;
        }
        A.box[4 * v + 0] = b0;
        A.box[4 * v + 1] = b1;
        A.box[4 * v + 2] = b2;
        A.box[4 * v + 3] = b3;
    }
}

namespace {
template <bool GROUPED>
__device__ inline void bounded_box(const BoundArgs& A) {
    const int n = A.n;
    const int i = (int)blockIdx.y;
    const RowOut o = row_out<GROUPED>(A.group, n, i);
    const int j = o.first + (int)blockIdx.x * BOUND_WAVE + (int)threadIdx.x;
    if (j >= o.end || j < i) return;
    if (j == i) {
        A.adjacency[o.at(i, i)] = 0;
        A.area[o.at(i, i)] = 0.0;
        return;
    }
    if (pdmpc_boxes_overlap(A.box + 4 * i, A.box + 4 * j)) {
        const int slot = atomicAdd(A.n_pairs, 1);
        A.pairs[slot] = i * n + j;
    } else {
        A.adjacency[o.at(i, j)] = 0;
        A.adjacency[o.at(j, i)] = 0;
        A.area[o.at(i, j)] = 0.0;
        A.area[o.at(j, i)] = 0.0;
    }
}

template <bool GROUPED>
__device__ inline void bounded_pairs(const BoundArgs& A) {
    __shared__ double sax[PDMPC_BOUND_SLOT], say[PDMPC_BOUND_SLOT], sbx[PDMPC_BOUND_SLOT], sby[PDMPC_BOUND_SLOT];
    __shared__ double scr[2 * PDMPC_BOUND_SLOT];
    const int n = A.n, S = A.S;
    const int lane = (int)threadIdx.x;
    const int total = *A.n_pairs;
    for (int pr = (int)blockIdx.x; pr < total; pr += (int)gridDim.x) {
        const int code = A.pairs[pr];
        const int i = code / n, j = code - i * n;
        const RowOut o = row_out<GROUPED>(A.group, n, i);
        const size_t si = (size_t)i * S + S - 1, sj = (size_t)j * S + S - 1;
        const double* hix = A.set_x + si * PDMPC_BOUND_SLOT;
        const double* hiy = A.set_y + si * PDMPC_BOUND_SLOT;
        const double* hjx = A.set_x + sj * PDMPC_BOUND_SLOT;
        const double* hjy = A.set_y + sj * PDMPC_BOUND_SLOT;
        int ma = A.set_n[si], mb = A.set_n[sj];
        ma = ma < PDMPC_BOUND_SLOT ? ma : PDMPC_BOUND_SLOT;  // (the host couples only when no set overflowed; never read past a slot)
        mb = mb < PDMPC_BOUND_SLOT ? mb : PDMPC_BOUND_SLOT;
        // (closed sets: the repeated first vertex is dropped, as the host twin does)
        if (ma > 1 && hix[0] == hix[ma - 1] && hiy[0] == hiy[ma - 1]) --ma;
        if (mb > 1 && hjx[0] == hjx[mb - 1] && hjy[0] == hjy[mb - 1]) --mb;
        const double ox = hix[0], oy = hiy[0];
        for (int r = lane; r < ma; r += BOUND_WAVE) {
            sax[r] = hix[r] - ox;
            say[r] = hiy[r] - oy;
        }
        for (int r = lane; r < mb; r += BOUND_WAVE) {
            sbx[r] = hjx[r] - ox;
            sby[r] = hjy[r] - oy;
        }
        __syncthreads();
        for (int e = lane; e < ma; e += BOUND_WAVE) scr[e] = pdmpc_edge_overlap_term(sax, say, ma, e, sbx, sby, mb, 0);
        for (int e = lane; e < mb; e += BOUND_WAVE) scr[ma + e] = pdmpc_edge_overlap_term(sbx, sby, mb, e, sax, say, ma, 1);
        __syncthreads();
        if (lane == 0) {
            double sum = 0.0;
            for (int e = 0; e < ma + mb; ++e) sum = sum + scr[e];
            const double ar = -0.5 * sum;
            const uint8_t cpl = ar > PDMPC_COUPLING_AREA_THRESHOLD ? 1 : 0;
            A.area[o.at(i, j)] = ar;
            A.area[o.at(j, i)] = ar;
            A.adjacency[o.at(i, j)] = cpl;
            A.adjacency[o.at(j, i)] = cpl;
        }
        __syncthreads();
    }
}
}  // namespace

extern "C" __global__ __launch_bounds__(BOUND_WAVE) void pdmpc_bounded_box_kernel(const BoundArgs A) { bounded_box<false>(A); }
extern "C" __global__ __launch_bounds__(BOUND_WAVE) void pdmpc_bounded_pairs_kernel(const BoundArgs A) { bounded_pairs<false>(A); }
extern "C" __global__ __launch_bounds__(BOUND_WAVE) void pdmpc_bounded_box_grouped_kernel(const BoundArgs A) { bounded_box<true>(A); }
extern "C" __global__ __launch_bounds__(BOUND_WAVE) void pdmpc_bounded_pairs_grouped_kernel(const BoundArgs A) { bounded_pairs<true>(A); }

extern "C" int pdmpc_launch_bound_sets(const BoundArgs* args, void* stream) {
    const int sets = args->n * args->S;
    if (sets <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_bound_sets_kernel, dim3((uint32_t)sets), dim3(BOUND_WAVE), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_bounded_coupling(const BoundArgs* args, void* stream) {
    const int n = args->n;
    if (n <= 0) return 0;
    const uint32_t col_blocks = (uint32_t)((n + BOUND_WAVE - 1) / BOUND_WAVE);
    hipLaunchKernelGGL(pdmpc_bounded_box_kernel, dim3(col_blocks, (uint32_t)n), dim3(BOUND_WAVE), 0, (hipStream_t)stream, *args);
    if (n >= 2) {
        const long long max_pairs = (long long)n * (n - 1) / 2;
        const uint32_t blocks = (uint32_t)(max_pairs < PDMPC_BOUND_PAIR_BLOCKS ? max_pairs : PDMPC_BOUND_PAIR_BLOCKS);
        hipLaunchKernelGGL(pdmpc_bounded_pairs_kernel, dim3(blocks), dim3(BOUND_WAVE), 0, (hipStream_t)stream, *args);
    }
    return (int)hipGetLastError();
}

// the same two passes for consecutive groups (args->n vehicles in all): the box grid as wide as the largest group
extern "C" int pdmpc_launch_bounded_coupling_grouped(const BoundArgs* args, void* stream) {
    const int n = args->n, mg = args->max_group;
    if (n <= 0 || mg <= 0) return 0;
    const uint32_t col_blocks = (uint32_t)((mg + BOUND_WAVE - 1) / BOUND_WAVE);
    hipLaunchKernelGGL(pdmpc_bounded_box_grouped_kernel, dim3(col_blocks, (uint32_t)n), dim3(BOUND_WAVE), 0, (hipStream_t)stream, *args);
    if (mg >= 2) {
        const long long max_pairs = (long long)n * (mg - 1) / 2;  // (an upper bound of the pairs inside the groups)
        const uint32_t blocks = (uint32_t)(max_pairs < PDMPC_BOUND_PAIR_BLOCKS ? (max_pairs < 1 ? 1 : max_pairs) : PDMPC_BOUND_PAIR_BLOCKS);
        hipLaunchKernelGGL(pdmpc_bounded_pairs_grouped_kernel, dim3(blocks), dim3(BOUND_WAVE), 0, (hipStream_t)stream, *args);
    }
    return (int)hipGetLastError();
}
