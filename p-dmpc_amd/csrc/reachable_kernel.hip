// reachable_kernel.hip — the reachable-set coupler on the device (ReachableSetCoupler.couple,
// hlc/controller/common/couple/ReachableSetCoupler.m:5-56), f64 throughout.  DESIGN.md §3.17.
//
//   pass 1  one lane per vehicle: its trim's local step-Hp hull moved to (x, y, yaw) with the host's libm cos / sin (multiplies and
//           adds only), and the hull's bounding box; the vehicle's diagonal entries are written as 0
//   pass 2  a workgroup of one wavefront per (row i, 64 columns j): one lane per pair i < j runs the box test (boxes that only touch are
//           not coupled) and writes 0 for a pair that fails it; the pairs that pass are taken from the ballot one after the other,
//           each by the whole wavefront: hull i (relative to its first vertex) and hull j in LDS, lanes over the edges of both, every
//           edge clipped against the other hull (include/pdmpc_geometry.h), and one lane sums the edge contributions in edge order —
//           the same sequence of additions as the host twin (reachable_sets.cpp) and reachability.py, so the 1e-3 decision and the
//           area bits agree with both.
// Every entry of the n x n outputs is written by exactly one lane: no clearing, no atomics, the same bits in any dispatch order.
//
// The grouped call (pdmpc_reachable_set_coupling_grouped) runs the same two passes over the concatenated vehicles of
// several groups: pass 2's workgroup serves (row i, 64 columns of i's OWN group, counted from the group's first vehicle), so a pair of
// two groups is neither box-tested nor written, and entry (i, j) goes to the group's own n_g x n_g block.  A pair's arithmetic does not
// depend on which 64 columns it was served with: every block holds the bits of the ungrouped call on that group alone.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_geometry.h"
#include "pair_groups.hpp"
#include "pdmpc_device.h"

namespace {
template <bool GROUPED>
__device__ inline void reach_pose(const ReachArgs& A) {
    const int v = (int)(blockIdx.x * PDMPC_REACH_WAVE + threadIdx.x);
    const int n = A.n;
    if (v >= n) return;
    const int t = A.trim[v];
    const int a = A.local_off[t], m = A.local_off[t + 1] - a;
    const double x0 = A.in[v], y0 = A.in[n + v], c = A.in[2 * n + v], s = A.in[3 * n + v];
    double* hx = A.hull_x + (size_t)v * A.max_cols;
    double* hy = A.hull_y + (size_t)v * A.max_cols;
    double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    for (int q = 0; q < m; ++q) {
        double px, py;
        pdmpc_move_point(c, s, x0, y0, A.local_x[a + q], A.local_y[a + q], &px, &py);
        hx[q] = px;
        hy[q] = py;
        if (q == 0 || px < b0) b0 = px;
        if (q == 0 || px > b1) b1 = px;
        if (q == 0 || py < b2) b2 = py;
        if (q == 0 || py > b3) b3 = py;
    }
    A.hull_n[v] = m;
    A.box[4 * v + 0] = b0;
    A.box[4 * v + 1] = b1;
    A.box[4 * v + 2] = b2;
    A.box[4 * v + 3] = b3;
    const RowOut o = row_out<GROUPED>(A.group, n, v);
    A.adjacency[o.at(v, v)] = 0;
    A.area[o.at(v, v)] = 0.0;
}

template <bool GROUPED>
__device__ inline void reach_pairs(const ReachArgs& A) {
    __shared__ double sax[PDMPC_REACH_MAX_COLS], say[PDMPC_REACH_MAX_COLS], sbx[PDMPC_REACH_MAX_COLS], sby[PDMPC_REACH_MAX_COLS];
    __shared__ double scr[2 * PDMPC_REACH_MAX_COLS];
    __shared__ uint8_t sok[2 * PDMPC_REACH_MAX_COLS];
    const int i = (int)blockIdx.y;
    const int lane = (int)threadIdx.x;
    const RowOut o = row_out<GROUPED>(A.group, A.n, i);
    const int j0 = o.first + (int)blockIdx.x * PDMPC_REACH_WAVE;
    if (j0 + PDMPC_REACH_WAVE - 1 <= i || j0 >= o.end) return;  // (uniform) no column of this block lies right of the diagonal
    const int j = j0 + lane;
    bool cand = false;
    if (j > i && j < o.end) {
        cand = pdmpc_boxes_overlap(A.box + 4 * i, A.box + 4 * j) != 0;
        if (!cand) {
            A.adjacency[o.at(i, j)] = 0;
            A.adjacency[o.at(j, i)] = 0;
            A.area[o.at(i, j)] = 0.0;
            A.area[o.at(j, i)] = 0.0;
        }
    }
    uint64_t pending = __ballot(cand);
    if (pending == 0) return;
    const int ma = A.hull_n[i];
    const double* hix = A.hull_x + (size_t)i * A.max_cols;
    const double* hiy = A.hull_y + (size_t)i * A.max_cols;
    const double ox = hix[0], oy = hiy[0];
    for (int q = lane; q < ma; q += PDMPC_REACH_WAVE) {
        sax[q] = hix[q] - ox;
        say[q] = hiy[q] - oy;
    }
    while (pending) {
        const int b = __builtin_ctzll(pending);
        pending &= pending - 1;
        const int jj = j0 + b;
        const int mb = A.hull_n[jj];
        const double* hjx = A.hull_x + (size_t)jj * A.max_cols;
        const double* hjy = A.hull_y + (size_t)jj * A.max_cols;
        for (int q = lane; q < mb; q += PDMPC_REACH_WAVE) {
            sbx[q] = hjx[q] - ox;
            sby[q] = hjy[q] - oy;
        }
        __syncthreads();
        for (int e = lane; e < ma; e += PDMPC_REACH_WAVE) {  // edges of i inside j (closed)
            const int e1 = e + 1 == ma ? 0 : e + 1;
            double cr = 0.0;
            sok[e] = (uint8_t)pdmpc_clip_edge(sax[e], say[e], sax[e1], say[e1], sbx, sby, mb, 0, &cr);
            scr[e] = cr;
        }
        for (int e = lane; e < mb; e += PDMPC_REACH_WAVE) {  // edges of j strictly inside i
            const int e1 = e + 1 == mb ? 0 : e + 1;
            double cr = 0.0;
            sok[ma + e] = (uint8_t)pdmpc_clip_edge(sbx[e], sby[e], sbx[e1], sby[e1], sax, say, ma, 1, &cr);
            scr[ma + e] = cr;
        }
        __syncthreads();
        if (lane == 0) {
            double total = 0.0;
            for (int e = 0; e < ma + mb; ++e)
                if (sok[e]) total = total + scr[e];
            const double ar = -0.5 * total;
            const uint8_t c = ar > PDMPC_COUPLING_AREA_THRESHOLD ? 1 : 0;
            A.area[o.at(i, jj)] = ar;
            A.area[o.at(jj, i)] = ar;
            A.adjacency[o.at(i, jj)] = c;
            A.adjacency[o.at(jj, i)] = c;
        }
        __syncthreads();
    }
}
}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_REACH_WAVE) void pdmpc_reach_pose_kernel(const ReachArgs A) { reach_pose<false>(A); }
extern "C" __global__ __launch_bounds__(PDMPC_REACH_WAVE) void pdmpc_reach_pairs_kernel(const ReachArgs A) { reach_pairs<false>(A); }
extern "C" __global__ __launch_bounds__(PDMPC_REACH_WAVE) void pdmpc_reach_pose_grouped_kernel(const ReachArgs A) { reach_pose<true>(A); }
extern "C" __global__ __launch_bounds__(PDMPC_REACH_WAVE) void pdmpc_reach_pairs_grouped_kernel(const ReachArgs A) { reach_pairs<true>(A); }

extern "C" int pdmpc_launch_reachable_coupling(const ReachArgs* args, void* stream) {
    const int n = args->n;
    if (n <= 0) return 0;
    const uint32_t col_blocks = (uint32_t)((n + PDMPC_REACH_WAVE - 1) / PDMPC_REACH_WAVE);
    hipLaunchKernelGGL(pdmpc_reach_pose_kernel, dim3(col_blocks), dim3(PDMPC_REACH_WAVE), 0, (hipStream_t)stream, *args);
    if (n >= 2) hipLaunchKernelGGL(pdmpc_reach_pairs_kernel, dim3(col_blocks, (uint32_t)(n - 1)), dim3(PDMPC_REACH_WAVE), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}

// the same two passes for consecutive groups: as many launches as for one group, the pair grid as wide as the largest group
extern "C" int pdmpc_launch_reachable_coupling_grouped(const ReachArgs* args, void* stream) {
    const int n = args->n;
    if (n <= 0) return 0;
    const uint32_t pose_blocks = (uint32_t)((n + PDMPC_REACH_WAVE - 1) / PDMPC_REACH_WAVE);
    const uint32_t col_blocks = (uint32_t)((args->max_group + PDMPC_REACH_WAVE - 1) / PDMPC_REACH_WAVE);
    hipLaunchKernelGGL(pdmpc_reach_pose_grouped_kernel, dim3(pose_blocks), dim3(PDMPC_REACH_WAVE), 0, (hipStream_t)stream, *args);
    if (args->max_group >= 2)
        hipLaunchKernelGGL(pdmpc_reach_pairs_grouped_kernel, dim3(col_blocks, (uint32_t)(n - 1)), dim3(PDMPC_REACH_WAVE), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
