// fca_kernel.hip — future collision assessment on the device (FcaPrioritizer.m:11-92), f64 throughout.  DESIGN.md §3.19.
//
//   pass 1  one lane per (vehicle, step): the footprint at the reference point, rotated with the host's libm cos / sin (multiplies and
//           adds only, pdmpc_fca_footprint), written to the handle's buffer; lanes 0 .. n - 1 also clear the counts
//   pass 2  one lane per work item, grid-stride over the flat item index:
//             [0, n_pairs Hp)                         (pair p, step k): footprint a against footprint b; a hit counts for a and for b
//             [.., + (n - 1) Hp n_static)             (vehicle v < n - 1, step k, static obstacle o)
//             [.., + (n - 1) Hp n_rows)               (vehicle v < n - 1, step k, dynamic row r): polygon r Hp + k of the rows
//           each by pdmpc_sat_intersect (include/pdmpc_geometry.h, the arithmetic of sat_pair_lane and of the host twin); a hit adds
//           1 to the counts with an integer atomic, so the counts do not depend on the order of the lanes.
// Both polygons of a test are read from global memory where they lie (no private arrays: no scratch).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pdmpc_geometry.h"
#include "pdmpc_device.h"

extern "C" __global__ __launch_bounds__(PDMPC_FCA_BLOCK) void pdmpc_fca_footprint_kernel(const FcaArgs A) {
    const int i = (int)(blockIdx.x * PDMPC_FCA_BLOCK + threadIdx.x);
    const int m = A.n * A.Hp;
    if (i < A.n) A.counts[i] = 0;
    if (i >= m) return;
    double* f = A.fp + (size_t)8 * i;
    pdmpc_fca_footprint(A.in[2 * m + i], A.in[3 * m + i], A.in[i], A.in[m + i], A.length, A.width, A.offset, f, f + 4);
}

extern "C" __global__ __launch_bounds__(PDMPC_FCA_BLOCK) void pdmpc_fca_items_kernel(const FcaArgs A) {
    const int Hp = A.Hp;
    const int64_t stride = (int64_t)gridDim.x * PDMPC_FCA_BLOCK;
    for (int64_t t = (int64_t)blockIdx.x * PDMPC_FCA_BLOCK + threadIdx.x; t < A.n_items; t += stride) {
        if (t < A.n_pair_items) {
            const int p = (int)(t / Hp), k = (int)(t - (int64_t)p * Hp);
            const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];
            const double* fa = A.fp + (size_t)8 * ((size_t)a * Hp + k);
            const double* fb = A.fp + (size_t)8 * ((size_t)b * Hp + k);
            if (pdmpc_sat_intersect(fa, fa + 4, 4, fb, fb + 4, 4)) {
                atomicAdd(A.counts + a, 1);
                atomicAdd(A.counts + b, 1);
            }
            continue;
        }
        const bool is_static = t < A.n_pair_items + A.n_static_items;
        const int64_t u = is_static ? t - A.n_pair_items : t - A.n_pair_items - A.n_static_items;
        const int per = is_static ? A.n_static : A.n_rows;  // polygons per (vehicle, step)
        const int64_t vk = u / per;
        const int o = (int)(u - vk * per);
        const int v = (int)(vk / Hp), k = (int)(vk - (int64_t)v * Hp);
        const double* f = A.fp + (size_t)8 * ((size_t)v * Hp + k);
        const int q = is_static ? o : o * Hp + k;
        const int32_t* off = is_static ? A.static_off : A.dyn_off;
        const int a0 = off[q], m = off[q + 1] - a0;
        const double* px = (is_static ? A.static_x : A.dyn_x) + a0;
        const double* py = (is_static ? A.static_y : A.dyn_y) + a0;
        if (pdmpc_sat_intersect(f, f + 4, 4, px, py, m)) atomicAdd(A.counts + v, 1);
    }
}

extern "C" int pdmpc_launch_fca(const FcaArgs* args, void* stream) {
    const int m = args->n * args->Hp;
    if (m <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_fca_footprint_kernel, dim3((uint32_t)((m + PDMPC_FCA_BLOCK - 1) / PDMPC_FCA_BLOCK)), dim3(PDMPC_FCA_BLOCK), 0, (hipStream_t)stream,
                       *args);
    if (args->n_items > 0) {
        const int64_t blocks = std::min<int64_t>((args->n_items + PDMPC_FCA_BLOCK - 1) / PDMPC_FCA_BLOCK, PDMPC_FCA_MAX_BLOCKS);
        hipLaunchKernelGGL(pdmpc_fca_items_kernel, dim3((uint32_t)blocks), dim3(PDMPC_FCA_BLOCK), 0, (hipStream_t)stream, *args);
    }
    return (int)hipGetLastError();
}
