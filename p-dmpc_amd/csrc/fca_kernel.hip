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
//
// Both passes are compiled twice from one body.  GROUPED (pdmpc_fca_collisions_grouped): the vehicles are consecutive
// groups with their own sizes, obstacles and rows.  Pass 1 takes length, width and offset from the vehicle's group.  In pass 2 the pair
// items are as above (the host has rebased the pairs to the concatenated numbering); the static range is the groups' ranges
// (n_g - 1) Hp S_g one after the other and the dynamic range their (n_g - 1) Hp R_g, each with a prefix table over the groups that an
// item is located in by binary search; inside its group's range an item decodes as above, on the group's vehicles and polygons.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pdmpc_geometry.h"
#include "pdmpc_device.h"

namespace {
template <bool GROUPED>
__device__ __forceinline__ void fca_footprints(const FcaArgs& A, const FcaGroups& G) {
    const int i = (int)(blockIdx.x * PDMPC_FCA_BLOCK + threadIdx.x);
    const int m = A.n * A.Hp;
    if (i < A.n) A.counts[i] = 0;
    if (i >= m) return;
    double* f = A.fp + (size_t)8 * i;
    double length = A.length, width = A.width, offset = A.offset;
    if constexpr (GROUPED) {
        const FcaGroup& g = G.group[G.vehicle_group[i / A.Hp]];
        length = g.length;
        width = g.width;
        offset = g.offset;
    }
    pdmpc_fca_footprint(A.in[2 * m + i], A.in[3 * m + i], A.in[i], A.in[m + i], length, width, offset, f, f + 4);
}

// the group whose range of `first` (a prefix table, first[0] = 0) holds item u < first[n_groups]: the last g with first[g] <= u
__device__ __forceinline__ int fca_group_of(const int64_t* first, int n_groups, int64_t u) {
    int lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= u)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

template <bool GROUPED>
__device__ __forceinline__ void fca_items(const FcaArgs& A, const FcaGroups& G) {
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
        int64_t u = is_static ? t - A.n_pair_items : t - A.n_pair_items - A.n_static_items;
        int per = is_static ? A.n_static : A.n_rows;  // polygons per (vehicle, step)
        int v0 = 0, q0 = 0;                           // the group's first vehicle and first polygon
        if constexpr (GROUPED) {
            const int64_t* first = is_static ? G.static_first : G.dyn_first;
            const int gi = fca_group_of(first, G.n_groups, u);
            const FcaGroup& g = G.group[gi];
            u -= first[gi];
            per = is_static ? g.n_static : g.n_rows;
            v0 = g.first;
            q0 = is_static ? g.static_polygon : g.dyn_polygon;
        }
        const int64_t vk = u / per;
        const int o = (int)(u - vk * per);
        const int vl = (int)(vk / Hp), k = (int)(vk - (int64_t)vl * Hp);
        const int v = v0 + vl;
        const double* f = A.fp + (size_t)8 * ((size_t)v * Hp + k);
        const int q = q0 + (is_static ? o : o * Hp + k);
        const int32_t* off = is_static ? A.static_off : A.dyn_off;
        const int a0 = off[q], m = off[q + 1] - a0;
        const double* px = (is_static ? A.static_x : A.dyn_x) + a0;
        const double* py = (is_static ? A.static_y : A.dyn_y) + a0;
        if (pdmpc_sat_intersect(f, f + 4, 4, px, py, m)) atomicAdd(A.counts + v, 1);
    }
}

template <class Footprints, class Items, class Args>
int launch_fca(Footprints footprints, Items items, const FcaArgs& a, const Args& args, void* stream) {
    const int m = a.n * a.Hp;
    if (m <= 0) return 0;
    hipLaunchKernelGGL(footprints, dim3((uint32_t)((m + PDMPC_FCA_BLOCK - 1) / PDMPC_FCA_BLOCK)), dim3(PDMPC_FCA_BLOCK), 0, (hipStream_t)stream, args);
    if (a.n_items > 0) {
        const int64_t blocks = std::min<int64_t>((a.n_items + PDMPC_FCA_BLOCK - 1) / PDMPC_FCA_BLOCK, PDMPC_FCA_MAX_BLOCKS);
        hipLaunchKernelGGL(items, dim3((uint32_t)blocks), dim3(PDMPC_FCA_BLOCK), 0, (hipStream_t)stream, args);
    }
    return (int)hipGetLastError();
}
}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_FCA_BLOCK) void pdmpc_fca_footprint_kernel(const FcaArgs A) { fca_footprints<false>(A, FcaGroups{}); }
extern "C" __global__ __launch_bounds__(PDMPC_FCA_BLOCK) void pdmpc_fca_items_kernel(const FcaArgs A) { fca_items<false>(A, FcaGroups{}); }
extern "C" __global__ __launch_bounds__(PDMPC_FCA_BLOCK) void pdmpc_fca_footprint_grouped_kernel(const FcaGroupedArgs B) { fca_footprints<true>(B.a, B.g); }
extern "C" __global__ __launch_bounds__(PDMPC_FCA_BLOCK) void pdmpc_fca_items_grouped_kernel(const FcaGroupedArgs B) { fca_items<true>(B.a, B.g); }

extern "C" int pdmpc_launch_fca(const FcaArgs* args, void* stream) {
    return launch_fca(pdmpc_fca_footprint_kernel, pdmpc_fca_items_kernel, *args, *args, stream);
}

extern "C" int pdmpc_launch_fca_grouped(const FcaGroupedArgs* args, void* stream) {
    return launch_fca(pdmpc_fca_footprint_grouped_kernel, pdmpc_fca_items_grouped_kernel, args->a, *args, stream);
}
