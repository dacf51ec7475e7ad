// priority_kernel.hip — the unique prioritizations of a coupling graph on the device (Prioritizer.unique_priorities,
// hlc/controller/prioritized/priority/Prioritizer.m:97-140): of the 2^E orientations of the graph's E edges, the acyclic ones in
// ascending order of their mask m = i_permutation - 1, and for each the priorities of its lexicographically smallest topological order.
//
// One lane per mask.  The flip set of lane m is m itself (pdmpc_device.h: edge e is bit E - 1 - e), so the edges that point into
// vertex v are (in_base[v] & ~m) | (out_base[v] & m): two uniform words per vertex, read from the kernel arguments.  A lane keeps
// only R, the set of edges not yet removed, and peels: every sweep over the vertices that have edges removes all edges of a vertex
// that no remaining edge points into.  R reaching 0 means acyclic; a sweep that leaves R as it was means a cycle.
//
// The acyclic masks are compacted in mask order, deterministically, in two passes over fixed tiles of PDMPC_PRIO_TILE masks:
//   count  per tile the number of acyclic masks (ballot + popcount per wavefront, summed over the workgroup)
//   scan   exclusive int64 prefix sum of the tile counts (one workgroup); entry n_tiles is the total K
//   write  the same test again; a mask's position = tile offset + masks of the earlier rounds + earlier wavefronts (LDS) + earlier
//          lanes (mbcnt over the ballot)
//   order  one lane per written mask: priorities(topological_order) = 1:n, the order that takes the smallest-index vertex with no
//          remaining incoming edge first (toposort(..., 'Order', 'stable'))
// Integer work only: no f64, no scratch (make resources).
//
// Every pass but the scan is compiled twice from one body.  GROUPED (pdmpc_unique_priorities_grouped): several graphs
// in one call.  The host stages one PriorityArgs per graph and tile_first, the prefix of the graphs' tile counts: a tile belongs to
// exactly one graph (a graph's last tile may be partly empty, a graph without edges is one tile that holds mask 0).  A workgroup finds
// its graph by a binary search over tile_first that is the same for all its lanes and reads the graph through uniform loads; the peel
// is the ungrouped one.  The scan runs over all tiles, so the graphs' lists stand one after the other and graph g's masks start at
// tile_off[tile_first[g]] (offsets pass: mask_first).  In the order pass a lane finds the graph of its mask by a binary search over
// mask_first, and its row at row_first[g] + (k - mask_first[g]) * n_g.  The ungrouped instantiations read the graph from the kernel
// arguments as before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pdmpc_device.h"

namespace {

// what a pass reads its graph(s) from: the graph itself in the kernel arguments, or the staged tables of a grouped call
struct GroupTables {
    const PriorityArgs* __restrict__ graph;
    const int64_t* __restrict__ first;  // tile_first (count, write) or mask_first (order)
    const int64_t* __restrict__ row_first;
    int32_t n_groups;
};
template <bool GROUPED>
using PrioIn = std::conditional_t<GROUPED, GroupTables, PriorityArgs>;

// the group g whose range first[g] .. first[g + 1] - 1 holds x (first[0] = 0 <= x < first[n_groups]; an empty range holds nothing)
__device__ __forceinline__ int group_of(const int64_t* __restrict__ first, int n_groups, int64_t x) {
    int lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// the graph of this workgroup's tile, and the tile's first mask within that graph (uniform)
template <bool GROUPED>
__device__ __forceinline__ const PriorityArgs& tile_graph(const PrioIn<GROUPED>& in, uint64_t& first) {
    if constexpr (GROUPED) {
        const int g = group_of(in.first, in.n_groups, (int64_t)blockIdx.x);
        first = (uint64_t)((int64_t)blockIdx.x - in.first[g]) * PDMPC_PRIO_TILE;
        return in.graph[g];
    } else {
        first = (uint64_t)blockIdx.x * PDMPC_PRIO_TILE;
        return in;
    }
}

// peel the orientation F: true if it has no cycle
__device__ __forceinline__ bool prio_acyclic(const PriorityArgs& A, uint32_t F) {
    uint32_t R = A.all_edges;
    while (R != 0u) {
        const uint32_t before = R;
        for (int q = 0; q < A.n_active; ++q) {
            const int v = A.active[q];
            const uint32_t ib = A.in_base[v], ob = A.out_base[v];
            if ((((ib & ~F) | (ob & F)) & R) == 0u) R &= ~(ib | ob);
        }
        if (R == before) return false;
    }
    return true;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

template <bool GROUPED>
__device__ __forceinline__ void count_pass(const PrioIn<GROUPED>& in, uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t wave_count[PDMPC_PRIO_THREADS / PDMPC_WAVE];
    const int wave = (int)threadIdx.x / PDMPC_WAVE;
    uint64_t first;
    const PriorityArgs& A = tile_graph<GROUPED>(in, first);
    uint32_t count = 0;
    for (int r = 0; r < PDMPC_PRIO_ROUNDS; ++r) {
        const uint64_t round0 = first + (uint64_t)r * PDMPC_PRIO_THREADS;
        if (round0 >= A.n_masks) break;  // (uniform)
        const uint64_t m = round0 + threadIdx.x;
        const bool ok = m < A.n_masks && prio_acyclic(A, (uint32_t)m);
        count += (uint32_t)__popcll(__ballot(ok));
    }
    if ((threadIdx.x & (PDMPC_WAVE - 1)) == 0) wave_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < PDMPC_PRIO_THREADS / PDMPC_WAVE; ++w) sum += wave_count[w];
        tile_count[blockIdx.x] = sum;
    }
}

template <bool GROUPED>
__device__ __forceinline__ void write_pass(const PrioIn<GROUPED>& in, const int64_t* __restrict__ tile_off, int64_t capacity, uint32_t* __restrict__ masks) {
    __shared__ uint32_t wave_count[PDMPC_PRIO_THREADS / PDMPC_WAVE];
    const int wave = (int)threadIdx.x / PDMPC_WAVE;
    uint64_t first;
    const PriorityArgs& A = tile_graph<GROUPED>(in, first);
    int64_t pos = tile_off[blockIdx.x];
    for (int r = 0; r < PDMPC_PRIO_ROUNDS; ++r) {
        const uint64_t round0 = first + (uint64_t)r * PDMPC_PRIO_THREADS;
        if (round0 >= A.n_masks) break;  // (uniform)
        const uint64_t m = round0 + threadIdx.x;
        const bool ok = m < A.n_masks && prio_acyclic(A, (uint32_t)m);
        const uint64_t b = __ballot(ok);
        if ((threadIdx.x & (PDMPC_WAVE - 1)) == 0) wave_count[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < PDMPC_PRIO_THREADS / PDMPC_WAVE; ++w) {
            const uint32_t c = wave_count[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        const int64_t at = pos + before + lanes_below(b);
        if (ok && at < capacity) masks[at] = (uint32_t)m;  // (at < capacity always: the host sized masks by the scan's total)
        pos += total;
        __syncthreads();  // (wave_count is rewritten by the next round)
    }
}

template <bool GROUPED>
__device__ __forceinline__ void order_pass(const PrioIn<GROUPED>& in, const uint32_t* __restrict__ masks, int64_t count, int32_t* __restrict__ priorities) {
    const int64_t stride = (int64_t)gridDim.x * PDMPC_PRIO_THREADS;  // (grid-stride: a launch holds fewer than 2^32 threads)
    for (int64_t k = (int64_t)blockIdx.x * PDMPC_PRIO_THREADS + threadIdx.x; k < count; k += stride) {
        const PriorityArgs* graph;
        int32_t* row;
        if constexpr (GROUPED) {
            const int g = group_of(in.first, in.n_groups, k);
            graph = in.graph + g;
            row = priorities + in.row_first[g] + (k - in.first[g]) * graph->n;
        } else {
            graph = &in;
            row = priorities + k * in.n;
        }
        const PriorityArgs& A = *graph;
        const uint32_t F = masks[k];
        uint32_t R = A.all_edges;
        uint64_t placed = 0;
        for (int pos = 1; pos <= A.n; ++pos) {
            for (int v = 0; v < A.n; ++v) {
                if ((placed >> v) & 1ull) continue;
                const uint32_t ib = A.in_base[v], ob = A.out_base[v];
                if ((((ib & ~F) | (ob & F)) & R) == 0u) {  // the smallest vertex that no remaining edge points into
                    row[v] = pos;
                    placed |= 1ull << v;
                    R &= ~(ib | ob);
                    break;
                }
            }
        }
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_PRIO_THREADS) void pdmpc_priority_count_kernel(const PriorityArgs A, uint32_t* __restrict__ tile_count) {
    count_pass<false>(A, tile_count);
}
extern "C" __global__ __launch_bounds__(PDMPC_PRIO_THREADS) void pdmpc_priority_count_grouped_kernel(const PriorityArgs* __restrict__ graph, const int64_t* __restrict__ tile_first,
                                                                                                     int32_t n_groups, uint32_t* __restrict__ tile_count) {
    count_pass<true>(GroupTables{graph, tile_first, nullptr, n_groups}, tile_count);
}

// one workgroup of 1024 threads walks the tile counts in chunks of 1024: a scan per chunk in LDS, plus the carry of the chunks before
extern "C" __global__ __launch_bounds__(1024) void pdmpc_priority_scan_kernel(const uint32_t* __restrict__ tile_count, int64_t n_tiles, int64_t* __restrict__ tile_off) {
    __shared__ int64_t s[1024];
    __shared__ int64_t carry;
    const int t = (int)threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_tiles; base += 1024) {
        const int64_t i = base + t;
        const int64_t v = i < n_tiles ? (int64_t)tile_count[i] : 0;
        s[t] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t add = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        if (i < n_tiles) tile_off[i] = carry + s[t] - v;
        __syncthreads();
        if (t == 1023) carry += s[1023];
        __syncthreads();
    }
    if (t == 0) tile_off[n_tiles] = carry;
}

// grouped: where every graph's masks start in the concatenated list (entry n_groups: the total), read back by the host in one copy
extern "C" __global__ __launch_bounds__(PDMPC_PRIO_THREADS) void pdmpc_priority_group_offsets_kernel(const int64_t* __restrict__ tile_off, const int64_t* __restrict__ tile_first,
                                                                                                     int32_t n_groups, int64_t* __restrict__ mask_first) {
    const int g = (int)(blockIdx.x * PDMPC_PRIO_THREADS + threadIdx.x);
    if (g <= n_groups) mask_first[g] = tile_off[tile_first[g]];
}

extern "C" __global__ __launch_bounds__(PDMPC_PRIO_THREADS) void pdmpc_priority_write_kernel(const PriorityArgs A, const int64_t* __restrict__ tile_off, int64_t capacity,
                                                                                             uint32_t* __restrict__ masks) {
    write_pass<false>(A, tile_off, capacity, masks);
}
extern "C" __global__ __launch_bounds__(PDMPC_PRIO_THREADS) void pdmpc_priority_write_grouped_kernel(const PriorityArgs* __restrict__ graph, const int64_t* __restrict__ tile_first,
                                                                                                     int32_t n_groups, const int64_t* __restrict__ tile_off, int64_t capacity,
                                                                                                     uint32_t* __restrict__ masks) {
    write_pass<true>(GroupTables{graph, tile_first, nullptr, n_groups}, tile_off, capacity, masks);
}

extern "C" __global__ __launch_bounds__(PDMPC_PRIO_THREADS) void pdmpc_priority_order_kernel(const PriorityArgs A, const uint32_t* __restrict__ masks, int64_t count,
                                                                                             int32_t* __restrict__ priorities) {
    order_pass<false>(A, masks, count, priorities);
}
extern "C" __global__ __launch_bounds__(PDMPC_PRIO_THREADS) void pdmpc_priority_order_grouped_kernel(const PriorityArgs* __restrict__ graph, const int64_t* __restrict__ mask_first,
                                                                                                     const int64_t* __restrict__ row_first, int32_t n_groups,
                                                                                                     const uint32_t* __restrict__ masks, int64_t count, int32_t* __restrict__ priorities) {
    order_pass<true>(GroupTables{graph, mask_first, row_first, n_groups}, masks, count, priorities);
}

extern "C" int pdmpc_launch_priority_count(const PriorityArgs* args, int64_t n_tiles, uint32_t* tile_count, void* stream) {
    if (n_tiles <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_priority_count_kernel, dim3((uint32_t)n_tiles), dim3(PDMPC_PRIO_THREADS), 0, (hipStream_t)stream, *args, tile_count);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_priority_scan(const uint32_t* tile_count, int64_t n_tiles, int64_t* tile_off, void* stream) {
    hipLaunchKernelGGL(pdmpc_priority_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, tile_count, n_tiles, tile_off);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_priority_write(const PriorityArgs* args, int64_t n_tiles, const int64_t* tile_off, int64_t capacity, uint32_t* masks, void* stream) {
    if (n_tiles <= 0 || capacity <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_priority_write_kernel, dim3((uint32_t)n_tiles), dim3(PDMPC_PRIO_THREADS), 0, (hipStream_t)stream, *args, tile_off, capacity, masks);
    return (int)hipGetLastError();
}

static int64_t order_blocks(int64_t count) { return std::min<int64_t>((count + PDMPC_PRIO_THREADS - 1) / PDMPC_PRIO_THREADS, (int64_t)1 << 20); }

extern "C" int pdmpc_launch_priority_order(const PriorityArgs* args, const uint32_t* masks, int64_t count, int32_t* priorities, void* stream) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_priority_order_kernel, dim3((uint32_t)order_blocks(count)), dim3(PDMPC_PRIO_THREADS), 0, (hipStream_t)stream, *args, masks, count, priorities);
    return (int)hipGetLastError();
}

// the grouped passes: count over all tiles, and behind the scan the graphs' mask offsets | write | order
extern "C" int pdmpc_launch_priority_count_grouped(const PriorityGroups* g, int64_t n_tiles, uint32_t* tile_count, void* stream) {
    if (n_tiles <= 0 || n_tiles > PDMPC_PRIO_MAX_TILES || g->n_groups < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pdmpc_priority_count_grouped_kernel, dim3((uint32_t)n_tiles), dim3(PDMPC_PRIO_THREADS), 0, (hipStream_t)stream, g->graph, g->tile_first, g->n_groups,
                       tile_count);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_priority_group_offsets(const PriorityGroups* g, const int64_t* tile_off, void* stream) {
    const int blocks = (g->n_groups + 1 + PDMPC_PRIO_THREADS - 1) / PDMPC_PRIO_THREADS;
    hipLaunchKernelGGL(pdmpc_priority_group_offsets_kernel, dim3((uint32_t)blocks), dim3(PDMPC_PRIO_THREADS), 0, (hipStream_t)stream, tile_off, g->tile_first, g->n_groups,
                       g->mask_first);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_priority_write_grouped(const PriorityGroups* g, int64_t n_tiles, const int64_t* tile_off, int64_t capacity, uint32_t* masks, void* stream) {
    if (capacity <= 0) return 0;
    if (n_tiles <= 0 || n_tiles > PDMPC_PRIO_MAX_TILES || g->n_groups < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pdmpc_priority_write_grouped_kernel, dim3((uint32_t)n_tiles), dim3(PDMPC_PRIO_THREADS), 0, (hipStream_t)stream, g->graph, g->tile_first, g->n_groups,
                       tile_off, capacity, masks);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_priority_order_grouped(const PriorityGroups* g, const uint32_t* masks, int64_t count, int32_t* priorities, void* stream) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_priority_order_grouped_kernel, dim3((uint32_t)order_blocks(count)), dim3(PDMPC_PRIO_THREADS), 0, (hipStream_t)stream, g->graph, g->mask_first,
                       g->row_first, g->n_groups, masks, count, priorities);
    return (int)hipGetLastError();
}
