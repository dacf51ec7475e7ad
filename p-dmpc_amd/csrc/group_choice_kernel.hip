// group_choice_kernel.hip — the choice among the plans of a batch whose records lie on the ranks of a group (pdmpc_choice over
// pdmpc_group_*, include/pdmpc.h).  The contract is choice_kernel.hip's and pdmpc_choose_host's: sums from +0.0 IN LIST
// ORDER, round(., 8), the first minimum per graph.  f64 throughout, compiled without contraction like the searches.
//
//   entries  ONE workgroup per rank over the records the rank holds: (cost of the final node, status) of each as a 16-byte entry, and
//            in front of them the rank's status counters (records that outgrew their arena / timed out / carry any other status that
//            is no planning result), summed in LDS — one workgroup, so no global atomic and nothing to clear between calls.
//   (the ranks' blocks are all-gathered by group.cpp: 16 bytes per record, never the record)
//   cells    on EVERY rank, on the gathered blocks: one wavefront per graph, lanes striding over its candidates, each adding its cell's
//            costs one after the other in list order; the (value, index) reduction, the smaller index winning a tie also between
//            candidates 64 lanes apart.  Cells of no graph one lane per cell.  Every rank computes the same bits from the same
//            entries, in the list's order and not the ranks': chosen and cell_cost are the host twin's.
//   gather   on every rank: a workgroup per pick whose chosen record this rank holds copies it, in 8-byte words, to pick i of the ONE
//            block in host memory that the ranks share; exactly one rank holds a record, so exactly one writes a pick.  Rank 0 also
//            writes the counters, summed over the ranks' headers, chosen and cell_cost there.
// Entries another device wrote arrive by the collective's copies, ordered before these launches by its events (or RCCL's stream
// order); they are read with per-lane (vector) loads.  Stores to host memory are ordinary vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "group_choice.h"

static_assert(sizeof(pdmpc_vehicle_out) % 8 == 0 && alignof(pdmpc_vehicle_out) == 8, "the gather copies records in 8-byte words");

namespace {
__device__ double group_cell_cost_of(const GroupChoiceArgs& A, int cell) {
    double sum = 0.0;
    for (int q = A.cell_offset[cell], e = A.cell_offset[cell + 1]; q < e; ++q) {
        const GroupEntry& r = A.gathered[A.cell_entry[q]];
        sum += r.status == PDMPC_OK ? r.cost : __builtin_inf();
    }
    return nearbyint(sum * 1e8) / 1e8;
}
}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_GROUP_ENTRIES_BLOCK) void pdmpc_group_entries_kernel(const GroupEntriesArgs A) {
    __shared__ int counts[PDMPC_CHOICE_COUNTERS];
    const int t = (int)threadIdx.x;
    if (t < PDMPC_CHOICE_COUNTERS) counts[t] = 0;
    __syncthreads();
    int overflow = 0, timed_out = 0, other = 0;
    for (int i = t; i < A.n_a + A.n_b; i += PDMPC_GROUP_ENTRIES_BLOCK) {
        const pdmpc_vehicle_out& r = i < A.n_a ? A.rec_a[i] : A.rec_b[i - A.n_a];
        const int st = r.status;
        GroupEntry e;
        e.cost = r.path_nodes[A.Hp][4];
        e.status = st;
        e._pad = 0;
        A.block[1 + i] = e;
        overflow += st == PDMPC_ARENA_OVERFLOW;
        timed_out += st == PDMPC_ERR_HIP;
        other += st != PDMPC_OK && st != PDMPC_EXHAUSTED && st != PDMPC_ARENA_OVERFLOW && st != PDMPC_ERR_HIP;
    }
    if (overflow) atomicAdd(&counts[PDMPC_CHOICE_OVERFLOW], overflow);
    if (timed_out) atomicAdd(&counts[PDMPC_CHOICE_TIMED_OUT], timed_out);
    if (other) atomicAdd(&counts[PDMPC_CHOICE_OTHER], other);
    __syncthreads();
    if (t < PDMPC_CHOICE_COUNTERS) ((int32_t*)A.block)[t] = counts[t];
}

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_group_cells_kernel(const GroupChoiceArgs A) {
    const int lane = (int)threadIdx.x;
    const int n_stray = A.n_cells - (A.end_graph_cell - A.first_graph_cell);
    const int n_units = A.n_graphs + (n_stray + PDMPC_WAVE - 1) / PDMPC_WAVE;  // a graph, or 64 cells of no graph
    for (int u = (int)blockIdx.x; u < n_units; u += (int)gridDim.x) {
        if (u >= A.n_graphs) {
            const int q = (u - A.n_graphs) * PDMPC_WAVE + lane;
            if (q < n_stray) {
                const int cell = q < A.first_graph_cell ? q : q - A.first_graph_cell + A.end_graph_cell;
                A.cell_cost[cell] = group_cell_cost_of(A, cell);
            }
            continue;
        }
        const int c0 = A.graph_offset[u], count = A.graph_offset[u + 1] - c0;
        double best = __builtin_inf();
        int best_i = 0x7fffffff;
        for (int i = lane; i < count; i += PDMPC_WAVE) {
            const double v = group_cell_cost_of(A, c0 + i);
            A.cell_cost[c0 + i] = v;
            if (v < best || (v == best && i < best_i)) {
                best = v;
                best_i = i;
            }
        }
        for (int d = PDMPC_WAVE / 2; d >= 1; d >>= 1) {
            const double v = __shfl_xor(best, d, PDMPC_WAVE);
            const int i = __shfl_xor(best_i, d, PDMPC_WAVE);
            if (v < best || (v == best && i < best_i)) {
                best = v;
                best_i = i;
            }
        }
        if (lane == 0) A.chosen[u] = count > 0 ? best_i : 0;
    }
}

extern "C" __global__ __launch_bounds__(PDMPC_CHOICE_GATHER_BLOCK) void pdmpc_group_gather_kernel(const GroupChoiceArgs A) {
    const int t = (int)threadIdx.x;
    const int stride = A.per + 1;
    constexpr int kWords = (int)(sizeof(pdmpc_vehicle_out) / 8);
    pdmpc_vehicle_out* picks = (pdmpc_vehicle_out*)(A.host_block + A.off_picks);
    for (int i = (int)blockIdx.x; i < A.n_picks; i += (int)gridDim.x) {
        const int g = A.pick_graph[i];
        const int e = A.pick_entry[A.pick_offset[i] + (g < 0 ? 0 : A.chosen[g])];
        if (e / stride != A.rank) continue;  // another rank holds the record and writes this pick
        const int p = e % stride - 1;
        const pdmpc_vehicle_out* rec = p < A.n_a ? A.rec_a + p : A.rec_b + (p - A.n_a);
        const unsigned long long* src = (const unsigned long long*)rec;
        unsigned long long* dst = (unsigned long long*)(picks + i);
        for (int w = t; w < kWords; w += PDMPC_CHOICE_GATHER_BLOCK) dst[w] = src[w];
    }
    if (A.rank != 0) return;
    const int id = (int)blockIdx.x * PDMPC_CHOICE_GATHER_BLOCK + t, n_threads = (int)gridDim.x * PDMPC_CHOICE_GATHER_BLOCK;
    int32_t* chosen = (int32_t*)(A.host_block + A.off_chosen);
    double* cell_cost = (double*)(A.host_block + A.off_cell_cost);
    for (int g = id; g < A.n_graphs; g += n_threads) chosen[g] = A.chosen[g];
    for (int c = id; c < A.n_cells; c += n_threads) cell_cost[c] = A.cell_cost[c];
    if (id < PDMPC_CHOICE_COUNTERS) {
        int sum = 0;
        for (int r = 0; r < A.world; ++r) sum += ((const int32_t*)(A.gathered + (size_t)r * stride))[id];
        ((int32_t*)A.host_block)[id] = sum;
    }
}

extern "C" int pdmpc_launch_group_entries(const GroupEntriesArgs* args, void* stream) {
    hipLaunchKernelGGL(pdmpc_group_entries_kernel, dim3(1), dim3(PDMPC_GROUP_ENTRIES_BLOCK), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_group_cells(const GroupChoiceArgs* args, void* stream) {
    const int n_stray = args->n_cells - (args->end_graph_cell - args->first_graph_cell);
    const int units = args->n_graphs + (n_stray + PDMPC_WAVE - 1) / PDMPC_WAVE;
    if (units <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_group_cells_kernel, dim3(std::min(units, PDMPC_GROUP_CELLS_MAX_WAVES)), dim3(PDMPC_WAVE), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_group_gather(const GroupChoiceArgs* args, void* stream) {
    const int blocks = std::min(std::max(args->n_picks, 1), PDMPC_GROUP_GATHER_MAX_BLOCKS);
    hipLaunchKernelGGL(pdmpc_group_gather_kernel, dim3(blocks), dim3(PDMPC_CHOICE_GATHER_BLOCK), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
