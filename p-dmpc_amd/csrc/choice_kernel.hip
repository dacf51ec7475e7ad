// choice_kernel.hip — the choice among the plans of a batch on the device (pdmpc_choice, include/pdmpc.h): what
// PrioritizedExplorativeController.m:94-176 and PrioritizedOptimalController.m:56-114 do with the plans of all prioritizations, on the
// result records where the search left them.  f64 throughout, compiled without contraction like the searches.
//
//   pass 1  one wavefront per graph.  Lanes stride over the graph's candidates; a lane adds its cell's costs one after the other IN
//           LIST ORDER (the order is the contract: the bits are the host twin's), rounds as round(., 8) and writes the cell's cost;
//           the wavefront then reduces on (value, index), the smaller index winning a tie — also a tie between candidates 64 lanes
//           apart — and writes the first minimum.  Wavefronts beyond the graphs take the cells that belong to no graph, one lane per
//           cell.  All lanes of the launch together look at every record of the batch once and count the statuses that are no
//           planning results (vector integer atomics; none in a launch without such a record).
//   pass 2  one workgroup per pick: the record of the slot its graph chose (or its single slot), copied in 8-byte words — the record is
//           a multiple of 8 bytes but not of 16, so every other record starts on no 16-byte boundary.  Workgroup 0 moves the status
//           counters to where the call reads them back and clears the tally for the next call.
// The dependency decides the two launches: a pick needs its graph's minimum, the minimum every cell of the graph.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pdmpc_device.h"

static_assert(sizeof(pdmpc_vehicle_out) % 8 == 0 && sizeof(pdmpc_vehicle_out) % 16 != 0 && alignof(pdmpc_vehicle_out) == 8,
              "the gather copies records in 8-byte words: the widest their size and alignment allow");

namespace {
__device__ double cell_cost_of(const ChoiceArgs& A, int cell) {
    double sum = 0.0;
    for (int q = A.cell_offset[cell], e = A.cell_offset[cell + 1]; q < e; ++q) {
        const pdmpc_vehicle_out& r = A.rec[A.cell_slot[q]];
        sum += r.status == PDMPC_OK ? r.path_nodes[A.Hp][4] : __builtin_inf();
    }
    return nearbyint(sum * 1e8) / 1e8;
}
}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_choice_cells_kernel(const ChoiceArgs A) {
    const int lane = (int)threadIdx.x;
    // every record of the batch once, by whichever lane of the launch comes by
    int overflow = 0, timed_out = 0, other = 0;
    for (int i = (int)blockIdx.x * PDMPC_WAVE + lane; i < A.n; i += (int)gridDim.x * PDMPC_WAVE) {
        const int st = A.rec[i].status;
        overflow += st == PDMPC_ARENA_OVERFLOW;
        timed_out += st == PDMPC_ERR_HIP;
        other += st != PDMPC_OK && st != PDMPC_EXHAUSTED && st != PDMPC_ARENA_OVERFLOW && st != PDMPC_ERR_HIP;
    }
    if (overflow) atomicAdd(A.tally + PDMPC_CHOICE_OVERFLOW, overflow);
    if (timed_out) atomicAdd(A.tally + PDMPC_CHOICE_TIMED_OUT, timed_out);
    if (other) atomicAdd(A.tally + PDMPC_CHOICE_OTHER, other);

    const int g = (int)blockIdx.x;
    if (g >= A.n_graphs) {  // cells of no graph
        const int q = (g - A.n_graphs) * PDMPC_WAVE + lane;
        const int n_stray = A.n_cells - (A.end_graph_cell - A.first_graph_cell);
        if (q < n_stray) {
            const int cell = q < A.first_graph_cell ? q : q - A.first_graph_cell + A.end_graph_cell;
            A.cell_cost[cell] = cell_cost_of(A, cell);
        }
        return;
    }
    const int c0 = A.graph_offset[g], count = A.graph_offset[g + 1] - c0;
    double best = __builtin_inf();
    int best_i = 0x7fffffff;
    for (int i = lane; i < count; i += PDMPC_WAVE) {
        const double v = cell_cost_of(A, c0 + i);
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
    if (lane == 0) A.chosen[g] = count > 0 ? best_i : 0;
}

extern "C" __global__ __launch_bounds__(PDMPC_CHOICE_GATHER_BLOCK) void pdmpc_choice_gather_kernel(const ChoiceArgs A) {
    const int i = (int)blockIdx.x, t = (int)threadIdx.x;
    if (i == 0 && t < PDMPC_CHOICE_COUNTERS) {
        A.counters[t] = A.tally[t];
        A.tally[t] = 0;
    }
    if (i >= A.n_picks) return;
    const int g = A.pick_graph[i];
    const int slot = A.pick_slot[A.pick_offset[i] + (g < 0 ? 0 : A.chosen[g])];
    const unsigned long long* src = (const unsigned long long*)(A.rec + slot);
    unsigned long long* dst = (unsigned long long*)(A.picks + i);
    constexpr int kWords = (int)(sizeof(pdmpc_vehicle_out) / 8);
    for (int w = t; w < kWords; w += PDMPC_CHOICE_GATHER_BLOCK) dst[w] = src[w];
}

extern "C" int pdmpc_launch_choice(const ChoiceArgs* args, void* stream) {
    const int n_stray = args->n_cells - (args->end_graph_cell - args->first_graph_cell);
    const int waves = std::max(args->n_graphs + (n_stray + PDMPC_WAVE - 1) / PDMPC_WAVE, 1);
    hipLaunchKernelGGL(pdmpc_choice_cells_kernel, dim3(waves), dim3(PDMPC_WAVE), 0, (hipStream_t)stream, *args);
    if (const hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(pdmpc_choice_gather_kernel, dim3(std::max(args->n_picks, 1)), dim3(PDMPC_CHOICE_GATHER_BLOCK), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
