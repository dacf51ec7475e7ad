// sampled_kernel.hip — the reference's sampled optimizer (OptimizerType.MatlabSampled) at its own budget of 250 expansions
// (MonteCarloTreeSearch.m:8), one wavefront per vehicle.
//
// The search is sampled_search.hpp's, specialised for the reference's numbers: budget and tree rows are compile-time constants, and
// the Hp * 250 doubles of mt19937ar(seed) -- the host generator's bits -- are drawn into LDS ahead of the predecessor wait, with the
// tree's region as the generator's scratch.  Tables and the obstacle soups are staged in LDS exactly as in the graph search
// (search_common.hpp).  A whole time step is one launch (pdmpc_plan_step_sampled): slots are in level order.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_math.h"
#include "sampled_budget.h"

namespace {

#include "wave_primitives.hpp"
#include "search_state.hpp"
#include "edge_checks.hpp"
#include "mt19937_device.hpp"
#include "sampled_search.hpp"

static_assert(PDMPC_SB_DEFAULT_ROWS > 1 + PDMPC_SAMPLED_BUDGET_DEFAULT + PDMPC_HP_MAX, "the last descent may overshoot the limit by Hp - 1 nodes");
static_assert(PDMPC_SB_DEFAULT_ROWS * PDMPC_SB_ROW * 2 >= PDMPC_SB_MT_BYTES, "the tree region holds the generator's state");

}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_sampled_kernel(const SampledArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sampled_slot_body<true, DrawnAhead, ReferenceLimits>(A, (LDS_AS unsigned char*)smem, nullptr);
}

extern "C" int pdmpc_launch_sampled(const SampledArgs* args, int count, void* stream) {
    if (count <= 0) return 0;
    hipError_t e = hipFuncSetAttribute((const void*)pdmpc_sampled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)args->lds.total);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pdmpc_sampled_kernel, dim3(count), dim3(PDMPC_WAVE), args->lds.total, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
