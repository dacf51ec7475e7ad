// sampled_budget_kernel.hip — the sampled optimizer (MonteCarloTreeSearch.m:40-249) with n_expansions_max as a run-time argument
// (pdmpc_set_sampled_budget; the reference reads it from config/mcts.json, :16-26), one wavefront per vehicle.
//
// The search is sampled_search.hpp's, the one pdmpc_sampled_kernel runs.  What a budget other than 250 changes is where two things live:
//   the random numbers   Hp * budget doubles do not fit LDS (2 MB at the limit): the generator's state stays in LDS and the stream is
//                        produced one twist at a time (TwistByTwist).
//   the tree             in LDS where the layout holds it, else in a per-handle HBM buffer (the _hbm instantiation: the accessor is a
//                        template parameter, so the LDS kernel pays nothing for it).
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_math.h"
#include "sampled_budget.h"

namespace {

#include "wave_primitives.hpp"
#include "search_state.hpp"
#include "edge_checks.hpp"
#include "mt19937_device.hpp"
#include "sampled_search.hpp"

}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_sampled_budget_kernel(const SampledArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sampled_slot_body<true, TwistByTwist, ArgumentLimits>(A, (LDS_AS unsigned char*)smem, nullptr);
}

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_sampled_budget_kernel_hbm(const SampledArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sampled_slot_body<false, TwistByTwist, ArgumentLimits>(A, (LDS_AS unsigned char*)smem, A.tree);
}

extern "C" int pdmpc_launch_sampled_budget(const SampledArgs* args, int count, void* stream) {
    if (count <= 0) return 0;
    const bool in_lds = args->tree == nullptr;
    const void* fn = in_lds ? (const void*)pdmpc_sampled_budget_kernel : (const void*)pdmpc_sampled_budget_kernel_hbm;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)args->lds.total);
    if (e != hipSuccess) return (int)e;
    if (in_lds)
        hipLaunchKernelGGL(pdmpc_sampled_budget_kernel, dim3(count), dim3(PDMPC_WAVE), args->lds.total, (hipStream_t)stream, *args);
    else
        hipLaunchKernelGGL(pdmpc_sampled_budget_kernel_hbm, dim3(count), dim3(PDMPC_WAVE), args->lds.total, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}

// The chunked generator on its own: workgroup i writes the first n doubles of mt19937ar(seeds[i]) to out[i][0 .. n), twist by twist
// out of the state's 624 words, by the device functions the kernels above draw with (any n: nothing but the state is held in LDS).
extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_debug_random_stream_kernel(const uint32_t* seeds, int n, double* out) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PDMPC_SB_MT_BYTES];
    mt19937_doubles_wave(seeds[blockIdx.x], n, (lds_u32*)(LDS_AS unsigned char*)smem, out + (size_t)blockIdx.x * (size_t)n, (int)threadIdx.x);
}

extern "C" int pdmpc_launch_debug_random_stream(const uint32_t* seeds, int count, int n, double* out, void* stream) {
    if (count <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_debug_random_stream_kernel, dim3(count), dim3(PDMPC_WAVE), 0, (hipStream_t)stream, seeds, n, out);
    return (int)hipGetLastError();
}
