// sampled_ensemble_kernel.hip — the sampled optimizer (MonteCarloTreeSearch.m:40-249) planned as a seed ensemble
// (pdmpc_set_sampled_ensemble): E members per vehicle, one wavefront each, the cheapest collision-free plan wins on
// the device.
//
// The grid is count * E workgroups; block b is member b % E of slot b / E (reverse_dispatch turns the slots round as in the other
// sampled kernels), so all members of a slot lie below the blocks of its successors.  A member is sampled_search.hpp's search as the
// sampled_budget kernels run it, at any budget, called with three things of its own: its seed PDMPC_SAMPLED_MEMBER_SEED(seed, e), its
// record member_out[slot * E + e] in place of out[slot], and its tree (LDS, or tree slot * E + e of the HBM buffer).  Every member
// reads the same soups: the literal ones and the areas its predecessors published in out[].  An exhausted member has the fallback
// areas in its record, so that member 0's is the slot's record as the other sampled kernels write it if no member is OK.
//
// The protocol of a slot (split-K's "last block reduces"):
//   every member   writes its record, its tree size and its 16-byte entry (status, expansions, final cost) with vector stores, drains
//                  them, then lane 0: release fence (agent), s_waitcnt vmcnt(0), relaxed agent-scope fetch_add on the slot's ticket.
//   ticket E - 1   (the member that arrives last, whichever it is) one agent-scope acquire; reads the E entries with vector loads
//                  (lane e reads entry e: never through the scalar cache); picks the winner -- the smallest cost among the members
//                  with PDMPC_OK, compared with <, members in ascending order, so the lowest index wins a tie --; copies the
//                  chosen record to out[slot] with vector loads and stores; drains; releases and stores the done flag like the
//                  other sampled kernels.  No member OK: member 0's record (PDMPC_EXHAUSTED, with the fallback areas its search
//                  published in it).  A member that timed out waiting for a predecessor: that member's record (PDMPC_ERR_HIP).
//   No member waits for a member, and a member that does not draw the last ticket is finished: a workgroup depends only on the done
//   flags of predecessor slots, whose blocks all lie below it.
// Tickets: the host clears the tickets of the launched slots on the stream ahead of every launch (sampled_launch.hpp: launch_sampled) -- also right
// after a launch that failed half-way, which a last arriver that restores them is not.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_math.h"
#include "sampled_ensemble.h"

namespace {

#include "wave_primitives.hpp"
#include "search_state.hpp"
#include "edge_checks.hpp"
#include "mt19937_device.hpp"
#include "sampled_search.hpp"

template <bool IN_LDS>
__device__ __forceinline__ void sampled_ensemble_body(const SampledEnsembleArgs& G, LDS_AS unsigned char* lsm) {
    const SampledArgs& A = G.s;
    const int lane = threadIdx.x;
    const int E = G.n_members;
    const int b_slot = (int)blockIdx.x / E;
    const int e = (int)blockIdx.x - b_slot * E;
    const int slot = A.first + (A.reverse_dispatch ? A.n_searches - 1 - b_slot : b_slot);
    const size_t base = (size_t)slot * (size_t)E;
    pdmpc_vehicle_out* const mine = G.member_out + base + e;

    const SearchResult R = sampled_search<IN_LDS, TwistByTwist, ArgumentLimits>(A, lsm, slot, PDMPC_SAMPLED_MEMBER_SEED(A.veh[slot].seed, e), mine,
                                                                                IN_LDS ? nullptr : A.tree + (base + e) * (size_t)A.node_cap * PDMPC_SB_ROW);

    // ---- arrive: the entry and the tree size behind the record, everything drained, then the ticket
    if (lane == 0) {
        EnsembleEntry en;
        en.status = R.status;
        en.n_expanded = R.n_expanded;
        en.cost = R.cost;
        G.entries[base + e] = en;
        G.member_nodes[base + e] = R.n_nodes;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    uint32_t ticket = 0;
    if (lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(G.tickets + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ticket = uni_u(ticket);
    if (ticket != (uint32_t)(E - 1)) return;  // (not the last: finished, without waiting for anybody)

    // ---- the member that arrived last acts for the slot
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    int st = PDMPC_EXHAUSTED;
    double cost = 0.0;
    if (lane < E) {  // (lane-dependent index: vector loads)
        const EnsembleEntry* en = G.entries + base + lane;
        st = en->status;
        cost = en->cost;
    }
    const unsigned long long timed = __ballot(lane < E && st == PDMPC_ERR_HIP);
    unsigned long long ok = __ballot(lane < E && st == PDMPC_OK);
    int chosen = 0;
    if (timed != 0ull) {
        chosen = uni_i(__builtin_ctzll(timed));
    } else if (ok != 0ull) {
        chosen = uni_i(__builtin_ctzll(ok));
        double best = lane_d(cost, chosen);
        for (ok &= ok - 1; ok != 0ull; ok &= ok - 1) {  // ascending members, <: the lowest index wins a tie
            const int q = uni_i(__builtin_ctzll(ok));
            const double cq = lane_d(cost, q);
            if (cq < best) {
                best = cq;
                chosen = q;
            }
        }
    }
    {
        const double* src = (const double*)(G.member_out + base + chosen);
        double* dst = (double*)(A.out + slot);
        const int nd = (int)(sizeof(pdmpc_vehicle_out) / 8);
        for (int i = lane; i < nd; i += PDMPC_WAVE) dst[i] = src[i];
        if (lane == 0) {
            A.tree_size[slot] = __hip_atomic_load(G.member_nodes + base + chosen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            G.chosen[slot] = chosen;
        }
    }
    sampled_release_slot(A, slot);  // publish like the other sampled kernels
}

}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_sampled_ensemble_kernel(const SampledEnsembleArgs G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sampled_ensemble_body<true>(G, (LDS_AS unsigned char*)smem);
}

extern "C" __global__ __launch_bounds__(PDMPC_WAVE) void pdmpc_sampled_ensemble_kernel_hbm(const SampledEnsembleArgs G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sampled_ensemble_body<false>(G, (LDS_AS unsigned char*)smem);
}

extern "C" int pdmpc_launch_sampled_ensemble(const SampledEnsembleArgs* args, int count, void* stream) {
    if (count <= 0) return 0;
    if (args->n_members < 2 || args->n_members > PDMPC_SAMPLED_ENSEMBLE_MAX) return (int)hipErrorInvalidValue;
    const bool in_lds = args->s.tree == nullptr;
    const void* fn = in_lds ? (const void*)pdmpc_sampled_ensemble_kernel : (const void*)pdmpc_sampled_ensemble_kernel_hbm;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)args->s.lds.total);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)count * (unsigned)args->n_members);
    if (in_lds)
        hipLaunchKernelGGL(pdmpc_sampled_ensemble_kernel, grid, dim3(PDMPC_WAVE), args->s.lds.total, (hipStream_t)stream, *args);
    else
        hipLaunchKernelGGL(pdmpc_sampled_ensemble_kernel_hbm, grid, dim3(PDMPC_WAVE), args->s.lds.total, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
