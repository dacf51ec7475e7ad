// sampled_budget.h — what the host and the sampled optimizer's kernels share: the tree's rows (sampled_search.hpp), and the ONE
// argument record of the sampled optimizer with its launchers.  The budget of MonteCarloTreeSearch.m:8 (250) runs
// pdmpc_sampled_kernel, which has it compiled in; every other budget (pdmpc_set_sampled_budget) runs the pdmpc_sampled_budget kernels.
#pragma once
#include "pdmpc_device.h"

// One tree node: a row of PDMPC_SB_ROW 16-bit words -- children(1:16, node), parent, trim -- written whole when the node is created.
#define PDMPC_SB_FANOUT 16
#define PDMPC_SB_PARENT 16
#define PDMPC_SB_TRIM 17
#define PDMPC_SB_ROW 18
#define PDMPC_SB_TWIST 312 /* doubles of one twist of mt19937ar: the chunk the kernel draws its random numbers in */
#define PDMPC_SB_MT_BYTES (624u * 4u)
#define PDMPC_SB_DEFAULT_ROWS 288 /* pdmpc_sampled_kernel's tree: > 1 + 250 + PDMPC_HP_MAX */

// Rows a tree of budget B has room for.  A descent starts with fewer than B expansions and at most one node per expansion behind the
// root, n_nodes <= B, so `n_nodes + Hp < capacity` -- the guard pdmpc_sampled_kernel ends its loop on at 288 rows -- holds for ever
// with B + PDMPC_HP_MAX + 1 rows: the reference has no such guard.  The last descent ends with n_nodes <= B + Hp - 1.
static inline uint32_t pdmpc_sb_node_cap(uint32_t budget) { return (budget + PDMPC_HP_MAX + 2u + 7u) & ~7u; }
static inline uint32_t pdmpc_sb_tree_bytes(uint32_t budget) { return pdmpc_sb_node_cap(budget) * PDMPC_SB_ROW * 2u; }

// What every sampled kernel takes (the ensemble's kernels inside SampledEnsembleArgs); the host fills it in one place
// (sampled_launch.hpp: sampled_args).  The graph search's KernelArgs is no part of a sampled launch.
struct SampledArgs {
    // the automaton
    const uint64_t* succ_mask;
    const int16_t* man_index;
    const DevManPose* man_pose;
    const double* man_area;  // double2 pairs
    int32_t n_trims, n_words, n_man, Hp;
    int32_t checker, areas_in_lds;
    // the batch and its records
    const DevVehicle* veh;
    const double* points;  // double2 pairs
    const int32_t* pred;
    pdmpc_vehicle_out* out;
    uint32_t* done_flag;
    uint32_t epoch;
    int32_t first, n_searches, reverse_dispatch;
    uint32_t spin_limit;
    int32_t* tree_size;
    unsigned long long* work_count;
    // the layout (launch_plan.hpp: layout_sampled): tree16 holds the tree if it is in LDS, rand the generator's 624 state words
    LdsLayout lds;
    int32_t budget;    // n_expansions_max (pdmpc_sampled_kernel: 250, compiled in)
    int32_t node_cap;  // rows of a slot's tree (pdmpc_sb_node_cap; pdmpc_sampled_kernel: PDMPC_SB_DEFAULT_ROWS, compiled in)
    uint16_t* tree;    // the trees in HBM, node_cap rows per slot (the _hbm kernel; null where the tree is in LDS)
};

#ifdef __cplusplus
extern "C" {
#endif
// sampled_kernel.hip: the sampled optimizer (MonteCarloTreeSearch.m) at the reference's budget, `count` workgroups of one wavefront
int pdmpc_launch_sampled(const SampledArgs* args, int count, void* stream);
// sampled_budget_kernel.hip: `count` workgroups of one wavefront; the tree in LDS (tree == null) or in HBM
int pdmpc_launch_sampled_budget(const SampledArgs* args, int count, void* stream);
// ... and its generator alone: out[i][0 .. n) = the first n doubles of mt19937ar(seeds[i]), one twist at a time
int pdmpc_launch_debug_random_stream(const uint32_t* seeds, int count, int n, double* out, void* stream);
#ifdef __cplusplus
}
#endif
