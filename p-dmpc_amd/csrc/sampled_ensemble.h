// sampled_ensemble.h — what the host and sampled_ensemble_kernel.hip share: the arguments of the sampled optimizer planned as a seed
// ensemble (pdmpc_set_sampled_ensemble) and its launcher.  One member (the default) keeps pdmpc_sampled_kernel and
// the kernels of sampled_budget.h; two or more run the kernels declared here at any budget.
#pragma once
#include "sampled_budget.h"

// What a member leaves for the member that arrives last at its slot: 16 bytes, written whole.
struct EnsembleEntry {
    int32_t status;      // PDMPC_OK / PDMPC_EXHAUSTED, or PDMPC_ERR_HIP if the member timed out waiting for a predecessor
    int32_t n_expanded;  // its expansions
    double cost;         // path_nodes[Hp][4] of its record if status == PDMPC_OK, +inf otherwise
};

struct SampledEnsembleArgs {
    SampledArgs s;            // the search: out = the slots' records, tree = n_members trees per slot (member e of slot s: tree s * E + e)
    int32_t n_members;              // E: block b is member b % E of slot b / E
    pdmpc_vehicle_out* member_out;  // [slot * E + e] every member's full record
    EnsembleEntry* entries;         // [slot * E + e]
    uint32_t* tickets;              // [slot] members arrived; zero when a launch starts (the host clears them on the stream ahead of it)
    int32_t* member_nodes;          // [slot * E + e] the member's tree size (tree_size[slot] becomes the chosen member's)
    int32_t* chosen;                // [slot] the member whose record the last arriver copied to out[slot]
};

#ifdef __cplusplus
extern "C" {
#endif
// sampled_ensemble_kernel.hip: `count` slots, count * n_members workgroups of one wavefront; the trees in LDS (s.tree == null) or in HBM
int pdmpc_launch_sampled_ensemble(const SampledEnsembleArgs* args, int count, void* stream);
#ifdef __cplusplus
}
#endif
