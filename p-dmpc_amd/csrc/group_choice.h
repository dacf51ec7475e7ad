// group_choice.h — what group.cpp and group_choice_kernel.hip share: the choice among the plans of a batch whose records lie on the
// ranks of a group (pdmpc_group_plan_step_chosen, include/pdmpc.h).  No HIP header: plain structs and prototypes.
//
// A rank HOLDS the records it planned last: those of its whole components in its handle's record buffer (rec_a), rank 0 also those of
// the component planned by levels (rec_b, behind its own).  A held record's place is (rank, position); what the ranks exchange of it
// is one GroupEntry.  A rank's block of an exchange is per + 1 entries: a header with the rank's status counters, then its entries.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pdmpc_device.h"

struct GroupEntry {
    double cost;     // path_nodes[Hp][4] of the record, whatever its status
    int32_t status;  // ... and its status
    int32_t _pad;
};
static_assert(sizeof(GroupEntry) == 16, "an exchanged entry is 16 bytes");
// the header of a rank's block: counters[PDMPC_CHOICE_COUNTERS] of the records it holds, in a GroupEntry's 16 bytes
static_assert(PDMPC_CHOICE_COUNTERS * sizeof(int32_t) == sizeof(GroupEntry), "the status counters fill one entry");

#define PDMPC_GROUP_ENTRIES_BLOCK 1024  // the ONE workgroup that writes a rank's block (its counters need no global atomic)
#define PDMPC_GROUP_CELLS_MAX_WAVES 64  // wavefronts of the cells-and-minima pass: graphs and stray cells beyond them are strided over
#define PDMPC_GROUP_GATHER_MAX_BLOCKS 256  // workgroups of the gather: picks beyond them are strided over

struct GroupEntriesArgs {
    const pdmpc_vehicle_out* rec_a;  // the first n_a records the rank holds
    const pdmpc_vehicle_out* rec_b;  // ... and the n_b behind them (may be null with n_b == 0)
    int32_t n_a, n_b, Hp, _pad;
    GroupEntry* block;  // [1 + n_a + n_b]: header, entries (device memory, or host memory mapped into the device)
};

struct GroupChoiceArgs {
    const GroupEntry* gathered;  // [world][per + 1] every rank's block
    int32_t world, per, rank;
    int32_t n_cells, n_graphs, n_picks;
    int32_t first_graph_cell, end_graph_cell;
    // the caller's lists with every slot replaced by its entry index rank * (per + 1) + 1 + position (group_route.hpp)
    const int32_t* cell_offset;   // [n_cells + 1]
    const int32_t* cell_entry;
    const int32_t* graph_offset;  // [n_graphs + 1]
    const int32_t* pick_graph;    // [n_picks]
    const int32_t* pick_offset;   // [n_picks + 1]
    const int32_t* pick_entry;
    int32_t* chosen;    // [n_graphs] this rank's device memory
    double* cell_cost;  // [n_cells]
    const pdmpc_vehicle_out* rec_a;  // the records this rank holds, as in GroupEntriesArgs
    const pdmpc_vehicle_out* rec_b;
    int32_t n_a, _pad;
    // The block the host reads (choice_host.hpp: ChoiceLayout), in host memory mapped into every device: every rank writes the picks it
    // holds, rank 0 also the counters (summed over the ranks' headers), chosen and cell_cost.
    unsigned char* host_block;
    size_t off_chosen, off_cell_cost, off_picks;
};

#ifdef __cplusplus
extern "C" {
#endif
// group_choice_kernel.hip: a rank's block of entries; the cells and first minima on the gathered blocks; the gather of the picks a rank holds
int pdmpc_launch_group_entries(const GroupEntriesArgs* args, void* stream);
int pdmpc_launch_group_cells(const GroupChoiceArgs* args, void* stream);
int pdmpc_launch_group_gather(const GroupChoiceArgs* args, void* stream);
#ifdef __cplusplus
}
#endif
