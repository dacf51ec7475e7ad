// hdv_grouped_host.hpp — the host-only rules of the grouped HDV traffic call (pdmpc_hdv_traffic_grouped): where every
// group's blocks stand in the call's arrays (ONE statement of it: the device call, the sweep's stage and the Python wrapper all go
// through pdmpc_hdv_grouped_layout_host, which is hdv_grouped_layout), and how the HDV members of a lock-step become batches of one
// call each and find their maps on the handle's map slots.  No HIP header, no handle (tests/hdv_grouped_checks.cpp runs this file
// under the sanitizers).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/pdmpc.h"

// Group g of n_groups (hdv_offset / cav_offset [n_groups + 1]: from 0, non-decreasing) with h0 = hdv_offset[g]:
//   closest_at[g]    first entry of its closest_offset block (n_g + 1 entries): h0 + g
//   list_at[g]       ... of its closest_index and row_hdv blocks: h0 PDMPC_HDV_MAX_CHAINS
//   set_offset_at[g] ... of its set_offset block (n_rows[g] Hp + 1 entries): h0 PDMPC_HDV_MAX_CHAINS Hp + g
//   set_at[g]        ... of its set_flags block: h0 PDMPC_HDV_MAX_CHAINS Hp
//   adjacency_at[g]  ... of its adjacency block (n_cav_g x n_hdv_g): the sum of n_cav_h n_hdv_h over the groups h < g
// Entry n_groups of each is the room the array needs (where a further group's block would start).  Any output may be null.
inline int hdv_grouped_layout(int32_t n_groups, const int32_t* hdv_offset, const int32_t* cav_offset, int32_t Hp, int32_t* closest_at, int32_t* list_at,
                              int32_t* set_offset_at, int32_t* set_at, int64_t* adjacency_at) {
    if (n_groups < 0 || Hp < 1 || !hdv_offset || !cav_offset || hdv_offset[0] != 0 || cav_offset[0] != 0) return PDMPC_ERR_INVALID;
    for (int g = 0; g < n_groups; ++g)
        if (hdv_offset[g + 1] < hdv_offset[g] || cav_offset[g + 1] < cav_offset[g]) return PDMPC_ERR_INVALID;
    // (the blocks are indexed in 32 bits)
    if ((int64_t)hdv_offset[n_groups] * PDMPC_HDV_MAX_CHAINS * Hp + n_groups > INT32_MAX) return PDMPC_ERR_CAPACITY;
    int64_t pairs = 0;
    for (int g = 0; g <= n_groups; ++g) {
        const int32_t h0 = hdv_offset[g];
        if (closest_at) closest_at[g] = h0 + g;
        if (list_at) list_at[g] = h0 * PDMPC_HDV_MAX_CHAINS;
        if (set_offset_at) set_offset_at[g] = h0 * PDMPC_HDV_MAX_CHAINS * Hp + g;
        if (set_at) set_at[g] = h0 * PDMPC_HDV_MAX_CHAINS * Hp;
        if (adjacency_at) adjacency_at[g] = pairs;
        if (g < n_groups) pairs += (int64_t)(cav_offset[g + 1] - cav_offset[g]) * (hdv_offset[g + 1] - h0);
    }
    return PDMPC_OK;
}

// ---- the members of a lock-step as batches (step_prepare.hpp: hdv_traffic_stage; step_hdv.hpp: the batch path)

// what a controller remembers of the slot its map was found in or uploaded to: the slot still holds that map while the slot's
// generation is the remembered one (every upload into a slot takes a new generation; 0: none)
struct HdvSlotNote {
    int32_t slot = -1;
    int64_t generation = 0;
};

// One grouped call: its members in member order, the distinct maps among them (by content) and which of them every member drives on
struct HdvBatch {
    std::vector<int> members;
    std::vector<int> map_of;   // [members.size()] index into maps
    std::vector<int> maps;     // the first member of the batch with each distinct map
    std::vector<int32_t> slot; // [maps.size()] the handle's slot of each (hdv_assign_slots)
    std::vector<uint8_t> upload;  // [maps.size()] 1: the map goes into its slot before the call
    int n_hdv = 0;
};

// The members with HDVs (n_hdv[m] > 0) in order, as few batches as the limits allow: a batch closes when the next member would need a
// map beyond PDMPC_HDV_MAP_SLOTS distinct ones or push the batch above PDMPC_HDV_GROUPED_MAX_VEHICLES HDVs.  same(a, b): members a and
// b hold equal maps and hulls.
template <class Same>
std::vector<HdvBatch> hdv_split_batches(int M, const int32_t* n_hdv, Same&& same) {
    std::vector<HdvBatch> out;
    for (int m = 0; m < M; ++m) {
        if (n_hdv[m] <= 0) continue;
        for (int attempt = 0;; ++attempt) {
            if (out.empty() || attempt) out.emplace_back();
            HdvBatch& B = out.back();
            int d = 0;
            while (d < (int)B.maps.size() && !same(B.maps[(size_t)d], m)) ++d;
            const bool fits = B.n_hdv + n_hdv[m] <= PDMPC_HDV_GROUPED_MAX_VEHICLES && d < PDMPC_HDV_MAP_SLOTS;
            if (!fits && !B.members.empty()) continue;  // (into a fresh batch, which takes any member: the call itself refuses one too large)
            if (d == (int)B.maps.size()) B.maps.push_back(m);
            B.members.push_back(m);
            B.map_of.push_back(d);
            B.n_hdv += n_hdv[m];
            break;
        }
    }
    return out;
}

// The slots of a batch's maps on a handle whose slots have the generations generation[PDMPC_HDV_MAP_SLOTS] now.  A map stays where it
// is: in the slot a member of it noted, if the slot's generation has not moved since (no check); else in any slot that holds it
// (holds(slot, member): the byte-for-byte check against the handle's copy).  The maps that are nowhere take the free slots in member
// order and are uploaded: slots never uploaded to from slot 0 up, then slots that hold another map from the last slot down.  Returns
// the number of content checks made.
template <class Holds>
int hdv_assign_slots(HdvBatch& B, const HdvSlotNote* note, const int64_t* generation, Holds&& holds) {
    const size_t D = B.maps.size();
    bool taken[PDMPC_HDV_MAP_SLOTS] = {};
    int checks = 0;
    B.slot.assign(D, -1);
    B.upload.assign(D, 0);
    for (size_t i = 0; i < B.members.size(); ++i) {
        const HdvSlotNote& N = note[B.members[i]];
        int32_t& slot = B.slot[(size_t)B.map_of[i]];
        if (slot >= 0 || N.slot < 0 || N.slot >= PDMPC_HDV_MAP_SLOTS || taken[N.slot] || N.generation == 0 || generation[N.slot] != N.generation) continue;
        slot = N.slot;
        taken[slot] = true;
    }
    for (size_t d = 0; d < D; ++d)
        for (int s = 0; B.slot[d] < 0 && s < PDMPC_HDV_MAP_SLOTS; ++s) {
            if (taken[s] || generation[s] == 0) continue;
            ++checks;
            if (holds(s, B.maps[d])) {
                B.slot[d] = s;
                taken[s] = true;
            }
        }
    for (size_t d = 0; d < D; ++d)  // slots never uploaded to, from slot 0 up
        for (int s = 0; B.slot[d] < 0 && s < PDMPC_HDV_MAP_SLOTS; ++s) {
            if (taken[s] || generation[s] != 0) continue;
            B.slot[d] = s;
            B.upload[d] = 1;
            taken[s] = true;
        }
    for (size_t d = 0; d < D; ++d)  // ... then over another map, from the last slot down: slot 0, which pdmpc_hdv_traffic reads, goes last
        for (int s = PDMPC_HDV_MAP_SLOTS - 1; B.slot[d] < 0 && s >= 0; --s) {
            if (taken[s]) continue;
            B.slot[d] = s;
            B.upload[d] = 1;
            taken[s] = true;
        }
    return checks;
}
