// group_route.hpp — how a group splits a time step and where its records are afterwards (pdmpc_group_*, include/pdmpc.h).
// Host only: no HIP header, no handle, no device — group.cpp packs, launches and exchanges by what this header decides, and
// pdmpc_group_partition / pdmpc_group_route_host expose it without a device.  `make host-parts` compiles it alone with the host compiler.
//
//   the partition   which rank plans which slot (the twin of pdmpc.distributed's partition_components / hybrid_partition /
//                   level_partition);
//   the route       which rank HOLDS which slot's record after the launches, and at which position: a rank keeps the records of its
//                   whole components in its handle's record buffer, in the order of its part.  The records of the component planned
//                   by levels pass through every rank during the level exchange; the copy that outlives the whole components'
//                   launches is rank 0's, so rank 0 holds them, behind its own.  Every slot has exactly one holder.
//   what follows    the seeds of a sub-problem (routed with its slots), the caller's order of lean entries, and the lists of a
//                   pdmpc_choice with slots replaced by entry indices of the gathered blocks.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/pdmpc.h"
#include "coupling_order.hpp"

struct GroupPartition {
    std::vector<std::vector<int>> parts;  // per device: the slots (caller's indices) of its whole components, in level order
    std::vector<int> shared;              // slots of the component planned by levels over all devices, in LEVEL ORDER
    std::vector<int> level_sizes;         // ... and its computation levels
    std::vector<int> level_of;            // [n] computation level (1-based) within the whole problem's coupling DAG
};

// union-find over the predecessor lists: component label per slot = smallest slot of the component (distributed.weak_components)
inline std::vector<int> weak_components(int n, const int32_t* off, const int32_t* idx) {
    std::vector<int> parent((size_t)n);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int a) {
        while (parent[(size_t)a] != a) {
            parent[(size_t)a] = parent[(size_t)parent[(size_t)a]];
            a = parent[(size_t)a];
        }
        return a;
    };
    if (off)
        for (int s = 0; s < n; ++s)
            for (int q = off[s]; q < off[s + 1]; ++q) {
                const int p = idx[q];
                if (p < 0 || p >= n) continue;
                const int ra = find(s), rb = find(p);
                if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);
            }
    std::vector<int> label((size_t)n);
    for (int s = 0; s < n; ++s) label[(size_t)s] = find(s);
    return label;
}

// PDMPC_OK, or PDMPC_ERR_INVALID with `err` set
inline int make_partition(int n, const int32_t* off, const int32_t* idx, const double* weights, int world, int mode, GroupPartition& P, std::string& err) {
    P.parts.assign((size_t)world, {});
    P.shared.clear();
    P.level_sizes.clear();
    // (without predecessor lists the weights only balance the devices: every slot is its own component, in the caller's order)
    CouplingOrder order;
    if (order.build(n, off, idx, off ? weights : nullptr) != CouplingOrder::kOk) {
        err = "the sequential coupling graph has a cycle";
        return PDMPC_ERR_INVALID;
    }
    P.level_of = order.level;
    const std::vector<int> label = weak_components(n, off, idx);
    std::vector<int> comp_ids;  // labels in ascending order
    std::vector<std::vector<int>> comp((size_t)n);
    for (int s = 0; s < n; ++s) {
        if (comp[(size_t)label[(size_t)s]].empty()) comp_ids.push_back(label[(size_t)s]);
        comp[(size_t)label[(size_t)s]].push_back(s);
    }
    std::sort(comp_ids.begin(), comp_ids.end());
    auto weight = [&](int c) {
        double w = 0;
        for (int s : comp[(size_t)c]) w += weights ? weights[s] : 1.0;
        return w;
    };
    int heavy = -1;
    if (mode == PDMPC_SHARD_LEVELS) {
        for (int s = 0; s < n; ++s) P.shared.push_back(s);
        comp_ids.clear();
    } else if (mode == PDMPC_SHARD_AUTO && world > 1 && !comp_ids.empty()) {
        // distributed.hybrid_partition: the heaviest component (ties: the smaller label) is shared if it outweighs the mean load per device
        double total = 0, wh = -1;
        for (int c : comp_ids) {
            const double w = weight(c);
            total += w;
            if (w > wh) {
                wh = w;
                heavy = c;
            }
        }
        if ((int)comp[(size_t)heavy].size() >= 2 * world && wh > total / world) {
            P.shared = comp[(size_t)heavy];
            comp_ids.erase(std::find(comp_ids.begin(), comp_ids.end(), heavy));
        }
    }
    // whole components: longest processing time first (ties: the smaller label), each to the least loaded device (ties: the lower rank)
    std::stable_sort(comp_ids.begin(), comp_ids.end(), [&](int a, int b) { return weight(a) > weight(b); });
    std::vector<double> load((size_t)world, 0.0);
    for (int c : comp_ids) {
        int r = 0;
        for (int q = 1; q < world; ++q)
            if (load[(size_t)q] < load[(size_t)r]) r = q;
        for (int s : comp[(size_t)c]) P.parts[(size_t)r].push_back(s);
        load[(size_t)r] += weight(c);
    }
    // a device's slots in a topological order of the coupling DAG: the sub-problem handed to pdmpc_pack_step then has its
    // predecessors in lower slots whatever order the caller's slots are in, so the handle does not permute it and the device-resident
    // record path (pdmpc_export_results_async) applies; group_fetch scatters back through these lists.  Without weights that is
    // level order (ascending caller index within a level); with weights, PRIORITY order (coupling_order.hpp: the packer does the same
    // for a single handle, pdmpc_set_step_weights): a device with more searches than CUs starts its heavy searches with the launch,
    // not behind the searches that wait.
    for (auto& p : P.parts) {
        std::sort(p.begin(), p.end());
        order.sort(p);
    }
    // the shared component in level order (levels by longest path, ascending vehicle index within a level: find(levels == i))
    if (!P.shared.empty()) {
        std::stable_sort(P.shared.begin(), P.shared.end(), [&](int a, int b) { return P.level_of[(size_t)a] < P.level_of[(size_t)b]; });
        int cur = -1;
        for (int s : P.shared) {
            if (P.level_of[(size_t)s] != cur) {
                cur = P.level_of[(size_t)s];
                P.level_sizes.push_back(0);
            }
            P.level_sizes.back() += 1;
        }
    }
    return PDMPC_OK;
}

// Which rank holds which slot's record, and where.  A rank's block of an exchange is a header and `per` entries (group_choice.h), so
// the entry of slot v in the gathered blocks has index rank[v] * (per + 1) + 1 + pos[v].
struct GroupRoute {
    std::vector<int32_t> rank, pos;  // [n]
    std::vector<int32_t> held;       // [world] records a rank holds
    int32_t per = 1;                 // entries per block: the largest held[], at least 1
    int n() const { return (int)rank.size(); }
    int32_t entry(int v) const { return rank[(size_t)v] * (per + 1) + 1 + pos[(size_t)v]; }
};

// ... after the launches of a partitioned step
inline void route_partition(const GroupPartition& P, int n, GroupRoute& R) {
    const size_t world = P.parts.size();
    R.rank.assign((size_t)n, -1);
    R.pos.assign((size_t)n, -1);
    R.held.assign(world, 0);
    for (size_t r = 0; r < world; ++r) {
        for (size_t i = 0; i < P.parts[r].size(); ++i) {
            R.rank[(size_t)P.parts[r][i]] = (int32_t)r;
            R.pos[(size_t)P.parts[r][i]] = (int32_t)i;
        }
        R.held[r] = (int32_t)P.parts[r].size();
    }
    for (size_t i = 0; i < P.shared.size(); ++i) {
        R.rank[(size_t)P.shared[i]] = 0;
        R.pos[(size_t)P.shared[i]] = R.held[0] + (int32_t)i;
    }
    R.held[0] += (int32_t)P.shared.size();
    R.per = std::max<int32_t>(1, *std::max_element(R.held.begin(), R.held.end()));
}

// ... of records placed by hand (pdmpc_group_debug_choose): record v on rank rank_of[v], a rank's records in ascending v; a record
// with rank_of[v] == -1 is on every rank, as a record of the shared component is, and rank 0 holds it behind its own.
// False: a rank outside [-1, world).
inline bool route_placed(int n, const int32_t* rank_of, int world, GroupRoute& R) {
    R.rank.assign((size_t)n, -1);
    R.pos.assign((size_t)n, -1);
    R.held.assign((size_t)world, 0);
    for (int v = 0; v < n; ++v) {
        if (rank_of[v] < -1 || rank_of[v] >= world) return false;
        if (rank_of[v] < 0) continue;
        R.rank[(size_t)v] = rank_of[v];
        R.pos[(size_t)v] = R.held[(size_t)rank_of[v]]++;
    }
    for (int v = 0; v < n; ++v)
        if (rank_of[v] < 0) {
            R.rank[(size_t)v] = 0;
            R.pos[(size_t)v] = R.held[0]++;
        }
    R.per = std::max<int32_t>(1, *std::max_element(R.held.begin(), R.held.end()));
    return true;
}

// the seeds of the sub-problem made of `slots` (the caller's seeds travel with the slots)
inline std::vector<uint32_t> route_seeds(const std::vector<int>& slots, const std::vector<uint32_t>& seeds) {
    std::vector<uint32_t> sub;
    sub.reserve(slots.size());
    for (int s : slots) sub.push_back(seeds[(size_t)s]);
    return sub;
}

// `count` slots of a pdmpc_choice list as entry indices of the gathered blocks
inline void route_slots(const GroupRoute& R, const int32_t* slot, int count, int32_t* entry) {
    for (int q = 0; q < count; ++q) entry[q] = R.entry(slot[q]);
}
