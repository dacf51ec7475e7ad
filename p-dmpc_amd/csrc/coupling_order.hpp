// coupling_order.hpp — the slot order of a step's coupling DAG, once: the packer (pack.cpp, a single handle's batch) and
// make_partition (group.cpp, every device's sub-problem) fill slots by it.  Host only, no HIP.
//
// A search spins for predecessors of the same launch, so every predecessor must sit in a lower slot than its successors (api.cpp,
// launch_range: forward progress of oversubscribed launches).  Without weights the order is level order — computation levels by
// longest path (kahn.m: a vehicle's level = 1 + the highest level among its predecessors), the caller's order within a level.
// With an expected work per vehicle (pdmpc_set_step_weights) it is PRIORITY order: the largest expected work among a vehicle and its
// descendants, descending; ties by level, then by the caller's index.  A predecessor's priority is at least its successors' and its
// level is lower, so that is a topological order too.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct CouplingOrder {
    enum Status { kOk, kSelfEdge, kCycle };
    std::vector<int32_t> level;  // [n] computation level, 1-based
    std::vector<double> prio;    // [n] inherited priority; empty without weights: level order

    // The DAG as CSR predecessor lists (off may be null: no edges); entries outside [0, n) are predecessors outside the batch and
    // ignored.  weights (may be null) are the caller's, one per vehicle: anything but a positive number counts as 0.
    Status build(int n, const int32_t* off, const int32_t* idx, const double* weights) {
        level.assign((size_t)n, 0);
        prio.clear();
        std::vector<int32_t> indeg((size_t)n, 0), succ_off((size_t)n + 1, 0), succ, queue;
        auto each_edge = [&](auto&& f) {  // f(vehicle, predecessor inside the batch)
            if (off)
                for (int i = 0; i < n; ++i)
                    for (int q = off[i]; q < off[i + 1]; ++q)
                        if (idx[q] >= 0 && idx[q] < n) f(i, idx[q]);
        };
        bool self_edge = false;
        each_edge([&](int i, int p) {
            self_edge = self_edge || p == i;
            succ_off[(size_t)p + 1] += 1;
            indeg[(size_t)i] += 1;
        });
        if (self_edge) return kSelfEdge;
        for (int i = 0; i < n; ++i) succ_off[(size_t)i + 1] += succ_off[(size_t)i];
        succ.resize((size_t)succ_off[(size_t)n]);
        std::vector<int32_t> fill(succ_off.begin(), succ_off.end() - 1);
        each_edge([&](int i, int p) { succ[(size_t)fill[(size_t)p]++] = i; });
        for (int i = 0; i < n; ++i)
            if (indeg[(size_t)i] == 0) {
                level[(size_t)i] = 1;
                queue.push_back(i);
            }
        for (size_t qi = 0; qi < queue.size(); ++qi) {
            const int u = queue[qi];
            for (int q = succ_off[(size_t)u]; q < succ_off[(size_t)u + 1]; ++q) {
                const int w = succ[(size_t)q];
                level[(size_t)w] = std::max(level[(size_t)w], level[(size_t)u] + 1);
                if (--indeg[(size_t)w] == 0) queue.push_back(w);
            }
        }
        if ((int)queue.size() != n) return kCycle;
        if (weights) {
            prio.resize((size_t)n);
            for (int i = 0; i < n; ++i) prio[(size_t)i] = (weights[i] == weights[i] && weights[i] > 0) ? weights[i] : 0.0;
            for (size_t qi = queue.size(); qi-- > 0;) {  // (reverse topological order: a vehicle after all its successors)
                const int u = queue[qi];
                for (int q = succ_off[(size_t)u]; q < succ_off[(size_t)u + 1]; ++q) prio[(size_t)u] = std::max(prio[(size_t)u], prio[(size_t)succ[(size_t)q]]);
            }
        }
        return kOk;
    }

    // vehicles (ascending indices on entry) into slot order
    void sort(std::vector<int32_t>& vehicles) const {
        std::stable_sort(vehicles.begin(), vehicles.end(), [&](int32_t x, int32_t y) {
            if (!prio.empty() && prio[(size_t)x] != prio[(size_t)y]) return prio[(size_t)x] > prio[(size_t)y];
            return level[(size_t)x] < level[(size_t)y];
        });
    }
};
