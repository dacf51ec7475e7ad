// reference_tree.hpp — a frontier kernel's raw arena read as the reference's tree: the reconstruction behind pdmpc_debug_tree and
// pdmpc_debug_pop_trace, as a function of plain arrays.  Host only: no HIP header, no handle, no device — api.cpp copies the records, keys,
// validity bytes, the result record and (replayed) the pop sequence from the device, then calls in here.  `make host-parts` compiles this
// header alone with the host compiler; tests/host_only_checks.cpp checks it against a literal best-first search.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "pdmpc_device.h"

// the column arrays of pdmpc_debug_tree / pdmpc_debug_raw_tree (a null column is not written)
struct TreeColumns {
    double *x, *y, *yaw, *g, *hh;
    int32_t *trim, *k, *parent;
    void put(size_t i, const NodeRec& r, int32_t parent_id) const {
        if (x) x[i] = r.x;
        if (y) y[i] = r.y;
        if (yaw) yaw[i] = r.yaw;
        if (g) g[i] = r.g;
        if (hh) hh[i] = r.h;
        if (parent) parent[i] = parent_id;
        if (trim) trim[i] = NODE_TRIM(r.packed);
        if (k) k[i] = NODE_K(r.packed);
    }
};

struct RefTree {
    std::vector<uint32_t> pops;      // raw indices in the reference's pop order
    std::vector<uint32_t> ref_nodes; // raw index of reference node id r (0-based position = id - 1)
    std::vector<uint32_t> ref_id;    // raw index -> reference id (0: not in the reference's tree)
};

// The frontier kernel processes open nodes in parallel, so its arena holds the reference's tree plus some nodes the
// reference never creates, in another order.  This turns it back into the reference's tree and pop sequence, on the host
// and independently of the kernel's phase B (it sorts the popped nodes instead of counting them), for the debug read-backs
// the parity tests use.  Order (bulk_search.hpp): X is popped before Y iff X is an ancestor of Y or the largest key on
// the path (LCA, X] is smaller than the largest key on (LCA, Y].
//
// R, key, vs: the raw_n records of the arena with their keys and validity bytes; status: of the search's result record; replayed_pops: null, or
// (a search that ended on the replay through the binary heap) the record's n_popped pops in arena indices.  What the loops below assume of an
// arena is checked first — a node's parent was created before it and lies one step above it, within the horizon; a replayed pop is a node of
// the arena —: an arena that breaks it is refused with PDMPC_ERR_INVALID and the node's index in err, nothing is indexed with it.
inline int reconstruct_reference_tree(const NodeRec* R, uint32_t raw_n, const double* key, const uint8_t* vs, int Hp, int32_t status, const std::vector<uint32_t>* replayed_pops,
                                      RefTree& T, std::string& err) {
    auto depth = [&](uint32_t i) { return NODE_K(R[i].packed); };
    auto refuse = [&err](const std::string& msg) {
        err = "reference tree: " + msg;
        return (int)PDMPC_ERR_INVALID;
    };
    if (raw_n == 0) return refuse("the arena holds no node");
    if (R[0].parent != 0) return refuse("node 0 (the root) has parent " + std::to_string(R[0].parent));
    for (uint32_t i = 1; i < raw_n; ++i) {
        if (R[i].parent < 1 || R[i].parent > i) return refuse("node " + std::to_string(i) + " has parent " + std::to_string(R[i].parent) + ", not one of 1 .. " + std::to_string(i));
        if (depth(i) != depth(R[i].parent - 1) + 1 || depth(i) > Hp)
            return refuse("node " + std::to_string(i) + " is at step " + std::to_string(depth(i)) + ", its parent at step " + std::to_string(depth(R[i].parent - 1)) + " (Hp " + std::to_string(Hp) + ")");
    }
    for (size_t q = 0; replayed_pops && q < replayed_pops->size(); ++q)
        if ((*replayed_pops)[q] >= raw_n) return refuse("replayed pop " + std::to_string(q) + " is node " + std::to_string((*replayed_pops)[q]) + " of " + std::to_string(raw_n));
    std::vector<uint8_t> alive(raw_n, 0);
    alive[0] = 1;
    for (uint32_t i = 1; i < raw_n; ++i) {
        const uint32_t p = R[i].parent - 1;
        alive[i] = alive[p] && vs[p] == 1;
    }
    // -1: x first, +1: y first, 0: same node
    auto before = [&](uint32_t x, uint32_t y) -> int {
        if (x == y) return 0;
        double mx = -1.0, my = -1.0;
        uint32_t a = x, b = y;
        while (depth(a) > depth(b)) {
            mx = std::max(mx, key[a]);
            a = R[a].parent - 1;
        }
        while (depth(b) > depth(a)) {
            my = std::max(my, key[b]);
            b = R[b].parent - 1;
        }
        if (a == b) return depth(x) < depth(y) ? -1 : 1;  // ancestor first
        while (a != b) {
            mx = std::max(mx, key[a]);
            my = std::max(my, key[b]);
            a = R[a].parent - 1;
            b = R[b].parent - 1;
        }
        return mx < my ? -1 : 1;
    };
    // the goal: the first collision-free node at the horizon
    int64_t goal = -1;
    if (status == PDMPC_OK)
        for (uint32_t i = 0; i < raw_n; ++i)
            if (alive[i] && vs[i] == 1 && depth(i) == Hp && (goal < 0 || before(i, (uint32_t)goal) < 0)) goal = i;
    T.pops.clear();
    if (replayed_pops) {
        // equal keys: the order is the binary heap's, which the kernel's replay has run (bulk_search.hpp, bk_replay) and left behind
        T.pops = *replayed_pops;
    } else {
        for (uint32_t i = 0; i < raw_n; ++i)
            if (alive[i] && (goal < 0 || i == (uint32_t)goal || before(i, (uint32_t)goal) < 0)) T.pops.push_back(i);
        std::sort(T.pops.begin(), T.pops.end(), [&](uint32_t x, uint32_t y) { return before(x, y) < 0; });
    }
    // children of a node are consecutive raw indices in ascending trim order
    std::vector<uint32_t> first_child(raw_n, 0), n_child(raw_n, 0);
    for (uint32_t i = raw_n; i-- > 1;) {
        const uint32_t p = R[i].parent - 1;
        first_child[p] = i;
        n_child[p] += 1;
    }
    T.ref_id.assign(raw_n, 0);
    T.ref_nodes.clear();
    T.ref_nodes.push_back(0);
    T.ref_id[0] = 1;
    for (uint32_t x : T.pops) {
        if (vs[x] != 1 || depth(x) == Hp) continue;  // discarded (GraphSearch.m:75-77) or the goal
        for (uint32_t c = 0; c < n_child[x]; ++c) {
            T.ref_nodes.push_back(first_child[x] + c);
            T.ref_id[first_child[x] + c] = (uint32_t)T.ref_nodes.size();
        }
    }
    return PDMPC_OK;
}
