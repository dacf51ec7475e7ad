// launch_plan.hpp — the plan of a launch: everything that decides how a search, a sampled or a joint launch goes out, as functions of a
// dozen integers (LaunchDims), the tuning string and the constants of pdmpc_device.h.  Host only: no HIP header, no handle, no device —
// api.cpp gathers the dimensions, calls plan_launch and copies the plan into the kernel's arguments; pdmpc_launch_plan_host (include/pdmpc.h)
// shows the same plan to a test on a CPU.  `make host-parts` compiles this header alone with the host compiler.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "pdmpc_device.h"
#include "sampled_budget.h"
#include "sampled_ensemble.h"

// Tuning knobs and A/B / test switches of the graph search.  The defaults are the measured optima quoted next to their use; every
// setting leaves the results bit-identical.  ONE environment variable overrides them, read once in pdmpc_create (a launch makes no
// getenv call):  PDMPC_TUNING="key=value,key=value,..."  with the keys below (include/pdmpc.h documents the variable).
struct Tuning {
    int round0 = -1;        // nodes a round of a young search takes (-1: 24; 32 for a launch that leaves CUs idle but has fewer than four helpers per search, C3, and for one of more than two searches per CU, C5)
    int round = -1;         // the most a round takes (-1: 1000 with helper workgroups, else 256)
    int ramp = -1;          // a round grows by 1 / ramp of the nodes processed so far (-1: 2 with helper workgroups, else 4)
    int ready = 2048;       // entries of the ready list with helper workgroups (half of it without): the most a round can take
    int share_min = -1;     // a round with at least this many nodes is shared with the helper workgroups (-1: by the number of helpers per search, launch_policy)
    int tile = -1;          // the most nodes of a shared round one seated helper takes (-1: 256; what it stages in LDS: at most 768)
    int mid_min = 24576;    // far lists longer than this feed near through the mid list (a band of far's smallest keys)
    int mid_fill = 12288;   // entries a refill of mid aims at
    int tentative = 1;      // expected areas of predecessors that are still planning (A/B switch)
    int fast_arrival = 1;   // finished searches check arrivals against their plan's path first and publish early (A/B switch)
    int helpers = -1;       // helper workgroups of a launch with at most one search per CU (-1: by launch size, 0: none)
    int helpers_oversub = -1;  // ... of a launch with more searches than CUs (-1: 200)
    int seat_nodes = 256;   // a search may hold its share of the launch's helpers (helpers / searches) per this many nodes it has processed
    int helpers_first = -1; // ... of them dispatched in front of the searches (-1: half the CUs when most searches of the launch have predecessors)
    int speculate = 1;      // 0: every search waits for all its predecessors before it starts
    int compact = -1;       // 1: the kernel built for two workgroups per CU (8 wavefronts, <= 80 KB of LDS: bulk_kernel_compact.hip) where it applies (InterX, one mask word, the soup fits); 0: never; -1: for launches of more than two searches per CU
    int waves = -1;         // wavefronts per workgroup (4 .. PDMPC_MAX_WAVES; -1: 16 for the InterX kernels — 12 for a launch of more than two searches per CU —, 12 for the separating-axis kernel)
    uint32_t spin_limit = 1u << 22;  // the watchdog's limit of polls / rounds (debugging: fail fast)
    int force_tie = 0;      // testing only: every search ends on the replay through the reference's binary heap (as if it had met equal keys)
    int reverse_dispatch = 0;  // testing only: workgroup b takes slot n - 1 - b (successors dispatched before their predecessors)
    int debug_tail = 0;     // round / node / tick counters of every search in the unused rows of its record's path_nodes (tools/fr_step_profile.py)
    int debug_lds = 0;      // print the LDS layout of every launch
    int debug_host = 0;     // 1: a line per launch; 2: the host-time breakdown of the literal path
    int debug_progress = 0; // live counters in host-mapped memory (pdmpc_debug_progress)
    int generic = 0;        // 1: every search launch runs the generic instantiation of its kernel, which reads all switches from KernelArgs (A/B and tests; pdmpc_device.h: ProductSwitches)
};

// parses PDMPC_TUNING; an unknown key or a malformed entry is an error (a typo must not silently measure the default)
inline bool parse_tuning(const char* text, Tuning& T, std::string& err) {
    struct Key { const char* name; int* dst; };
    int spin = (int)T.spin_limit;
    const Key keys[] = {{"round0", &T.round0}, {"round", &T.round}, {"ramp", &T.ramp}, {"ready", &T.ready}, {"share_min", &T.share_min},
                        {"tile", &T.tile}, {"mid_min", &T.mid_min}, {"mid_fill", &T.mid_fill}, {"tentative", &T.tentative}, {"fast_arrival", &T.fast_arrival}, {"helpers_first", &T.helpers_first}, {"seat_nodes", &T.seat_nodes},
                        {"helpers", &T.helpers}, {"helpers_oversub", &T.helpers_oversub}, {"speculate", &T.speculate}, {"waves", &T.waves}, {"compact", &T.compact}, {"spin_limit", &spin},
                        {"force_tie", &T.force_tie}, {"reverse_dispatch", &T.reverse_dispatch}, {"debug_tail", &T.debug_tail}, {"debug_lds", &T.debug_lds},
                        {"debug_host", &T.debug_host}, {"debug_progress", &T.debug_progress}, {"generic", &T.generic}};
    std::string str(text ? text : "");
    size_t pos = 0;
    while (pos < str.size()) {
        size_t end = str.find(',', pos);
        if (end == std::string::npos) end = str.size();
        const std::string item = str.substr(pos, end - pos);
        pos = end + 1;
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos || eq == 0 || eq + 1 >= item.size()) {
            err = "PDMPC_TUNING: '" + item + "' is not key=value";
            return false;
        }
        const std::string name = item.substr(0, eq);
        char* tail = nullptr;
        const long v = strtol(item.c_str() + eq + 1, &tail, 10);
        if (!tail || *tail) {
            err = "PDMPC_TUNING: value of '" + name + "' is not an integer";
            return false;
        }
        bool found = false;
        for (const Key& k : keys)
            if (name == k.name) {
                *k.dst = (int)v;
                found = true;
            }
        if (!found) {
            err = "PDMPC_TUNING: unknown key '" + name + "'";
            return false;
        }
    }
    if (T.compact < -1 || T.compact > 1) {
        err = "PDMPC_TUNING: compact takes -1, 0 or 1";
        return false;
    }
    if (T.round0 >= 0) T.round0 = std::max(1, T.round0);
    if (T.round >= 0) T.round = std::max(1, T.round);
    if (T.ramp >= 0) T.ramp = std::max(1, T.ramp);
    T.ready = std::min(2048, std::max(256, T.ready)) & ~63;
    if (T.share_min >= 0) T.share_min = std::max(32, T.share_min);
    if (T.tile >= 0) T.tile = std::min(768, std::max(8, T.tile));
    T.mid_min = std::max(0, T.mid_min);
    T.mid_fill = std::max(256, T.mid_fill);
    if (T.waves >= 0) T.waves = std::min(PDMPC_MAX_WAVES, std::max(4, T.waves));
    T.spin_limit = (uint32_t)std::max(1024, spin);
    return true;
}

// What planning reads of a handle (the configuration, the uploaded automaton's sizes, the device, the arena) and of the packed bank
// (api.cpp fills it in this order).
struct LaunchDims {
    int checker = PDMPC_CHECK_INTERX, Hp = 0;
    int n_trims = 0, n_words = 0, n_man = 0;  // the automaton: trims, 64-bit words of a successor mask, maneuvers
    size_t mask_bytes = 0, mi_bytes = 0;      // its successor masks and maneuver index (mpa_table_sizes)
    int n_cu = 256, device_share = 1;
    uint32_t max_nodes = 0;  // the arena's
    bool sampled = false;    // the bank: packed with seeds; soup columns (a joint launch: pdmpc_joint_soup_columns + 2), boundary columns,
    int soup_cap = 0, ll_cap = 0, cand_cap = 0;  // ... segments of one edge check
};

// the sizes of the automaton's tables from (n_trims, Hp): what pdmpc_upload_mpa uploads and every layout reserves
inline void mpa_table_sizes(LaunchDims& d) {
    d.n_words = (d.n_trims + 63) / 64;
    d.mask_bytes = (size_t)d.Hp * d.n_trims * d.n_words * 8;
    d.mi_bytes = (size_t)d.n_trims * d.n_trims * 2;
}

enum PlanKind : int32_t { kPlanSearch = 0, kPlanSampled = 1, kPlanJoint = 2 };  // pdmpc_launch_query::kind

// The LDS layout of a search or sampled launch (compute_lds_bulk, compute_lds_sampled).
struct LaunchLayout {
    LdsLayout lds{};
    int n_waves = 0;       // wavefronts per workgroup
    int NL = 0, NV = 0;    // node records / validity bytes in LDS
    int areas_in_lds = 0;  // the automaton's maneuver areas are in LDS (else read from L2)
    int ready = 0;         // entries of the ready list
    bool compact = false;  // the compact kernel's (two workgroups per CU)
};

// The plan of one launch (launch_range, pdmpc_plan_joint): its LDS layout, the kernel that runs it, the sizes of its rounds, its
// helper workgroups and its slices.  Computed per launch and held by it, not by the handle.
struct LaunchPlan : LaunchLayout {
    JointLds joint{};       // the joint search's regions (with n_waves and areas_in_lds) ...
    uint32_t heap_lds = 0;  // ... and the entries of its open list in LDS
    // launch_policy (KernelArgs has a field of the same name for each)
    int bk_ready_cap = 0, bk_round0 = 0, bk_round = 0, bk_ramp = 0, bk_tile = 0, bk_share_min = 0, n_helpers = 0, bk_helpers_first = 0;
    int bk_seat_nodes = 1, reverse_dispatch = 0;
    uint32_t spin_limit = 0;
    int variant = PDMPC_BULK;  // which of the four search kernels (PDMPC_BULK ...), and which of its two instantiations
    bool generic = false;
    int slice = 0;             // searches per kernel launch: all of them, or what is resident as a whole in the safe mode
    const char* kernel = "";
};

inline uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

const size_t kLdsMax = 160 * 1024;  // gfx950: 160 KiB per CU (MI355X_MICROARCH.md)

// The automaton's tables, the front of every LDS layout from `off` on: successor masks, maneuver index, poses, then the maneuver
// areas (only with `areas`: else they are read from L2).  Returns the first free byte.
template <class Layout>
uint32_t layout_mpa(const LaunchDims& d, uint32_t off, bool areas, Layout& L) {
    L.mask = off;
    off = align16(off + (uint32_t)d.mask_bytes);
    L.man_index = off;
    off = align16(off + (uint32_t)d.mi_bytes);
    L.pose = off;
    off = align16(off + (uint32_t)(d.n_man * sizeof(DevManPose)));
    L.area = off;
    if (areas) off = align16(off + (uint32_t)(d.n_man * 3 * PDMPC_VMAX * 16));
    return off;
}

// one rung of compute_lds_bulk's ladder (budget 0: not tried)
struct BulkAttempt {
    size_t budget;
    int waves, ready, areas;
    bool compact, tight;
};

// LDS layout of the graph search: MPA tables, reference, per-wave tallies, shared words, obstacle soup, phase B's chunk state (12 B per
// thread), d_traveled table, the LDS part of the open set (PDMPC_BK_PER entries per thread), the ready list with its collision
// flags, the histogram / goal list / expansion lists, 2 KB of small tables, the areas of the published path, validity bytes, then
// as many node records as fit.
inline bool layout_bulk(const LaunchDims& d, const BulkAttempt& t, LdsLayout& L, uint32_t& nv, uint32_t& nl) {
    const bool compact = t.compact, tight = t.tight;
    const uint32_t lk_waves = compact ? PDMPC_LK_COMPACT_WAVES : PDMPC_MAX_WAVES, lk_ready = compact ? PDMPC_LK_COMPACT_READY_CAP : 2048u, lk_per = compact ? PDMPC_LK_COMPACT_BK_PER : PDMPC_BK_PER;
    if ((uint32_t)t.ready > lk_ready || (uint32_t)t.waves > lk_waves) return false;
    // the regions of fixed size at the kernel's compile-time offsets (pdmpc_device.h: PDMPC_LK_*) ...
    // ... the reach lists right behind them (InterX only: the separating-axis kernels have none and keep their layout; 2 B per soup
    // column, the boundary's once per step: their address is a constant too.  tight: ONE list of the boundary, the last step's, serves
    // every step — a superset of each step's own — and fewer node records are asked for: the layout of last resort, for a soup and
    // tables that leave the LDS no room for more) ...
    L.reach = pdmpc_lk_fixed(lk_waves, lk_ready, lk_per, &L);
    L.reach_shared = tight ? 1u : 0u;
    const uint32_t list_entries = d.checker == PDMPC_CHECK_INTERX ? (uint32_t)(std::max(d.soup_cap, 1) + (tight ? 0 : (d.Hp - 1) * std::max(d.ll_cap, 0))) : 0u;
    // ... the automaton's tables and the soup behind them
    uint32_t off = layout_mpa(d, align16(L.reach + list_entries * 2), t.areas, L);
    L.soup = off;
    off = align16(off + (uint32_t)std::max(d.soup_cap, 1) * 16);
    L.tree16 = L.bk_hist;  // (the sampled optimizer's region: not part of this layout)
    // (LDS-resident node records are a cache of the arena's first NL nodes: every access takes the HBM copy for a node beyond NL
    // (node_piece, node_store), and the joint search runs the same code with NL = 0.  64 is what keeps a light search's first rounds in
    // LDS; the layout of last resort asks for 16 — the root and its children — because its alternative is PDMPC_ERR_CAPACITY)
    const uint32_t min_nodes = (tight ? 16u : 64u) * (uint32_t)sizeof(NodeRec) + 1024;
    if ((size_t)off + min_nodes + 256 > t.budget) return false;
    const uint32_t rest = (uint32_t)(t.budget - off - 256);
    nv = std::min<uint32_t>(16384u, std::max<uint32_t>(compact ? 512u : 1024u, rest / 6));
    nv = std::min(nv, d.max_nodes) & ~15u;
    nl = std::min((rest - nv) / (uint32_t)sizeof(NodeRec), d.max_nodes);
    L.vstate = off;
    off += align16(nv);
    L.nodes = off;
    off += nl * (uint32_t)sizeof(NodeRec);
    L.total = align16(off);
    return L.total <= t.budget;
}

// helper workgroups serve the launches that leave CUs idle (launch_policy)
inline bool bulk_has_helpers(const Tuning& T, int n_cu, int n_launch) {
    if (!T.speculate || T.helpers == 0) return false;
    if (n_launch > n_cu) return T.helpers_oversub != 0;  // (the tail of a launch with more searches than CUs)
    return n_launch <= n_cu - 2;
}

// The graph search's layout: the first rung of a ladder that fits — the compact layout where it applies, the full one with the maneuver
// areas in LDS, with the areas in L2 (when the soup leaves no room), the layout of last resort (layout_bulk: tight).
inline int compute_lds_bulk(const Tuning& T, const LaunchDims& d, int n_launch, LaunchPlan& out, std::string& err) {
    // large rounds pay where helper workgroups share them; without helpers the LDS is better spent on node records
    const int ready_want = bulk_has_helpers(T, d.n_cu, n_launch) ? T.ready : std::max(256, T.ready / 2);
    // Sixteen wavefronts where the kernel's registers allow four per SIMD (measured against twelve: C2 +1.5 %, C3 +1.3 %, C4 +7.5 %;
    // C5, five light searches per CU one after the other, -1.7 %: it keeps twelve and the LDS-resident nodes that go with them)
    const int cap = d.checker == PDMPC_CHECK_SAT ? PDMPC_MAX_WAVES_SAT : PDMPC_MAX_WAVES;
    // Two workgroups per CU (bulk_kernel_compact.hip: 8 wavefronts, at most half the LDS, a near list of 1 024 entries, the automaton's
    // areas in L2) for launches of more than two searches per CU — C5's class: light searches one after the other on every CU, each
    // bound by the latency of its own passes; two side by side fill each other's gaps (C5 557 -> 710 steps/s).  NOT for launches whose
    // step is one heavy search (C4, 512 searches: 94.6 -> 31 steps/s with it — half the lanes, a quarter of the near list, rounds of
    // 240 entries that are never shared).  InterX with one mask word only; falls back to the full layout if the soup does not fit.
    const bool want_compact = d.checker == PDMPC_CHECK_INTERX && d.n_words == 1 && (T.compact > 0 || (T.compact < 0 && n_launch > 2 * d.n_cu));
    const int cwaves = T.waves >= 0 ? std::min(T.waves, PDMPC_LK_COMPACT_WAVES) : PDMPC_LK_COMPACT_WAVES;
    const int waves = T.waves >= 0 ? std::min(T.waves, cap) : (n_launch > 2 * d.n_cu ? std::min(12, cap) : cap);
    const int ready = std::min(ready_want, 3 * PDMPC_WAVE * waves);
    const BulkAttempt tries[] = {{want_compact ? kLdsMax / 2 : 0, cwaves, std::min(std::min(ready_want, 3 * PDMPC_WAVE * cwaves), (int)PDMPC_LK_COMPACT_READY_CAP), 0, true, false},
                                 {kLdsMax, waves, ready, 1, false, false},
                                 {kLdsMax, waves, ready, 0, false, false},  // (the maneuver areas fall back to L2 when the soup leaves no room)
                                 {kLdsMax, waves, ready, 0, false, true}};
    for (const BulkAttempt& t : tries) {
        LdsLayout L{};
        uint32_t nv = 0, nl = 0;
        if (t.budget == 0 || !layout_bulk(d, t, L, nv, nl)) continue;
        static_cast<LaunchLayout&>(out) = {L, t.waves, (int)nl, (int)nv, t.areas, t.ready, t.compact};
        return PDMPC_OK;
    }
    char buf[256];
    snprintf(buf, sizeof buf, "obstacle soup (%d columns) + MPA tables do not fit into %zu B of LDS", d.soup_cap, kLdsMax);
    err = buf;
    return PDMPC_ERR_CAPACITY;
}

// What a sampled launch decides besides its LaunchPlan (extra[4] of pdmpc_sampled_plan_host, include/pdmpc.h): the tree's rows, where the tree
// lives, and how the random numbers are drawn.
struct SampledExtra {
    int node_cap = PDMPC_SB_DEFAULT_ROWS, tree_in_lds = 1;
    int64_t tree_hbm_bytes = 0;  // per slot (0: the tree is in LDS)
    int rand_chunk = 0;          // doubles drawn at a time
    // ... and a seed ensemble (pdmpc_set_sampled_ensemble; extra[4..7] of pdmpc_sampled_ensemble_plan_host)
    int members = 1;
    int64_t member_bytes = 0;        // member records per slot (0 for one member: the slot's record is the only one)
    int64_t ensemble_tree_bytes = 0; // HBM trees per slot, all members'
    int64_t grid = 0;                // workgroups of a kernel launch
};

// The sampled part of a packed bank: whether it was packed with seeds (its launches then run the sampled optimizer), and the expansion
// budget and ensemble size its owner had when it was packed (pdmpc_set_sampled_budget, pdmpc_set_sampled_ensemble).
struct SampledBank {
    bool on = false;
    int budget = PDMPC_SAMPLED_BUDGET_DEFAULT;
    int members = 1;
    // the reference's budget, one member: pdmpc_sampled_kernel, whose tree is always in LDS -- a bank that needs no scratch
    bool reference() const { return budget == PDMPC_SAMPLED_BUDGET_DEFAULT && members == 1; }
};

// The scratch a sampled bank of n_packed slots needs besides its batch, in elements of each buffer.  The pack grows the buffers to
// it and every launch checks them against it.
struct SampledNeed {
    size_t tree = 0;        // 16-bit words of the HBM trees: a slot's rows for every slot and member (0: the tree is in LDS)
    size_t per_member = 0;  // an ensemble's member records, entries and tree sizes, [slot * E + e] (0: one member)
    size_t per_slot = 0;    // ... and its tickets and chosen members, [slot]
};
inline SampledNeed sampled_need(const SampledBank& bank, int n_packed, const SampledExtra& extra) {
    const size_t n_members = (size_t)n_packed * (size_t)bank.members;
    SampledNeed need;
    if (!extra.tree_in_lds) need.tree = n_members * (size_t)extra.node_cap * PDMPC_SB_ROW;
    if (bank.members > 1) {
        need.per_member = n_members;
        need.per_slot = (size_t)n_packed;
    }
    return need;
}

// Seeds on their way to a pack: set by a call (pdmpc_set_step_seeds, pdmpc_group_set_step_seeds), taken by the next pack whether it
// succeeds or fails -- a pack that fails leaves no sampled bank behind it, and no seeds for the pack after it.
struct PendingSeeds {
    std::vector<uint32_t> seeds;  // one per vehicle of the next packed step, the caller's order
    bool set = false;
    void assign(const uint32_t* from, int n) {
        seeds.assign(from, from + n);
        set = true;
    }
    // the seeds into `taken`, nothing left; false: none were set, the pack is not a sampled one
    bool take(std::vector<uint32_t>& taken) {
        taken = std::move(seeds);
        seeds.clear();
        return std::exchange(set, false);
    }
};

// LDS layout of the sampled optimizer (one wavefront per vehicle; sampled_search.hpp): MPA tables, reference, the wave's two shapes,
// offsets, obstacle soup (with the predecessors' columns the packer counts into soup_cap), the candidate segments of one edge check,
// then the tree (`tree_bytes`: rows of 36 B) and the random numbers (`rand_bytes`).  80 KB first (two workgroups per CU), then the whole
// 160 KB (one); the automaton's areas go to L2 before a layout takes the larger budget.
//   pdmpc_sampled_kernel          288 rows, then the whole stream of Hp * 250 doubles (32 000 B at Hp 16); the tree's region is the
//                                 generator's state before the tree is set up.  The tree never leaves the LDS.
//   any other budget, ensembles   the generator's 624 state words, then pdmpc_sb_node_cap(budget) rows.  `hbm_allowed`: where no rung
//                                 holds the tree it goes to HBM (tree_in_lds = false) and the same ladder is walked without it.
inline int layout_sampled(const Tuning& T, const LaunchDims& d, uint32_t tree_bytes, uint32_t rand_bytes, bool hbm_allowed, LaunchPlan& out, bool& tree_in_lds, std::string& err) {
    for (int pass = 0; pass < (hbm_allowed ? 8 : 4); ++pass) {
        const int areas = (pass & 1) == 0;
        const size_t budget = (pass & 2) == 0 ? kLdsMax / 2 : kLdsMax;
        tree_in_lds = pass < 4;
        LdsLayout L{};
        uint32_t off = layout_mpa(d, 0, areas, L);
        L.ref = off;
        off += 3 * PDMPC_HP_MAX * 8;
        L.shape = off;
        off += (2 * PDMPC_VMAX + 1) * 16;
        L.path = off;
        off += PDMPC_LK_PATH_BYTES;
        L.soup = off;
        off = align16(off + (uint32_t)std::max(d.soup_cap, 1) * 16);
        L.cand = off;
        off += align16((uint32_t)std::max(d.cand_cap, 1) * 4u);
        L.expand = off;
        off += (2 * PDMPC_HP_MAX * PDMPC_HP_MAX) * 8 + 16 * 16;
        // (a tree that may leave the LDS lies behind everything else)
        if (!hbm_allowed) {
            L.tree16 = off;
            off += align16(tree_bytes);
        }
        L.rand = off;
        off += align16(rand_bytes);
        if (hbm_allowed) {
            L.tree16 = off;
            if (tree_in_lds) off += align16(tree_bytes);
        }
        L.total = align16(off);
        if (L.total <= budget) {
            static_cast<LaunchLayout&>(out) = {L, 1, 0, 0, areas, T.ready, false};  // (one wavefront, no ready list: the kernel reads none of the rounds' arguments)
            return PDMPC_OK;
        }
    }
    err = "obstacle soup + MPA tables do not fit into the LDS budget of the sampled optimizer";
    return PDMPC_ERR_CAPACITY;
}

// ... of pdmpc_sampled_kernel (plan_launch)
inline int compute_lds_sampled(const Tuning& T, const LaunchDims& d, LaunchPlan& out, std::string& err) {
    static_assert(PDMPC_SB_DEFAULT_ROWS * PDMPC_SB_ROW * 2u >= PDMPC_SB_MT_BYTES, "the tree region holds the generator's state");
    bool tree_in_lds;
    return layout_sampled(T, d, PDMPC_SB_DEFAULT_ROWS * PDMPC_SB_ROW * 2u, (uint32_t)d.Hp * PDMPC_SAMPLED_BUDGET_DEFAULT * 8u, false, out, tree_in_lds, err);
}

// LDS layout of the joint search (one wavefront per problem): MPA tables, every vehicle's reference, the node's areas, offsets and the
// path, successor lists, the problem's distinct soups (soup_cap: pdmpc_joint_soup_columns), then the LDS part of the open list.  Aimed at 64 KB (two workgroups per CU and more);
// a problem whose tables and soups do not leave room for 256 heap entries there may take up to the whole 160 KB.
inline int layout_joint(const LaunchDims& d, int soup_cap, LaunchPlan& out, std::string& err) {
    for (int pass = 0; pass < 4; ++pass) {
        const bool areas = pass == 0 || pass == 2;
        const size_t budget = pass < 2 ? 64 * 1024 : kLdsMax;
        JointLds& L = out.joint;
        uint32_t off = layout_mpa(d, 0, areas, L);
        L.ref = off;
        off += PDMPC_JOINT_MAX * 3 * PDMPC_HP_MAX * 8;
        L.shape = off;
        off += PDMPC_JOINT_MAX * 2 * PDMPC_VMAX * 16;
        L.ints = off;
        off = align16(off + PDMPC_JOINT_INTS * 4);
        L.succ = off;
        off = align16(off + (uint32_t)(PDMPC_JOINT_MAX * d.n_trims * 4));
        L.soup = off;
        off = align16(off + (uint32_t)std::max(soup_cap, 1) * 16);
        if (off + 256 * 12 > budget) continue;
        const uint32_t entries = std::min<uint32_t>(8192u, (uint32_t)((budget - off) / 12) & ~63u);
        L.heap_key = off;
        off += entries * 8;
        L.heap_id = off;
        off += entries * 4;
        L.total = align16(off);
        out.heap_lds = entries;
        out.areas_in_lds = areas ? 1 : 0;
        out.n_waves = 1;
        return PDMPC_OK;
    }
    err = "the MPA tables and a joint problem's obstacle soups do not fit into LDS";
    return PDMPC_ERR_CAPACITY;
}

// does launch_policy read n_chained?  (Where it does not, the caller need not count: launch_range walks the launch's slots for it.)
inline bool policy_reads_chained(const Tuning& T, int count, int n_cu, int device_share) {
    return count > n_cu && count <= 2 * n_cu && device_share == 1 && T.helpers_first < 0;
}

// The launch policy: the sizes of a launch's rounds, its helper workgroups and where they sit -- bk_ready_cap, bk_round0, bk_round, bk_ramp,
// bk_tile, bk_share_min, n_helpers and bk_helpers_first of the plan `p`, from its layout (ready, n_waves, compact), and nothing else of it.
// Every value it gives leaves the records bit-identical (struct Tuning), so only a benchmark sees it.  `n_chained`: how many of the
// launch's slots have predecessors (read only where the place of the helpers depends on it: policy_reads_chained).
inline void launch_policy(const Tuning& T, int count, int n_cu, int device_share, bool safe, bool search, int n_chained, LaunchPlan& p) {
    // rounds: measured on C2 / C3 (20 / 128 searches, helpers): cap 256, ramp 4 -> 646 / 589 steps/s; 512, 2 -> 735 / 786; 1000, 2 -> 769 / 909; 1000, 1 -> 620 / 772
    const bool helped = search && !safe && bulk_has_helpers(T, n_cu, count);
    p.bk_ready_cap = std::min(p.ready, 3 * PDMPC_WAVE * p.n_waves);  // (the verdict pass handles three entries per thread)
    p.bk_round0 = T.round0 > 0 ? T.round0 : 24;  // (C3's class: below, once the helpers are counted)
    p.bk_round = std::min(p.ready / 2 - 16, std::max(p.bk_round0, T.round > 0 ? T.round : (helped ? 1000 : 256)));
    p.bk_ramp = T.ramp > 0 ? T.ramp : (helped ? 2 : 4);
    p.bk_tile = T.tile > 0 ? T.tile : 256;
    if (p.compact) p.bk_tile = std::min(p.bk_tile, 256);  // (a helper stages its range in the near list's room: 12 KB in the compact layout)
    // Helper workgroups: the trailing workgroups of the launch, on the CUs it leaves idle, check tiles of the searches' large rounds.
    // A launch with more searches than CUs gets them for its tail, when CUs fall idle while a few long searches still run (measured on
    // C4, 512 searches: none 25.6 steps/s, 32 helpers 41.5, 96: 42.8-45.9; C5, 1 280 searches: none 478 steps/s, 64 behind the searches 543,
    // 200: 549, with rounds shared from 64 nodes on 560 — the last levels' searches, which run when the CUs fall idle, are the tail of
    // the step).  In the safe mode a launch gets none: they would sit where a slice's search could run.
    p.n_helpers = 0;
    if (helped) {
        if (count <= n_cu) {
            // every CU the launch leaves idle: a seated helper polls a word of its own, so helpers cost the searches nothing (measured on
            // C2, 20 searches: 32 helpers 1 110 steps/s, 64: 1 120, 96: 1 190, 128: 1 200, 200: 1 210, 230: 1 235; with the ticket word of
            // rounds 3-4 that all helpers polled and claimed from, 64 helpers were slower than 32 and 200 cost 40 %)
            int want = n_cu - count;
            if (T.helpers >= 0) want = T.helpers;
            p.n_helpers = std::max(0, std::min(want, n_cu - count));
            if (p.n_helpers < 2) p.n_helpers = 0;
        } else {
            p.n_helpers = 200;  // (seated helpers cost the searches nothing: measured on C4 96 -> 76.9 steps/s, 160-250 -> 77.7)
            if (T.helpers_oversub >= 0) p.n_helpers = std::min(T.helpers_oversub, 3 * n_cu);
            if (T.helpers >= 0) p.n_helpers = std::min(p.n_helpers, T.helpers);
        }
    }
    // ... and where do they sit?  Behind the searches they get the CUs the searches leave.  In a launch of more searches than CUs whose
    // searches wait for one another, finished searches hold their CUs until their predecessors are through, and the helpers behind them
    // start when the step is half over (C4: a helper lived 5-6 of the step's 11 ms, and the step's 10^5-node search ran most of its
    // rounds with fewer than eight seats).  Half the CUs' worth of helpers in front of the searches: C4 82.8 -> 90.2 steps/s (32: 84.2,
    // 64: 86.5, 128: 90.2, 160: 88.0, 200: 54.6).  A launch of independent searches keeps every CU for them.
    // (handles that share a device — the logical ranks of a group — launch side by side: the idle CUs are the device's, not the
    // launch's, and helper workgroups in FRONT of every launch's searches would fill the chip before any search starts)
    if (device_share > 1) p.n_helpers = p.n_helpers / device_share >= 2 ? p.n_helpers / device_share : 0;
    p.bk_helpers_first = 0;
    if (count > n_cu && p.n_helpers > 0 && device_share == 1) {
        int want = T.helpers_first;
        if (want < 0 && count > 2 * n_cu) want = 0;  // (five searches per CU, C5: the searches need every CU — 128 in front 331 steps/s, 32: 515, none: 560)
        if (want < 0) want = 2 * n_chained >= count ? n_cu / 2 : 0;
        p.bk_helpers_first = std::max(0, std::min(want, p.n_helpers));
    }
    // rounds are shared from 64 nodes on where helpers are plenty (C2: a dozen per search), from a few hundred on where there are
    // about as many helpers as searches or fewer (measured C3, 128 + 128: 64 -> 1 026 steps/s, 128-192 -> 1 070, 384 -> 986; C4, 512 + 96:
    // 64 -> 65.5, 192 -> 67, 512 -> 69; C5, 1 280 + 200 behind the searches, whose helpers only meet the medium searches of the tail: 32-128 -> 560)
    p.bk_share_min = T.share_min > 0 ? T.share_min : (p.n_helpers >= 4 * count ? 64 : (count <= n_cu ? 128 : (count <= 2 * n_cu ? 512 : 64)));
    // (sixteen wavefronts: C3 — 128 searches + 128 helpers — 1 135 steps/s with young rounds of 24 nodes and sharing from 160 on, 1 175 with 32
    // and 128; 28: 1 154, 36: 1 137.  C2 / C4 / C5 with 32: -0.6 % / -1 % / +0.6 %: they stay at 24)
    if (T.round0 < 0 && helped && ((count <= n_cu && p.n_helpers < 4 * count) || count > 2 * n_cu)) {  // (C5, 1 280 searches: 558 -> 565)
        p.bk_round0 = 32;
        p.bk_round = std::max(p.bk_round, p.bk_round0);
    }
}

// What a search launch reads of its plan and of the tuning's switches: every KernelArgs field that is a decision, none that
// is a pointer or a counter of its owner.
inline void set_plan_args(const Tuning& T, const LaunchPlan& p, KernelArgs& a) {
    a.areas_in_lds = p.areas_in_lds;
    a.lds = p.lds;
    a.NL = p.NL;
    a.NV = p.NV;
    a.n_waves = p.n_waves;
    a.n_helpers = p.n_helpers;
    a.bk_ready_cap = p.bk_ready_cap;
    a.bk_round0 = p.bk_round0;
    a.bk_round = p.bk_round;
    a.bk_ramp = p.bk_ramp;
    a.bk_helpers_first = p.bk_helpers_first;
    a.bk_seat_nodes = p.bk_seat_nodes;
    a.bk_tile = p.bk_tile;
    a.bk_share_min = p.bk_share_min;
    a.spin_limit = p.spin_limit;
    a.reverse_dispatch = p.reverse_dispatch;
    a.debug_tail = T.debug_tail;
    a.speculate = T.speculate;
    a.bk_mid_min = T.mid_min;
    a.bk_mid_fill = T.mid_fill;
    a.bk_tentative = T.tentative;
    a.bk_fast_arrival = T.fast_arrival;
    a.bk_force_tie = T.force_tie;
}

// the search kernels by (variant, generic), the sampled optimizer's, the joint search's
const char* const kBulkKernelNames[4][2] = {{"pdmpc_bulk_kernel", "pdmpc_bulk_kernel_any"},
                                            {"pdmpc_bulk_kernel_wide", "pdmpc_bulk_kernel_wide_any"},
                                            {"pdmpc_bulk_kernel_sat", "pdmpc_bulk_kernel_sat_any"},
                                            {"pdmpc_bulk_kernel_compact", "pdmpc_bulk_kernel_compact_any"}};

// Which of the four search kernels a layout runs, and which of its two instantiations: the product one exactly
// when the launch's switches are the ones it has compiled in (pdmpc_device.h: ProductSwitches) -- not with a debug or test switch of
// PDMPC_TUNING set, or maneuver areas that are not where that kernel expects them (a small soup grown until they move to L2) --, and never with generic=1.
inline int bulk_variant(const LaunchDims& d, const LaunchPlan& p) {
    return p.compact ? PDMPC_BULK_COMPACT : (d.checker == PDMPC_CHECK_SAT ? PDMPC_BULK_SAT : (d.n_words != 1 ? PDMPC_BULK_WIDE : PDMPC_BULK));
}
inline bool bulk_generic(const Tuning& T, const LaunchPlan& p) {
    KernelArgs a{};  // (the switches the launch will read: ProductSwitches::matches looks at nothing else)
    set_plan_args(T, p, a);
    return T.generic != 0 || !ProductSwitches::matches(a, p.variant);
}

// The plan of a launch of `count` searches (sampled: vehicles; joint: problems, with d.soup_cap their soup columns).
// safe: the recovery path after a predecessor time-out (plan_packed_growing) -- slices that are resident as a whole, no helper workgroups
// next to an oversubscribed launch, the default spin limit, no reversed dispatch.  PDMPC_ERR_CAPACITY with `err`: nothing fits.
inline int plan_launch(const Tuning& T, const LaunchDims& d, PlanKind kind, int count, int n_chained, bool safe, LaunchPlan& p, std::string& err) {
    p = LaunchPlan{};
    p.slice = count;
    if (kind == kPlanJoint) {
        p.kernel = "pdmpc_joint_kernel";
        return layout_joint(d, d.soup_cap, p, err);
    }
    const bool search = kind == kPlanSearch;
    if (const int rc = search ? compute_lds_bulk(T, d, count, p, err) : compute_lds_sampled(T, d, p, err)) return rc;
    launch_policy(T, count, d.n_cu, d.device_share, safe, search, n_chained, p);
    p.spin_limit = safe ? (1u << 22) : T.spin_limit;
    p.reverse_dispatch = (!safe && T.reverse_dispatch) ? 1 : 0;
    p.bk_seat_nodes = std::max(1, T.seat_nodes);
    if (search) {
        p.variant = bulk_variant(d, p);
        p.generic = bulk_generic(T, p);
        p.kernel = kBulkKernelNames[p.variant][p.generic ? 1 : 0];
        if (safe && count > d.n_cu) p.slice = d.n_cu;
    } else {
        // (no arenas: the tree is the fixed 288-node tree in LDS.  Resident slices: two workgroups per CU at <= 80 KB, else one)
        p.kernel = "pdmpc_sampled_kernel";
        if (safe) p.slice = p.lds.total <= kLdsMax / 2 ? 2 * d.n_cu : d.n_cu;
    }
    return PDMPC_OK;
}

// The plan of a sampled launch of `count` vehicles with expansion budget `budget` (pdmpc_set_sampled_budget) and `members` members per
// vehicle (pdmpc_set_sampled_ensemble).  One member: the reference's 250 is plan_launch's plan, field for field (pdmpc_sampled_kernel on
// compute_lds_sampled's layout), and any other budget runs sampled_budget_kernel.hip on layout_sampled's with the tree last.  Two or more
// members run sampled_ensemble_kernel.hip on that layout at every budget, 250 included: count * members workgroups, and slices
// of the safe mode that count slots -- as many as are resident with all their members.
inline int plan_sampled(const Tuning& T, const LaunchDims& d, int budget, int members, int count, bool safe, LaunchPlan& p, SampledExtra& extra, std::string& err) {
    if (budget < 1 || budget > PDMPC_SAMPLED_BUDGET_MAX) {
        err = "the sampled optimizer's budget must be in 1..PDMPC_SAMPLED_BUDGET_MAX";
        return PDMPC_ERR_INVALID;
    }
    if (members < 1 || members > PDMPC_SAMPLED_ENSEMBLE_MAX) {
        err = "the sampled optimizer's ensemble size must be in 1..PDMPC_SAMPLED_ENSEMBLE_MAX";
        return PDMPC_ERR_INVALID;
    }
    if (budget == PDMPC_SAMPLED_BUDGET_DEFAULT && members == 1) {
        extra = SampledExtra{};
        extra.rand_chunk = d.Hp * PDMPC_SAMPLED_BUDGET_DEFAULT;  // (the whole stream at once, into LDS)
        if (const int rc = plan_launch(T, d, kPlanSampled, count, 0, safe, p, err)) return rc;
        extra.grid = std::min(p.slice, count);
        return PDMPC_OK;
    }
    p = LaunchPlan{};
    p.slice = count;
    bool tree_in_lds;
    if (const int rc = layout_sampled(T, d, pdmpc_sb_tree_bytes((uint32_t)budget), PDMPC_SB_MT_BYTES, true, p, tree_in_lds, err)) return rc;
    extra = {(int)pdmpc_sb_node_cap((uint32_t)budget), tree_in_lds ? 1 : 0, tree_in_lds ? 0 : (int64_t)pdmpc_sb_tree_bytes((uint32_t)budget), PDMPC_SB_TWIST};
    // the kernel ends its loop on n_nodes + Hp < node_cap like pdmpc_sampled_kernel; with n_nodes <= budget that must never bind
    if (!(budget + d.Hp < extra.node_cap) || 1 + budget + PDMPC_HP_MAX - 1 > 0xffff) {
        err = "plan_sampled: the tree's capacity does not cover the budget";
        return PDMPC_ERR_INVALID;
    }
    launch_policy(T, count, d.n_cu, d.device_share, safe, false, 0, p);
    p.spin_limit = safe ? (1u << 22) : T.spin_limit;
    p.reverse_dispatch = (!safe && T.reverse_dispatch) ? 1 : 0;
    p.bk_seat_nodes = std::max(1, T.seat_nodes);
    const int resident = p.lds.total <= kLdsMax / 2 ? 2 * d.n_cu : d.n_cu;  // workgroups
    if (members == 1) {
        p.kernel = extra.tree_in_lds ? "pdmpc_sampled_budget_kernel" : "pdmpc_sampled_budget_kernel_hbm";
        if (safe) p.slice = resident;
    } else {
        p.kernel = extra.tree_in_lds ? "pdmpc_sampled_ensemble_kernel" : "pdmpc_sampled_ensemble_kernel_hbm";
        if (safe) p.slice = std::max(1, resident / members);
        extra.members = members;
        extra.member_bytes = (int64_t)members * (int64_t)sizeof(pdmpc_vehicle_out);
        extra.ensemble_tree_bytes = (int64_t)members * extra.tree_hbm_bytes;
    }
    extra.grid = (int64_t)std::min(p.slice, count) * members;
    return PDMPC_OK;
}

// PDMPC_TUNING=debug_lds=1: the layout of a search launch and the kernel instantiation that runs it, one line (tests parse it)
inline std::string format_bulk_layout(const LaunchPlan& p, int count) {
    const uint32_t near = (p.compact ? PDMPC_LK_COMPACT_BK_PER : PDMPC_BK_PER) * (uint32_t)p.n_waves * PDMPC_WAVE;
    char buf[320];
    if (p.compact)
        snprintf(buf, sizeof buf, "pdmpc LDS layout (compact): launch %d waves %d near %u ready %d nv %d nl %d total %u kernel %s\n", count, p.n_waves, near, p.ready, p.NV, p.NL, p.lds.total, p.kernel);
    else
        snprintf(buf, sizeof buf, "pdmpc LDS layout: launch %d waves %d areas %d near %u ready %d nv %d nl %d total %u kernel %s\n", count, p.n_waves, p.areas_in_lds, near, p.ready, p.NV, p.NL,
                 p.lds.total, p.kernel);
    return buf;
}

// a plan as the record of the windows (pdmpc_launch_plan)
inline void plan_record(const LaunchPlan& p, bool joint, pdmpc_launch_plan& plan) {
    const LdsLayout& L = p.lds;
    const JointLds& J = p.joint;
    plan = {p.n_waves, p.NL, p.NV, p.areas_in_lds, p.ready, p.compact ? 1 : 0, p.bk_ready_cap, p.bk_round0, p.bk_round, p.bk_ramp, p.bk_tile, p.bk_share_min,
            p.n_helpers, p.bk_helpers_first, p.bk_seat_nodes, p.reverse_dispatch, p.variant, p.generic ? 1 : 0, p.slice, (int32_t)p.heap_lds, p.spin_limit,
            joint ? J.mask : L.mask, joint ? J.man_index : L.man_index, joint ? J.pose : L.pose, joint ? J.area : L.area, joint ? J.ref : L.ref, joint ? J.shape : L.shape,
            L.path, joint ? J.soup : L.soup, L.cand, L.vstate, L.expand, L.tree16, L.rand, L.nodes, joint ? J.total : L.total, L.bk_near_key, L.bk_near_id, L.bk_ready,
            L.bk_hist, L.bk_misc, L.bk_pshape, L.reach_shared, L.bk_reach, L.reach, J.ints, J.succ, J.heap_key, J.heap_id, p.kernel};
}

// pdmpc_launch_plan_host (include/pdmpc.h), the window: the plan of the launch a query describes, as the record a test reads
inline int plan_query(const char* tuning, const pdmpc_launch_query& q, pdmpc_launch_plan& plan, std::string& err) {
    Tuning T;
    if (!parse_tuning(tuning, T, err)) return PDMPC_ERR_INVALID;
    LaunchDims d{q.checker, q.Hp, q.n_trims, 0, q.n_man, 0, 0, q.n_cu, q.device_share, (uint32_t)q.max_nodes, q.kind == kPlanSampled, q.soup_cap, q.ll_cap, q.cand_cap};
    mpa_table_sizes(d);
    LaunchPlan p;
    if (const int rc = plan_launch(T, d, (PlanKind)q.kind, q.count, q.n_chained, q.safe != 0, p, err)) return rc;
    plan_record(p, q.kind == kPlanJoint, plan);
    return PDMPC_OK;
}

// pdmpc_sampled_plan_host and pdmpc_sampled_ensemble_plan_host (include/pdmpc.h): the windows on plan_sampled.  n_extra: 4 or 8 numbers
inline void sampled_extra_record(const SampledExtra& x, int n_extra, int64_t* extra) {
    const int64_t all[8] = {x.node_cap, x.tree_in_lds, x.tree_hbm_bytes, x.rand_chunk, x.member_bytes, x.ensemble_tree_bytes, x.grid, x.members};
    for (int i = 0; i < n_extra; ++i) extra[i] = all[i];
}
inline int plan_sampled_query(const char* tuning, const pdmpc_launch_query& q, int budget, int members, pdmpc_launch_plan& plan, int n_extra, int64_t* extra, std::string& err) {
    Tuning T;
    if (!parse_tuning(tuning, T, err)) return PDMPC_ERR_INVALID;
    LaunchDims d{q.checker, q.Hp, q.n_trims, 0, q.n_man, 0, 0, q.n_cu, q.device_share, (uint32_t)q.max_nodes, true, q.soup_cap, q.ll_cap, q.cand_cap};
    mpa_table_sizes(d);
    LaunchPlan p;
    SampledExtra x;
    if (const int rc = plan_sampled(T, d, budget, members, q.count, q.safe != 0, p, x, err)) return rc;
    plan_record(p, false, plan);
    sampled_extra_record(x, n_extra, extra);
    return PDMPC_OK;
}
