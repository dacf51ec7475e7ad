// handle.hpp — what the translation units of the C ABI's host side share (api.cpp: the searches; pack.cpp: the packer; step_prep.cpp:
// the step-preparation calls): struct pdmpc_handle and its parts, on the plumbing of hip_host.hpp (error reporting, the device guard,
// the owning buffers).  Private to the library.
#pragma once
#include <vector>

#include "hdv_host.hpp"    // the HDV map as it is taken over (host only)
#include "hip_host.hpp"
#include "launch_plan.hpp"  // struct Tuning, the plan of a launch (host only)
#include "pdmpc_device.h"


// The per-vehicle arenas of the searches (NodeArena, pdmpc_device.h): max_nodes entries per vehicle in every array (contents are
// scratch: every search starts from an empty tree).
struct Arenas {
    uint32_t max_nodes = 0;
    DevBuf<NodeRec> nodes;
    DevBuf<double> key, far_key, mid_key, pb_key, walk;
    DevBuf<unsigned long long> link;
    DevBuf<uint32_t> far_id, mid_id, pb_d, child0, vlist;
    DevBuf<uint8_t> vstate;
    // every array with its entries per node: walk holds 16 bytes per node, vlist the verification's Hp + 1 lists
    template <class Self, class F>
    static void each(Self& a, int Hp, F&& f) {
        f(a.nodes, 1);
        f(a.key, 1);
        f(a.link, 1);
        f(a.vstate, 1);
        f(a.far_key, 1);
        f(a.far_id, 1);
        f(a.mid_key, 1);
        f(a.mid_id, 1);
        f(a.pb_key, 1);
        f(a.pb_d, 1);
        f(a.walk, 2);
        f(a.child0, 1);
        f(a.vlist, Hp + 1);
    }
    size_t bytes_per_node(int Hp) const {
        size_t sum = 0;
        each(*this, Hp, [&](const auto& b, int per) { sum += (size_t)per * sizeof *b.p; });
        return sum;
    }
    // everything released first (the arenas are sized in gigabytes); on failure max_nodes is 0 and the caller allocates again
    int alloc(int max_vehicles, uint32_t n, int Hp) {
        n = (n + 1u) & ~1u;
        const size_t tot = (size_t)max_vehicles * n;
        each(*this, Hp, [](auto& b, int) { b.release(); });
        max_nodes = 0;
        int bad = 0;
        each(*this, Hp, [&](auto& b, int per) { bad |= b.ensure_exact(tot * (size_t)per); });
        if (bad) return bad;
        max_nodes = n;
        return 0;
    }
    NodeArena view() const {
        return {nodes.p, key.p, link.p, vstate.p, far_key.p, far_id.p, mid_key.p, mid_id.p, pb_key.p, pb_d.p, walk.p, child0.p, vlist.p};
    }
};

// pdmpc_stats.kernel: what the last launch ran
enum LaunchKind : int32_t { kLaunchSearch = 2, kLaunchSampled = 3, kLaunchJoint = 4 };

// the regions of a batch blob: [vehicles | predecessor slots | points], each starting on a multiple of 16 bytes
struct BlobRegions {
    DevVehicle* veh = nullptr;
    int32_t* pred = nullptr;
    double* pts = nullptr;
};

// one packed batch: host mirror (pinned) + device copy, each ONE allocation -- BlobRegions --
// so a pack is one host-to-device copy
struct PackedStep {
    PinnedBuf<unsigned char> h_blob;
    DevBuf<unsigned char> d_blob;
    BlobRegions host, dev;  // (views into the blobs, set by pack_common)
    uint64_t staged_serial = ~0ull;  // the handle's sync_serial when the copy out of h_blob was queued (pack_common)
    int n_packed = 0;
    bool pack_failed = false;  // the last pack into this bank did not finish: nothing to launch or fetch
    SampledBank sampled;       // packed with seeds (pdmpc_set_step_seeds): its launches run the sampled optimizer, with the handle's budget and ensemble size of then
    int soup_cap = 0;
    int ll_cap = 0;    // most lanelet-boundary columns of any vehicle (the graph search's reach lists hold one boundary list per step)
    int cand_cap = 0;  // most segments any single edge check can see (one step's soups + the boundary)
    std::vector<int64_t> lit_cols;  // per slot: literal soup + boundary columns (for the bytes formula)
    std::vector<int32_t> perm;      // empty: slot s holds the caller's vehicle s; else slot s holds vehicle perm[s] (pack_common put the batch into level order)
    std::vector<int32_t> inv;       // ... and vehicle v sits in slot inv[v]
};

// what pack_common tells vehicles that hand over the same arrays by: the pointers and counts of a vehicle's polygon sets
struct SoupKey {
    const void* p[13];
    int32_t c[6];
};

// pack_common's scratch, kept with the handle for its allocations: an open-addressing table over the slots that brought new arrays
// (a batch of 1 280 slots looks its key up 1 280 times)
struct SoupTable {
    std::vector<SoupKey> keys;   // key of the q-th distinct vehicle, slot[q] the slot it was packed in
    std::vector<int32_t> slot;
    std::vector<int32_t> table;  // hash -> q + 1, 0 = empty
    static uint64_t hash(const SoupKey& k) {
        static_assert(sizeof(SoupKey) % 8 == 0, "SoupKey is hashed by 64-bit words");
        uint64_t hsh = 1469598103934665603ull;
        const uint64_t* w = (const uint64_t*)&k;
        for (size_t q = 0; q < sizeof(SoupKey) / 8; ++q) hsh = (hsh ^ w[q]) * 1099511628211ull;
        return hsh ^ (hsh >> 29);
    }
    void reset(int n) {  // empty, with room for n keys
        size_t size = 64;
        while (size < (size_t)n * 2) size *= 2;
        keys.clear();
        slot.clear();
        table.assign(size, 0);
    }
    // the slot the key was packed in, or -1 and `at`: where insert puts it
    int find(const SoupKey& k, size_t& at) const {
        for (at = (size_t)hash(k) & (table.size() - 1); table[at] != 0; at = (at + 1) & (table.size() - 1)) {
            const int q = table[at] - 1;
            if (std::memcmp(&keys[(size_t)q], &k, sizeof k) == 0) return slot[(size_t)q];
        }
        return -1;
    }
    void insert(const SoupKey& k, int packed_in, size_t at) {
        keys.push_back(k);
        slot.push_back(packed_in);
        table[at] = (int32_t)keys.size();
    }
};

// The event pairs around the search launches of a handle (launch_range, pdmpc_plan_joint) and their times for pdmpc_get_last_stats:
// a pair per launch since the last pack or pdmpc_reset_stats.
struct LaunchTimer {
    static constexpr size_t kMaxPairs = 4096;  // event pairs a handle keeps before it folds their times (begin)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    double folded_ms = 0.0;  // launches whose event pairs were recycled (resident launches without a pack or reset in between)
    int64_t folded_launches = 0;
    LaunchKind kind = kLaunchSampled;  // of the last launch (before the first one: what pdmpc_get_last_stats always reported)
    LaunchTimer() = default;
    LaunchTimer(const LaunchTimer&) = delete;
    LaunchTimer& operator=(const LaunchTimer&) = delete;
    ~LaunchTimer() { release(); }
    void release() {
        for (auto& ev : events) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        events.clear();
        used = 0;
    }
    // The next event pair, its start recorded on the stream; end records its end behind the launch.
    int begin(hipStream_t stream, LaunchKind launch_kind) {
        if (used == kMaxPairs) {
            // a caller that launches resident banks for ever (no pack, no pdmpc_reset_stats in between) must not make the handle hold an
            // event pair per launch: the pairs' times are folded into a sum and the pairs used again
            HIPCHK(hipStreamSynchronize(stream));
            for (size_t i = 0; i < used; ++i) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, events[i].first, events[i].second) == hipSuccess) folded_ms += t;
            }
            folded_launches += (int64_t)used;
            used = 0;
        }
        if (used == events.size()) {
            hipEvent_t e0, e1;
            HIPCHK(hipEventCreate(&e0));
            HIPCHK(hipEventCreate(&e1));
            events.emplace_back(e0, e1);
        }
        HIPCHK(hipEventRecord(events[used++].first, stream));
        kind = launch_kind;
        return PDMPC_OK;
    }
    int end(hipStream_t stream) {
        HIPCHK(hipEventRecord(events[used - 1].second, stream));
        return PDMPC_OK;
    }
    void reset() {  // the pairs stay for the next launches
        used = 0;
        folded_ms = 0.0;
        folded_launches = 0;
    }
    // kernel time and number of the launches since the last reset, once the stream is idle
    int total(double& ms, int64_t& launches) const {
        ms = folded_ms;
        for (size_t i = 0; i < used; ++i) {
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, events[i].first, events[i].second));
            ms += t;
        }
        launches = folded_launches + (int64_t)used;
        return PDMPC_OK;
    }
    // time of the last launch, once the stream is idle behind it; false: no launch, or its events are not readable
    bool last_ms(float& ms) const { return used > 0 && hipEventElapsedTime(&ms, events[used - 1].first, events[used - 1].second) == hipSuccess; }
};

// ---- state of the step-preparation calls (step_prep.cpp): work that runs once per time step before the searches are packed

// The event pair around one launch per call and its time (timed_launch in step_prep.cpp creates and records them): destroyed with
// its owner (pdmpc_destroy deletes the handle on the handle's device, after the handle's destructor has synchronised the stream).
struct TimedLaunch {
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms = 0.0f;  // of the last launch that was folded
    TimedLaunch() = default;
    TimedLaunch(const TimedLaunch&) = delete;
    TimedLaunch& operator=(const TimedLaunch&) = delete;
    ~TimedLaunch() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void fold() {  // after the stream was synchronised behind ev[1]
        float t = 0.0f;
        if (hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) ms = t;
    }
};

// pdmpc_unique_priorities / pdmpc_unique_priorities_grouped (priority_kernel.hip): grown when a call needs more, kept otherwise
struct PrioState {
    DevBuf<uint32_t> count, mask;  // acyclic masks per tile, the acyclic masks
    DevBuf<int64_t> off;           // exclusive offsets of the tiles (entry n_tiles: the total)
    DevBuf<int32_t> order;         // the priorities of every acyclic mask
    // the grouped call: a PriorityArgs per graph, the tile prefix and the row bases (prio_layout in step_prep.cpp) with their pinned
    // staging, and where every graph's masks start (read back in one copy)
    DevBuf<unsigned char> table;
    PinnedBuf<unsigned char> h_table;
    DevBuf<int64_t> group_off;
    PinnedBuf<int64_t> h_group_off;
    std::vector<int32_t> edges;    // E per graph (-1: outside the limits)
};

// pdmpc_upload_reachable_sets / pdmpc_reachable_set_coupling (reachable_kernel.hip): the local hulls, and the coupler's workspace
// and pinned staging (reach_layout), sized at upload for max_vehicles vehicles
struct ReachState {
    bool valid = false;  // an upload succeeded
    int trims = 0, Hp = 0, cols = 0;
    DevBuf<double> local;   // x of every trim's step-Hp hull, then y
    DevBuf<int32_t> off;    // [n_trims + 1]
    std::vector<int32_t> off_host;
    DevBuf<unsigned char> ws;
    PinnedBuf<unsigned char> h_in, h_out;
    DevBuf<double> all;     // every trim's local hulls of every step (x, then y), for pdmpc_bound_reachable_sets
    DevBuf<int32_t> all_off;  // [n_trims * Hp + 1]
    int all_tot = 0;
    TimedLaunch coupling;
};

// pdmpc_bound_reachable_sets / pdmpc_bounded_set_coupling (bounded_kernel.hip): the sets of the last bound call stay here; grown
// when a call needs more, kept otherwise
struct BoundState {
    bool valid = false;  // the last bound call succeeded
    int n = 0, S = 0, n_lan = 0;
    DevBuf<unsigned char> in;   // the staged inputs (bound_layout)
    DevBuf<double> sets;        // slots: x of every set, then y
    DevBuf<int32_t> set_n, pairs;  // vertices per set | the pair list, then its counter
    DevBuf<uint8_t> flags;
    DevBuf<double> box;
    DevBuf<unsigned char> out;  // adjacency and areas (carve_pair_out)
    PinnedBuf<unsigned char> h_in, h_out;
    PinnedBuf<double> h_xy;
    TimedLaunch bounding, coupling;
};

// pdmpc_fca_collisions (fca_kernel.hip): workspace and pinned staging of the inputs (carved in the call) and of the counts; grown when a
// call needs more, kept otherwise
struct FcaState {
    DevBuf<unsigned char> ws;
    PinnedBuf<unsigned char> h_in;
    PinnedBuf<int32_t> h_out;
    TimedLaunch timed;
};

// pdmpc_upload_hdv_map(_slot) / pdmpc_hdv_traffic(_grouped) (hdv_kernel.hip): a map and the HDV automaton's local hulls
// in one device table (hdv_table), the workspace of the four calls with its pinned staging (ONE layout, hdv_ws: h_in holds its first
// in_bytes, h_out what is read back from `out` on) and the slots of the lane pass (hdv_slot_doubles) -- all three in
// hdv_call_host.hpp, with the stages of a call; the workspace and the slots are grown when a call needs more, kept otherwise
// A handle has PDMPC_HDV_MAP_SLOTS map slots (pdmpc_upload_hdv_map_slot), each with its own table and the host's copy of it;
// pdmpc_hdv_traffic reads slot 0, a group of pdmpc_hdv_traffic_grouped the slot it names, through `maps`: one HdvMapRecord per slot
// on the device, written at the upload.
struct HdvMapSlot {
    bool valid = false;      // an upload succeeded
    int64_t generation = 0;  // of that upload (0: none): larger than any generation before it
    HdvSlotData data;        // the host's copy: sizes, limits, the offsets of the table; what pdmpc_hdv_map_slot_holds compares with
    DevBuf<unsigned char> table;
};
struct HdvState {
    HdvMapSlot map[PDMPC_HDV_MAP_SLOTS];
    int64_t uploads = 0;   // successful uploads into any slot so far
    DevBuf<HdvMapRecord> maps;
    DevBuf<unsigned char> ws;
    DevBuf<double> slots;  // x of every slot, then y
    PinnedBuf<unsigned char> h_in, h_out;
    TimedLaunch timed;
};

// pdmpc_choose_resident / pdmpc_plan_step_chosen (choice_kernel.hip): the staged lists, the read-back block (counters, chosen, cell
// costs, picked records: ChoiceLayout in choice_host.hpp) and the status tally; grown when a call needs more, kept otherwise
struct ChoiceState {
    DevBuf<int32_t> in, tally;
    PinnedBuf<int32_t> h_in;
    DevBuf<unsigned char> out;
    PinnedBuf<unsigned char> h_out;
    TimedLaunch timed;
};

// The sampled optimizer (sampled_launch.hpp): what the next pack of a sampled bank gives its bank, what the last launch ran, and the
// scratch of banks that need any (SampledNeed, launch_plan.hpp): the trees of a budget that does not fit LDS (sampled_budget.h) and
// the members of a seed ensemble (sampled_ensemble.h).  Like d_out the scratch is the handle's, shared by its banks and only grown,
// by the pack that needs more: resident banks of other budgets and sizes launch on it one after the other, and no launch reads
// anything of it that it has not written -- the tickets are cleared ahead of every launch.
struct SampledState {
    PendingSeeds seeds;                    // pdmpc_set_step_seeds: taken by the next pack, which makes its bank a sampled bank
    int budget = PDMPC_SAMPLED_BUDGET_DEFAULT;  // pdmpc_set_sampled_budget
    int members = 1;                       // pdmpc_set_sampled_ensemble
    int ensemble_bank = -1;                // the bank whose launch wrote the entries last (pdmpc_sampled_ensemble_result), -1: none since its pack
    const char* last_kernel = "";          // pdmpc_last_sampled_kernel
    DevBuf<uint16_t> tree;                 // SampledNeed::tree
    DevBuf<pdmpc_vehicle_out> member_out;  // SampledNeed::per_member: [slot * E + e] ...
    DevBuf<EnsembleEntry> member_entry;
    DevBuf<int32_t> member_nodes;
    DevBuf<uint32_t> ticket;               // SampledNeed::per_slot: [slot], cleared on the stream ahead of every launch of an ensemble bank ...
    DevBuf<int32_t> chosen;                // ... the member the kernel chose
    bool holds_trees(const SampledNeed& n) const { return tree.cap >= n.tree; }
    bool holds_members(const SampledNeed& n) const {
        return member_out.cap >= n.per_member && member_entry.cap >= n.per_member && member_nodes.cap >= n.per_member && ticket.cap >= n.per_slot && chosen.cap >= n.per_slot;
    }
    // (the stream idle: a launch of a resident bank may still use a buffer that is freed)
    int grow_trees(const SampledNeed& n) { return tree.ensure_exact(n.tree); }
    int grow_members(const SampledNeed& n) {
        return member_out.ensure_exact(n.per_member) | member_entry.ensure_exact(n.per_member) | member_nodes.ensure_exact(n.per_member) | ticket.ensure_exact(n.per_slot) | chosen.ensure_exact(n.per_slot);
    }
};

struct pdmpc_handle {
    pdmpc_config cfg{};
    Tuning tune{};
    hipStream_t stream = nullptr;
    int n_cu = 256;
    // MPA
    bool has_mpa = false;
    int n_trims = 0, n_words = 0, n_man = 0;
    DevBuf<uint64_t> d_mask;
    DevBuf<int16_t> d_mi;
    DevBuf<DevManPose> d_pose;
    DevBuf<double> d_area;
    size_t mask_bytes = 0, mi_bytes = 0;
    int64_t mpa_alg_bytes = 0;
    Arenas arena;
    uint32_t max_nodes_limit = 0;  // pdmpc_plan_* may grow the arenas up to this many nodes per vehicle (0: as far as HBM allows)
    int64_t arena_regrows = 0;     // times an overflowed call was re-planned with larger arenas
    int64_t safe_replans = 0;      // times a call was re-planned in resident slices after a predecessor time-out
    bool safe_launches = false;    // pdmpc_set_safe_launch: every launch in resident slices
    int max_vehicles = 0;
    DevBuf<pdmpc_vehicle_out> d_out;
    DevBuf<uint32_t> d_flag;
    DevBuf<int32_t> d_tree_size;
    DevBuf<int32_t> d_tie_count;
    DevBuf<unsigned long long> d_work_count;
    DevBuf<unsigned long long> d_help_board;  // helper workgroups (pdmpc_device.h)
    DevBuf<uint32_t> d_help_verdict, d_help_finished;
    DevBuf<double> d_bk_post;                 // records posted for the helper workgroups
    DevBuf<int32_t> d_joint_off;         // pdmpc_plan_joint: the problems' first slots
    // the step-preparation calls (step_prep.cpp), one member per call family: a family's ungrouped and grouped entry points stage
    // through one body into the same buffers
    PrioState prio;
    ReachState reach;
    BoundState bound;
    FcaState fca;
    HdvState hdv;
    ChoiceState choice;
    SampledState sampled;
    int device_share = 1;                // handles of one process that launch on this device side by side (pdmpc_set_device_share: a group's logical ranks)
    bool boards_dirty = true;            // the helper boards / the finished counter need clearing before the helper workgroups may read them
    uint32_t help_fin_total = 0;         // value of the finished counter once every launch so far has ended
    uint32_t launch_serial = 0;          // SEARCH launches of this handle so far: its only reader is KernelArgs::launch_id, which tells the helper boards' words of one search launch from an earlier one's (a sampled or joint launch has no boards and does not count)
    double last_us[3] = {0, 0, 0};       // pdmpc_last_call_timing: pack, enqueue, wait + read-back of the last pdmpc_plan_batch / pdmpc_plan_step
    double dbg_us[4] = {0, 0, 0, 0};     // debug_host 2: pack, launch, fetch (host clock) and kernel (events) time of the plan_batch calls
    uint64_t sync_serial = 0;            // stream synchronisations through sync_stream so far (PackedStep::staged_serial)
    SoupTable soups;                     // pack_common's scratch: vehicles by all their arrays,
    SoupTable obstacle_soups, boundary_soups;  // ... by their obstacle arrays, by their boundary arrays
    std::vector<double> next_weights;    // pdmpc_set_step_weights: expected work per vehicle of the NEXT packed step (the caller's order); consumed by that pack
    PinnedBuf<double> h_lean;            // fetch_lean: (cost, status) per slot
    DevBuf<double> d_lean;
    PinnedBuf<pdmpc_vehicle_out> h_out;  // pdmpc_fetch_results: the records land in pinned memory (a copy into the caller's pageable array goes through the runtime's staging otherwise)
    uint32_t* progress = nullptr;        // pinned, debug_progress
    // batch blobs: several packed steps can stay resident side by side ("banks", pdmpc_select_bank)
    std::vector<PackedStep> banks;
    int bank = 0;
    uint32_t epoch = 1;  // done flags start at 0, so no slot looks solved before its first launch
    LaunchTimer timer;  // launches
    pdmpc_stats stats{};
    // the buffers free themselves after this: the stream is idle by then
    ~pdmpc_handle() {
        if (stream) (void)hipStreamSynchronize(stream);
        timer.release();  // (the launches' events go before their stream)
        if (progress) (void)hipHostFree(progress);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// what planning reads of the handle and of a packed bank (launch_plan.hpp: LaunchDims)
inline LaunchDims launch_dims(const pdmpc_handle* h, const PackedStep& B) {
    return {h->cfg.checker, h->cfg.Hp, h->n_trims, h->n_words, h->n_man, h->mask_bytes, h->mi_bytes, h->n_cu, h->device_share, h->arena.max_nodes,
            B.sampled.on, B.soup_cap, B.ll_cap, B.cand_cap};
}

// what the graph search, the sampled optimizer and the joint search (KernelArgs, SampledArgs, JointArgs) all read: the automaton, the
// packed batch, the records, the tree sizes and work counters
template <class Args>
void set_batch_args(const pdmpc_handle* h, const PackedStep& B, int areas_in_lds, Args& a) {
    a.succ_mask = h->d_mask.p;
    a.man_index = h->d_mi.p;
    a.man_pose = h->d_pose.p;
    a.man_area = h->d_area.p;
    a.n_trims = h->n_trims;
    a.n_words = h->n_words;
    a.n_man = h->n_man;
    a.Hp = h->cfg.Hp;
    a.areas_in_lds = areas_in_lds;
    a.veh = B.dev.veh;
    a.points = B.dev.pts;
    a.out = h->d_out.p;
    a.tree_size = h->d_tree_size.p;
    a.work_count = h->d_work_count.p;
}

// hipStreamSynchronize on the launch stream, counted: a bank whose staging copy was queued before is free again (pack_common)
inline hipError_t sync_stream(pdmpc_handle* h) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) h->sync_serial += 1;
    return e;
}

// pack.cpp: the packer behind pdmpc_pack_step / pdmpc_pack_batch (flattens the caller's vehicles into the bank's blob and uploads it);
// not an export of the library
__attribute__((visibility("hidden"))) int pack_common(pdmpc_handle* h, int n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index, const pdmpc_polygon_set* fallback);
