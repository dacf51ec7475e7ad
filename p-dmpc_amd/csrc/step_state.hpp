// step_state.hpp — the state of the native step controller (step_controller.cpp, stage 5 of 9): the scratch of a step preparation, of the
// assembly and of a batch, and the controller itself as the parts that are written together.
//
// Two records and one path.  A StepProblem is what pdmpc_plan_step takes -- inputs, fallbacks, predecessor slots --
// with its seeds and weights, wherever it lives: a controller's step, each kept instance, its flattened batch, a sweep's concatenated
// step and batch; the per-slot tags (instance, vehicle, level, member, member_slot) are plain vectors next to it.  An Instance is a
// prioritization (both coupling matrices, levels, slot order): the controller's own (c->pri) and every kept one.  build_members
// (step_prepare.hpp) prepares the step of a span of members -- the device calls or their host twins, grouped by member, the only fork on
// the handle, every call that sizes its output under the one capacity retry (with_room, step_hdv.hpp) -- between the per-member halves
// begin_step and finish_step (pdmpc_controller_build_step: M = 1, in the controller's own scratch); plan_built plans a StepProblem (weights, seeds, the backend call, timing[1..3]); timed_steps is the loop of every *_run.
#pragma once
#include <memory>
#include <string>

#include "step_inputs.hpp"
#include "step_hdv.hpp"
#include "step_priorities.hpp"

namespace {
// What a member's step reads of the reachable sets (begin_step), and the scratch of ONE step preparation over a span of members
// (build_members): a sweep owns one for its members, a controller one for the steps it takes alone.
struct StepPrep {
    bool reach_parallel = false, reach = false, bounded = false;
};
struct PrepScratch {
    std::vector<StepPrep> prep;            // per member
    int32_t prep_calls[4] = {0, 0, 0, 0};  // of the last build: lanelet bounding, bounded coupling, hull coupling, collision assessment
    // one grouped bounding / coupler call: the vehicles of the members that take part, member after member
    struct Call {
        std::vector<int> who;                // members
        std::vector<int32_t> group_offset;   // [who.size() + 1]
        std::vector<double> x, y, cos_yaw, sin_yaw;
        std::vector<int32_t> trim, lan_off, set_off;
        std::vector<double> lan_x, lan_y, set_x, set_y;
        std::vector<uint8_t> adjacency;      // the blocks
    } call;
    int32_t hdv_calls[2] = {0, 0};  // ... its HDV traffic calls and the map uploads they needed (pdmpc_sweep_last_hdv_calls)
    HdvCallScratch hdv;             // ... and the scratch of one grouped call of them (step_hdv.hpp)
    // the grouped collision assessment: the FCA members' reference points, member after member, and what it returns
    struct Fca {
        std::vector<pdmpc_fca_group> groups;
        std::vector<pdmpc_polygon_set> obstacles;  // [groups.size()] views of the members' scenario obstacles
        std::vector<double> x, y, cos_yaw, sin_yaw;
        std::vector<int32_t> collisions, priorities;
    } fca;
    // the grouped enumeration of an optimal-priority step: the members' coupling graphs, and their lists one after the other
    struct Prio {
        int32_t calls = 0;  // enumeration calls of the last build
        std::vector<int32_t> group_n;
        std::vector<const uint8_t*> adjacency;
        std::vector<int64_t> max_out, n_out;
        std::vector<uint32_t> masks;
        std::vector<int32_t> priorities;
    } prio;
};
// the batch of prioritizations build_members puts behind every member's step: none, the explorative one (n_perm > 0) or the
// optimal-priority one (max_instances > 0)
struct BatchKind {
    int n_perm = 0, max_instances = 0;
};

// the arrays of the step's polygon sets: chunks that are kept from step to step and handed out front to back (a set's arrays
// never move; build_step starts over at the first chunk)
struct Arena {
    struct Chunk {
        std::unique_ptr<double[]> mem;  // (doubles: 8-byte alignment for both kinds of arrays)
        size_t cap = 0;
    };
    std::vector<Chunk> chunks;
    size_t cur = 0, used = 0;
    [[maybe_unused]] void reset() { cur = used = 0; }
    [[maybe_unused]] void* take(size_t bytes) {
        const size_t need = (bytes + 7) / 8;
        while (cur < chunks.size() && used + need > chunks[cur].cap) {
            ++cur;
            used = 0;
        }
        if (cur == chunks.size()) {
            Chunk ch;
            ch.cap = std::max(need, (size_t)1 << 17);
            ch.mem.reset(new double[ch.cap]);
            chunks.push_back(std::move(ch));
            used = 0;
        }
        void* p = chunks[cur].mem.get() + used;
        used += need;
        return p;
    }
};

// obstacle sets of a vehicle by who contributes to them (a function of the vehicle and of those lists alone): the prioritizations
// of an explorative step differ in a few couplings, so most of their vehicles share their sets — one build, one pointer, and
// pdmpc_pack_step packs a set it has seen under the same pointer once (pack.cpp: pack_common)
struct MemoKey {  // who contributes, as bit masks over the vehicles (up to 512: larger scenarios build every set)
    uint64_t w[16];
};
struct Memo {  // a vehicle's sets built so far this step, by key (a handful: searched front to back)
    std::vector<MemoKey> keys;
    std::vector<pdmpc_polygon_set> sets;
    [[maybe_unused]] const pdmpc_polygon_set* find(const MemoKey& k) const {
        for (size_t q = 0; q < keys.size(); ++q)
            if (std::memcmp(keys[q].w, k.w, sizeof k.w) == 0) return &sets[q];
        return nullptr;
    }
    [[maybe_unused]] void clear() {
        keys.clear();
        sets.clear();
    }
};

// The scratch of assemble_step: no meaning between steps (kept: no allocation per prioritization)
struct Assembly {
    Arena arena;
    std::vector<int32_t> sb_off;  // SetBuilder's scratch (one builder at a time)
    std::vector<double> sb_x, sb_y;
    // sets that do not depend on the prioritization are built once per time step and shared by the prioritizations of an explorative step
    std::vector<pdmpc_polygon_set> fb_of;
    std::vector<uint8_t> fb_done;
    std::vector<Memo> obst_memo, dyn_memo;
    Lists ls_dir_succ, ls_dir_pred, ls_seq_succ, ls_seq_pred;
    KahnScratch kahn;
    pdmpc_polygon_set empty_set{};
    bool empty_done = false;
    bool exploring = false;  // an explorative step is being built: its prioritizations share sets through the memos
};

// The batch of an explorative step (PrioritizedExplorativeController) or an optimal-priority step (PrioritizedOptimalController): the
// prioritizations of the current traffic state, flattened, and the choice among their plans
struct Batch {
    std::vector<Instance> inst;
    std::vector<StepProblem> inst_prob;  // an instance's step problem as assemble_step left it (kept from step to step: no allocation once warm)
    StepProblem prob;                    // the flattened batch, and per slot of it:
    std::vector<int32_t> instance, vehicle, level;
    std::vector<int32_t> slot;           // slot[p * n + vehicle] = slot in the flattened batch
    bool built_last = false;             // pdmpc_controller_seeds: the seeds of the batch (else of the controller's prob), whichever was built last
    std::vector<pdmpc_vehicle_out> out;
    std::vector<int32_t> status;
    std::vector<double> final_cost;
    std::vector<int32_t> chosen;  // per vehicle: the instance its sub-graph chose
    std::vector<double> cost;     // n_perm x n_graphs (the optimal step: n x K, row v = vehicle v's sums)
    int graphs = 0;
    // the unique prioritizations of the optimal-priority step's coupling graph
    std::vector<uint32_t> o_masks;  // [K] the acyclic orientations (pdmpc_unique_priorities)
    std::vector<int32_t> o_prio;    // [K x n] their priorities
    ChoiceLists choice;                  // the choice of the last explorative / optimal-priority step as data, and what came back for it:
    std::vector<int32_t> choice_chosen;  // [graphs] the candidate every graph chose
    std::vector<double> choice_cost;     // [cells]
};

// The joint problem of a centralized step (CentralizedController.m:33-59; step_centralized.hpp): one entry per vehicle in vehicle order,
// every entry's obstacles the scenario's set under the same pointers (the arena keeps it alive until the next build)
struct Centralized {
    std::vector<pdmpc_vehicle_in> in;
    bool built = false;
};
}  // namespace

struct pdmpc_controller {
    pdmpc_handle* h = nullptr;
    pdmpc_group* group = nullptr;           // pdmpc_controller_set_group: built problems are planned over this group (h is its rank 0)
    int32_t group_mode = PDMPC_SHARD_AUTO;
    Scenario sc;       // written by pdmpc_controller_create / _set_reachability
    Traffic tr;        // carried from step to step: written by pdmpc_controller_apply
    StepInputs in;     // rewritten every step (begin_step, the step preparation's coupling)
    ReachState reach;
    FcaInputs fca;
    HdvTraffic hdv;    // written by pdmpc_controller_set_hdvs / _set_hdv_measurements and the step's traffic call
    Assembly as;
    Batch x;
    Centralized cen;
    bool follow_own = false;                // the explorative step applies the plans of the controller's OWN prioritization (instance 0) whatever the choice: the traffic then follows pdmpc_controller_step's closed loop (measurement: the same steps as a recorded replay)
    bool lean_explore = false;              // the explorative step reads back status + final cost of every plan and the chosen plans' records only
    bool device_choice = false;             // pdmpc_controller_set_device_choice: the lean step chooses and gathers on the device (pdmpc_plan_step_chosen)
    int optimizer = PDMPC_OPTIMIZER_GRAPH_SEARCH;  // pdmpc_controller_set_optimizer
    Instance pri;                    // the controller's own prioritization (after a choice: every vehicle's row of its chosen instance's couplings)
    StepProblem prob;                // ... and its step problem; the arena keeps the pointed-to data alive
    std::vector<pdmpc_vehicle_out> out;
    double timing[6] = {0, 0, 0, 0, 0, 0};  // pdmpc_controller_last_timing
    double timing_sum[6] = {0, 0, 0, 0, 0, 0};  // ... summed over the steps since the last pdmpc_controller_timing_sum(reset)
    int64_t timing_steps = 0;
    PrepScratch prep;  // of the steps the controller builds alone (as a member of a sweep it is prepared in the sweep's)
    std::string err;
};
