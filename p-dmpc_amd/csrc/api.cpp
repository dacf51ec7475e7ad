// api.cpp — host side of libpdmpc_hip.so: the C ABI declared in include/pdmpc.h.
//
// Responsibilities: own all device memory of a handle, hand the caller's IterationData slices to the packer
// (pack.cpp: the pointer-free HBM blob of pdmpc_device.h), size the LDS regions, launch the search
// kernel on the handle's stream and time it with HIP events, copy results back.
// There is no CPU implementation of the search in this library: without a gfx950 device every planning
// entry point fails with PDMPC_ERR_NO_DEVICE.
// What needs no device lives in host-only headers that report through (return code, std::string& err) and are failed here: the plan of a launch
// (launch_plan.hpp), the automaton's reach and the reach lists (mpa_reach.hpp), the checked choice on the host (choice_host.hpp) and the
// reference's tree read out of a raw arena (reference_tree.hpp).  This file keeps the checks that need the handle, the copies and the launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "choice_host.hpp"
#include "handle.hpp"
#include "mpa_reach.hpp"
#include "reference_tree.hpp"
#include "sampled_launch.hpp"

namespace {

thread_local std::string g_err;  // pdmpc_last_error: every translation unit reports through pdmpc_set_last_error (fail, hip_host.hpp)

// The dynamic LDS size of a kernel is an attribute of the function ON THE DEVICE, not of a handle (hipFuncSetAttribute sets a
// maximum): the largest size set so far is kept per device, kernel (0 bulk, 1 bulk wide, 2 bulk SAT, 3 bulk compact) and instantiation
// (0 product, 1 generic: two functions on the device; kernels in the order of PDMPC_BULK ...), shared by every handle.
std::mutex g_lds_mutex;
uint32_t g_lds_high_water[64][4][2];

// what a search launch reads besides the batch: its plan (set_plan_args), the handle's buffers, the launch's number
void set_launch_args(pdmpc_handle* h, const PackedStep& B, const LaunchPlan& plan, int first, int count, KernelArgs& a) {
    set_batch_args(h, B, plan.areas_in_lds, a);
    set_plan_args(h->tune, plan, a);
    a.dt = h->cfg.dt_seconds;
    a.max_nodes = h->arena.max_nodes;
    a.checker = h->cfg.checker;
    a.pred = B.dev.pred;
    a.done_flag = h->d_flag.p;
    a.epoch = h->epoch;
    a.first = first;
    a.arena = h->arena.view();
    a.soup_cap = B.soup_cap;
    a.cand_cap = B.cand_cap;
    a.tie_count = h->d_tie_count.p;
    if (h->tune.debug_progress && !h->progress) {
        if (hipHostMalloc((void**)&h->progress, (size_t)h->max_vehicles * 64 * 4, hipHostMallocMapped) != hipSuccess) h->progress = nullptr;
        if (h->progress) std::memset(h->progress, 0, (size_t)h->max_vehicles * 64 * 4);
    }
    a.progress = h->progress;
    a.bk_post = h->d_bk_post.p;
    a.help_board = h->d_help_board.p;
    a.help_verdict = h->d_help_verdict.p;
    a.help_finished = h->d_help_finished.p;
    h->launch_serial += 1;
    if (h->launch_serial == 0) h->launch_serial = 1;
    a.launch_id = h->launch_serial;
    a.n_searches = count;
}

// The helper boards of a launch with helper workgroups: where its count of finished searches starts (KernelArgs::help_fin_base).
int prepare_boards(pdmpc_handle* h, int count, uint32_t& fin_base) {
    fin_base = 0;
    if (!h->boards_dirty) {
        // The boards stay closed between launches (a search closes every round it shares before it uses the verdicts, and a closed
        // ticket word offers nothing) and the count of finished searches runs on from launch to launch: nothing to clear -- two
        // memset dispatches less per launch.  A launch that ended with a watchdog status marks them dirty and the next one clears them.
        fin_base = h->help_fin_total;
        h->help_fin_total += (uint32_t)count;
    } else {
        HIPCHK(hipMemsetAsync(h->d_help_board.p, 0, (size_t)h->max_vehicles * PDMPC_HB_WORDS * sizeof(unsigned long long), h->stream));
        HIPCHK(hipMemsetAsync(h->d_help_finished.p, 0, 16 * sizeof(uint32_t), h->stream));
        h->help_fin_total = (uint32_t)count;
        h->boards_dirty = false;
    }
    return PDMPC_OK;
}

// One launch of the graph search, in the two steps timed_launch times: prepare (the plan, the arguments, the helper boards) and go (the
// kernels).
struct SearchLaunch {
    KernelArgs a{};

    int prepare(pdmpc_handle* h, const PackedStep& B, int first, int count, bool safe, LaunchPlan& plan) {
        const LaunchDims dims = launch_dims(h, B);
        int n_chained = 0;
        if (!safe && policy_reads_chained(h->tune, count, dims.n_cu, dims.device_share))
            for (int i = 0; i < count; ++i) n_chained += B.host.veh[first + i].n_pred > 0 ? 1 : 0;
        std::string err;
        int rc = plan_launch(h->tune, dims, kPlanSearch, count, n_chained, safe, plan, err);
        if (rc) return fail(rc, err);
        set_launch_args(h, B, plan, first, count, a);
        if (plan.n_helpers > 0 && (rc = prepare_boards(h, count, a.help_fin_base))) return rc;
        if (h->tune.debug_lds) fputs(format_bulk_layout(plan, count).c_str(), stderr);
        return PDMPC_OK;
    }

    // The kernel launches, plan.slice searches each; returns the hipError_t of the first that failed.
    // Oversubscribed launches (more searches than CUs).  A resident search spins for predecessors of the same launch; slots are in
    // level order (the packer sees to it: coupling_order.hpp), so as long as the hardware hands out workgroups in index order every
    // predecessor was dispatched before its successors and the launch cannot stall.  That order is not a documented guarantee: should a
    // launch ever stall, the watchdog (spin_limit) ends the waiting searches with an error status and plan_packed_growing plans the call
    // again with safe == true, in slices that are resident as a whole (a slice's predecessors are in it or in an earlier slice) -- forward
    // progress then needs no assumption at all.  (The sampled optimizer's launch slices the same way: sampled_launch.hpp.)
    int go(const pdmpc_handle* h, const LaunchPlan& plan) const {
        typedef int (*launcher_t)(const KernelArgs*, int, void*, uint32_t*);
        static const launcher_t launchers[4][2] = {{pdmpc_launch_bulk, pdmpc_launch_bulk_any},
                                                   {pdmpc_launch_bulk_wide, pdmpc_launch_bulk_wide_any},
                                                   {pdmpc_launch_bulk_sat, pdmpc_launch_bulk_sat_any},
                                                   {pdmpc_launch_bulk_compact, pdmpc_launch_bulk_compact_any}};
        const int variant = plan.variant, generic = plan.generic ? 1 : 0;
        int lrc = 0;
        for (int done = 0; done < a.n_searches && lrc == 0; done += plan.slice) {
            KernelArgs part = a;
            part.first = a.first + done;
            part.n_searches = std::min(plan.slice, a.n_searches - done);
            std::lock_guard<std::mutex> lock(g_lds_mutex);
            lrc = launchers[variant][generic](&part, part.n_searches, (void*)h->stream, &g_lds_high_water[h->cfg.device & 63][variant][generic]);
        }
        return lrc;
    }
};

// What the launch of a bank is, whichever optimizer runs it (Launch: SearchLaunch, or SampledLaunch of sampled_launch.hpp): prepared,
// then its kernels between the events of a pair (LaunchTimer), the failure text with the LDS size, the layout's figures for the stats.
template <class Launch>
int timed_launch(pdmpc_handle* h, const PackedStep& B, int first, int count, bool safe, LaunchKind kind) {
    LaunchPlan plan;
    Launch launch;
    int rc = launch.prepare(h, B, first, count, safe, plan);
    if (rc) return rc;
    if ((rc = h->timer.begin(h->stream, kind))) return rc;
    const int lrc = launch.go(h, plan);
    if (lrc != 0) {
        h->boards_dirty = true;  // (the searches that were to count themselves finished never ran: the next launch starts from cleared counters)
        char buf[256];
        snprintf(buf, sizeof buf, "kernel launch failed: %s (LDS %u B)", hipGetErrorString((hipError_t)lrc), plan.lds.total);
        return fail(PDMPC_ERR_HIP, buf);
    }
    if ((rc = h->timer.end(h->stream))) return rc;
    h->stats.lds_bytes = plan.lds.total;
    h->stats.lds_nodes = plan.NL;
    return PDMPC_OK;
}

// safe == true: the recovery path after a predecessor time-out (plan_packed_growing; launch_plan.hpp: plan_launch).
// The bank's kind decides the launch: the graph search's, or the sampled optimizer's for a bank packed with seeds.
int launch_range(pdmpc_handle* h, int first, int count, bool safe) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    PackedStep& B = h->banks[h->bank];
    if (B.pack_failed) return fail(PDMPC_ERR_INVALID, "the last pack into this bank failed: nothing is packed");
    if (first < 0 || count < 0 || first + count > B.n_packed) return fail(PDMPC_ERR_INVALID, "launch range outside the packed batch");
    if (!B.perm.empty() && (first != 0 || count != B.n_packed)) return fail(PDMPC_ERR_INVALID, "range launches need a batch packed in level order (predecessors in lower slots)");
    if (count == 0) return PDMPC_OK;
    return B.sampled.on ? timed_launch<SampledLaunch>(h, B, first, count, safe, kLaunchSampled) : timed_launch<SearchLaunch>(h, B, first, count, safe, kLaunchSearch);
}

// the device-resident record path addresses slots: the caller's vehicles only if the library kept the batch's order
int check_result_slots(const pdmpc_handle* h, int32_t first, int32_t n) {
    if (!h->banks[h->bank].perm.empty()) return fail(PDMPC_ERR_INVALID, "the packed batch was put into level order by the library: raw slots are not the caller's vehicles (pack it in level order to use the device-resident record path)");
    if (first < 0 || n < 0 || first + n > h->max_vehicles) return fail(PDMPC_ERR_INVALID, "slot range out of bounds");
    return PDMPC_OK;
}
}  // namespace

extern "C" {

const char* pdmpc_last_error(void) { return g_err.c_str(); }
void pdmpc_set_last_error(const char* msg) { g_err = msg ? msg : ""; }  // (group.cpp reports through the same string)
const char* pdmpc_version(void) { return "pdmpc-hip 0.1 (gfx950)"; }

int pdmpc_create(const pdmpc_config* config, pdmpc_handle** out_handle) {
    if (!config || !out_handle) return fail(PDMPC_ERR_INVALID, "null argument");
    if (config->Hp < 1 || config->Hp > PDMPC_HP_MAX) return fail(PDMPC_ERR_INVALID, "Hp must be in 1..PDMPC_HP_MAX");
    if (config->checker != PDMPC_CHECK_SAT && config->checker != PDMPC_CHECK_INTERX) return fail(PDMPC_ERR_INVALID, "unknown checker");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(PDMPC_ERR_NO_DEVICE, "no HIP device visible: this backend has no CPU fallback");
    if (config->device < 0 || config->device >= ndev) return fail(PDMPC_ERR_NO_DEVICE, "device ordinal out of range");
    ON_DEVICE(config->device);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, config->device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(PDMPC_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    pdmpc_handle* h = new pdmpc_handle();
    h->cfg = *config;
    h->banks.resize(1);
    {
        std::string err;
        if (!parse_tuning(getenv("PDMPC_TUNING"), h->tune, err)) {
            delete h;
            return fail(PDMPC_ERR_INVALID, err);
        }
    }
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const uint32_t want_nodes = config->max_nodes > 0 ? (uint32_t)config->max_nodes : 32768u;  // default arena: 256 x 32768 nodes, about 0.6 GB
    h->max_vehicles = config->max_vehicles > 0 ? config->max_vehicles : 256;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(PDMPC_ERR_HIP, "hipStreamCreate failed");
    }
    int bad = h->arena.alloc(h->max_vehicles, want_nodes, h->cfg.Hp);
    bad |= h->d_out.ensure((size_t)h->max_vehicles) | h->d_flag.ensure((size_t)h->max_vehicles) | h->d_tree_size.ensure((size_t)h->max_vehicles) | h->d_tie_count.ensure(4) | h->d_work_count.ensure(16);
    bad |= h->d_help_board.ensure((size_t)h->max_vehicles * PDMPC_HB_WORDS) | h->d_help_verdict.ensure((size_t)h->max_vehicles * PDMPC_HELP_CAP) | h->d_help_finished.ensure(16);
    bad |= h->d_bk_post.ensure((size_t)h->max_vehicles * (size_t)h->tune.ready * 6);
    if (bad) {
        delete h;
        return fail(PDMPC_ERR_HIP, "hipMalloc failed for the per-vehicle arenas (lower max_nodes / max_vehicles)");
    }
    (void)hipMemsetAsync(h->d_flag.p, 0, h->d_flag.cap * sizeof(uint32_t), h->stream);
    (void)hipMemsetAsync(h->d_tree_size.p, 0, h->d_tree_size.cap * sizeof(int32_t), h->stream);
    (void)hipMemsetAsync(h->d_tie_count.p, 0, 4 * sizeof(int32_t), h->stream);
    (void)hipMemsetAsync(h->d_work_count.p, 0, 16 * sizeof(unsigned long long), h->stream);
    (void)hipMemsetAsync(h->d_out.p, 0, h->d_out.cap * sizeof(pdmpc_vehicle_out), h->stream);
    (void)hipStreamSynchronize(h->stream);
    *out_handle = h;
    return PDMPC_OK;
}

int pdmpc_launch_plan_host(const char* tuning, const pdmpc_launch_query* q, pdmpc_launch_plan* plan) {
    if (!q || !plan) return fail(PDMPC_ERR_INVALID, "pdmpc_launch_plan_host: null argument");
    if (q->kind < kPlanSearch || q->kind > kPlanJoint) return fail(PDMPC_ERR_INVALID, "pdmpc_launch_plan_host: unknown kind");
    std::string err;
    return failed(plan_query(tuning, *q, *plan, err), err);
}

int pdmpc_sampled_plan_host(const char* tuning, const pdmpc_launch_query* q, int32_t n_expansions_max, pdmpc_launch_plan* plan, int64_t* extra) {
    if (!q || !plan || !extra) return fail(PDMPC_ERR_INVALID, "pdmpc_sampled_plan_host: null argument");
    std::string err;
    return failed(plan_sampled_query(tuning, *q, n_expansions_max, 1, *plan, 4, extra, err), err);
}

int pdmpc_sampled_ensemble_plan_host(const char* tuning, const pdmpc_launch_query* q, int32_t n_expansions_max, int32_t n_members, pdmpc_launch_plan* plan, int64_t* extra) {
    if (!q || !plan || !extra) return fail(PDMPC_ERR_INVALID, "pdmpc_sampled_ensemble_plan_host: null argument");
    std::string err;
    return failed(plan_sampled_query(tuning, *q, n_expansions_max, n_members, *plan, 8, extra, err), err);
}

int pdmpc_sampled_plan_bank(pdmpc_handle* h, int32_t n_expansions_max, pdmpc_launch_plan* plan, int64_t* extra) {
    if (!h || !plan || !extra) return fail(PDMPC_ERR_INVALID, "pdmpc_sampled_plan_bank: null argument");
    const PackedStep& B = h->banks[h->bank];
    if (B.pack_failed || B.n_packed == 0 || !B.sampled.on) return fail(PDMPC_ERR_INVALID, "pdmpc_sampled_plan_bank: the current bank holds no sampled batch");
    LaunchPlan p;
    SampledExtra x;
    std::string err;
    if (const int rc = plan_sampled(h->tune, launch_dims(h, B), n_expansions_max, B.sampled.members, B.n_packed, h->safe_launches, p, x, err)) return fail(rc, err);
    plan_record(p, false, *plan);
    sampled_extra_record(x, 4, extra);
    return PDMPC_OK;
}

int pdmpc_set_sampled_budget(pdmpc_handle* h, int32_t n_expansions_max) {
    if (!h) return fail(PDMPC_ERR_INVALID, "pdmpc_set_sampled_budget: null handle");
    if (n_expansions_max < 1 || n_expansions_max > PDMPC_SAMPLED_BUDGET_MAX) return fail(PDMPC_ERR_INVALID, "pdmpc_set_sampled_budget: the budget must be in 1..PDMPC_SAMPLED_BUDGET_MAX");
    h->sampled.budget = n_expansions_max;
    return PDMPC_OK;
}

int pdmpc_get_sampled_budget(pdmpc_handle* h, int32_t* n_expansions_max) {
    if (!h || !n_expansions_max) return fail(PDMPC_ERR_INVALID, "pdmpc_get_sampled_budget: null argument");
    *n_expansions_max = h->sampled.budget;
    return PDMPC_OK;
}

const char* pdmpc_last_sampled_kernel(pdmpc_handle* h) { return h ? h->sampled.last_kernel : ""; }

int pdmpc_set_sampled_ensemble(pdmpc_handle* h, int32_t n_members) {
    if (!h) return fail(PDMPC_ERR_INVALID, "pdmpc_set_sampled_ensemble: null handle");
    if (n_members < 1 || n_members > PDMPC_SAMPLED_ENSEMBLE_MAX) return fail(PDMPC_ERR_INVALID, "pdmpc_set_sampled_ensemble: the ensemble size must be in 1..PDMPC_SAMPLED_ENSEMBLE_MAX");
    h->sampled.members = n_members;
    return PDMPC_OK;
}

int pdmpc_get_sampled_ensemble(pdmpc_handle* h, int32_t* n_members) {
    if (!h || !n_members) return fail(PDMPC_ERR_INVALID, "pdmpc_get_sampled_ensemble: null argument");
    *n_members = h->sampled.members;
    return PDMPC_OK;
}

uint32_t pdmpc_sampled_member_seed(uint32_t seed, int32_t member) { return PDMPC_SAMPLED_MEMBER_SEED(seed, member); }

int pdmpc_sampled_ensemble_result(pdmpc_handle* h, int32_t n_vehicles, int32_t* winner, int32_t* member_status, double* member_cost) {
    if (!h) return fail(PDMPC_ERR_INVALID, "pdmpc_sampled_ensemble_result: null handle");
    const PackedStep& B = h->banks[h->bank];
    if (B.pack_failed || !B.sampled.on || B.sampled.members < 2 || h->sampled.ensemble_bank != h->bank) return fail(PDMPC_ERR_INVALID, "pdmpc_sampled_ensemble_result: the current bank was not packed as an ensemble or not launched since");
    if (n_vehicles != B.n_packed) return fail(PDMPC_ERR_INVALID, "pdmpc_sampled_ensemble_result: not the bank's vehicle count");
    ON_DEVICE(h->cfg.device);
    const int E = B.sampled.members;
    std::vector<EnsembleEntry> en((size_t)n_vehicles * (size_t)E);
    std::vector<int32_t> chosen((size_t)n_vehicles);
    if (en.empty()) return PDMPC_OK;
    HIPCHK(hipMemcpyAsync(en.data(), h->sampled.member_entry.p, en.size() * sizeof(EnsembleEntry), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(chosen.data(), h->sampled.chosen.p, chosen.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    for (int v = 0; v < n_vehicles; ++v) {
        const size_t slot = (size_t)(B.perm.empty() ? v : B.inv[(size_t)v]);
        const EnsembleEntry* row = en.data() + slot * (size_t)E;
        for (int e = 0; e < E; ++e) {
            if (member_status) member_status[(size_t)v * E + e] = row[e].status;
            if (member_cost) member_cost[(size_t)v * E + e] = row[e].status == PDMPC_OK ? row[e].cost : std::numeric_limits<double>::infinity();
        }
        if (winner) winner[v] = chosen[slot];
    }
    return PDMPC_OK;
}

int pdmpc_destroy(pdmpc_handle* h) {
    if (!h) return PDMPC_OK;
    DeviceGuard device_guard__(h->cfg.device);
    delete h;
    return PDMPC_OK;
}

int pdmpc_mpa_reach_host(const pdmpc_mpa* mpa, double* dmax, double* amax) {
    if (!mpa || !dmax || !amax || (mpa->n_maneuvers > 0 && !mpa->maneuvers)) return fail(PDMPC_ERR_INVALID, "pdmpc_mpa_reach_host: null argument");
    mpa_reach(mpa, *dmax, *amax);
    return PDMPC_OK;
}

int pdmpc_reach_lists_host(int32_t Hp, double dmax, double amax, double root_x, double root_y, const double* x, const double* y, const int32_t* step_first,
                           const int32_t* step_count, int32_t* list_offset, int32_t* list) {
    if (Hp < 1 || Hp > PDMPC_HP_MAX || !step_first || !step_count || !list_offset) return fail(PDMPC_ERR_INVALID, "pdmpc_reach_lists_host: bad argument");
    std::string err;
    return failed(reach_lists(Hp, dmax, amax, root_x, root_y, x, y, step_first, step_count, list_offset, list, err), err);
}

int pdmpc_mpa_reach_rects_host(const pdmpc_mpa* mpa, int32_t Hp, double* rects) {
    if (!mpa || !rects || !mpa->transition || !mpa->maneuver_index || (mpa->n_maneuvers > 0 && !mpa->maneuvers)) return fail(PDMPC_ERR_INVALID, "pdmpc_mpa_reach_rects_host: null argument");
    if (mpa->n_trims < 1 || Hp < 1 || Hp > PDMPC_HP_MAX || Hp > mpa->Hp) return fail(PDMPC_ERR_INVALID, "pdmpc_mpa_reach_rects_host: Hp out of range");
    mpa_reach_rects(mpa, Hp, rects);
    return PDMPC_OK;
}

int pdmpc_reach_lists_oriented_host(int32_t Hp, int32_t n_trims, const double* rects, int32_t root_trim, double root_x, double root_y, double root_yaw, const double* x, const double* y,
                                    const int32_t* step_first, const int32_t* step_count, int32_t* list_offset, int32_t* list) {
    if (Hp < 1 || Hp > PDMPC_HP_MAX || !rects || root_trim < 1 || root_trim > n_trims || !step_first || !step_count || !list_offset)
        return fail(PDMPC_ERR_INVALID, "pdmpc_reach_lists_oriented_host: bad argument");
    std::string err;
    return failed(reach_lists_oriented(Hp, rects, root_trim, root_x, root_y, root_yaw, x, y, step_first, step_count, list_offset, list, err), err);
}

int pdmpc_upload_mpa(pdmpc_handle* h, const pdmpc_mpa* mpa) {
    if (!h || !mpa) return fail(PDMPC_ERR_INVALID, "null argument");
    if (mpa->n_trims < 1 || mpa->n_trims > 1023) return fail(PDMPC_ERR_INVALID, "n_trims must be in 1..1023");
    if (mpa->Hp < h->cfg.Hp) return fail(PDMPC_ERR_INVALID, "mpa.Hp smaller than config.Hp");
    if (!mpa->transition || !mpa->maneuver_index || (mpa->n_maneuvers > 0 && !mpa->maneuvers)) return fail(PDMPC_ERR_INVALID, "null table");
    ON_DEVICE(h->cfg.device);
    const int n = mpa->n_trims, Hp = h->cfg.Hp;
    LaunchDims sizes{h->cfg.checker, Hp, n};
    mpa_table_sizes(sizes);
    const int nw = sizes.n_words;
    std::vector<uint64_t> mask((size_t)Hp * n * nw + 2, 0);
    for (int k = 0; k < Hp; ++k)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (mpa->transition[((size_t)k * n + i) * n + j]) {
                    const int mi = mpa->maneuver_index[i * n + j];
                    if (mi < 0 || mi >= mpa->n_maneuvers) return fail(PDMPC_ERR_INVALID, "transition allowed but maneuver missing");
                    mask[((size_t)k * n + i) * nw + j / 64] |= 1ull << (j % 64);
                }
    std::vector<int16_t> mi((size_t)n * n + 8, -1);
    for (int i = 0; i < n * n; ++i) mi[i] = (int16_t)mpa->maneuver_index[i];
    const int T = mpa->n_maneuvers;
    std::vector<DevManPose> pose((size_t)std::max(T, 1));
    std::vector<double> area((size_t)std::max(T, 1) * 3 * PDMPC_VMAX * 2 + 2 + (size_t)n * Hp * 4, 0.0);  // (+ the automaton's reach behind the areas: Dmax, Amax, the rectangles)
    for (int t = 0; t < T; ++t) {
        const pdmpc_maneuver& m = mpa->maneuvers[t];
        if (m.n_cols < 2 || m.n_cols > PDMPC_VMAX) return fail(PDMPC_ERR_INVALID, "maneuver area column count out of range");
        pose[t].dx = m.dx;
        pose[t].dy = m.dy;
        pose[t].dyaw = m.dyaw;
        pose[t].n_cols = m.n_cols;
        pose[t].pad = 0;
        const double(*src[3])[PDMPC_VMAX] = {m.area, m.area_without_offset, m.area_large_offset};
        for (int a = 0; a < 3; ++a)
            for (int v = 0; v < m.n_cols; ++v) {
                area[(((size_t)t * 3 + a) * PDMPC_VMAX + v) * 2 + 0] = src[a][0][v];
                area[(((size_t)t * 3 + a) * PDMPC_VMAX + v) * 2 + 1] = src[a][1][v];
            }
    }
    mpa_reach(mpa, area[(size_t)T * 3 * PDMPC_VMAX * 2], area[(size_t)T * 3 * PDMPC_VMAX * 2 + 1]);  // (Dmax, Amax: the graph search's reach lists)
    mpa_reach_rects(mpa, Hp, &area[(size_t)T * 3 * PDMPC_VMAX * 2 + 2]);  // ([trim][step] rectangles of the oriented rule, include/pdmpc_reach.h)
    if (h->d_mask.ensure(mask.size()) || h->d_mi.ensure(mi.size()) || h->d_pose.ensure(pose.size()) || h->d_area.ensure(area.size()))
        return fail(PDMPC_ERR_HIP, "hipMalloc failed for the MPA tables");
    HIPCHK(hipMemcpy(h->d_mask.p, mask.data(), mask.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_mi.p, mi.data(), mi.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_pose.p, pose.data(), pose.size() * sizeof(DevManPose), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_area.p, area.data(), area.size() * 8, hipMemcpyHostToDevice));
    h->n_trims = n;
    h->n_words = nw;
    h->n_man = T;
    h->mask_bytes = sizes.mask_bytes;
    h->mi_bytes = sizes.mi_bytes;
    // B_mpa = 8*T*(3 + 6*VMAX) + n*n*Hp/8
    h->mpa_alg_bytes = (int64_t)8 * T * (3 + 6 * PDMPC_VMAX) + (int64_t)n * n * Hp / 8;
    h->has_mpa = true;
    return PDMPC_OK;
}

int pdmpc_pack_batch(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in) { return pdmpc_pack_step(h, n, in, nullptr, nullptr, nullptr); }

int pdmpc_pack_step(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                    const pdmpc_polygon_set* fallback_shapes) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    ON_DEVICE(h->cfg.device);
    if (pred_offset && !pred_index) return fail(PDMPC_ERR_INVALID, "pred_index missing");
    return pack_common(h, n, in, pred_offset, pred_index, fallback_shapes);
}

int pdmpc_set_step_weights(pdmpc_handle* h, int32_t n, const double* weights) {
    if (!h || n < 0 || (n > 0 && !weights)) return fail(PDMPC_ERR_INVALID, "pdmpc_set_step_weights: bad argument");
    h->next_weights.assign(weights, weights + n);
    return PDMPC_OK;
}

int pdmpc_set_step_seeds(pdmpc_handle* h, int32_t n, const uint32_t* seeds) {
    if (!h || n < 0 || (n > 0 && !seeds)) return fail(PDMPC_ERR_INVALID, "pdmpc_set_step_seeds: bad argument");
    h->sampled.seeds.assign(seeds, n);
    return PDMPC_OK;
}

int pdmpc_launch_packed(pdmpc_handle* h) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    ON_DEVICE(h->cfg.device);
    h->epoch += 1;  // a new step: results of earlier launches no longer satisfy predecessor waits
    return launch_range(h, 0, h->banks[h->bank].n_packed, h->safe_launches);
}

int pdmpc_set_device_share(pdmpc_handle* h, int32_t n_handles) {
    if (!h || n_handles < 1) return fail(PDMPC_ERR_INVALID, "pdmpc_set_device_share: bad argument");
    h->device_share = n_handles;
    return PDMPC_OK;
}

int pdmpc_set_safe_launch(pdmpc_handle* h, int32_t on) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    h->safe_launches = on != 0;
    return PDMPC_OK;
}

int pdmpc_begin_step(pdmpc_handle* h) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    h->epoch += 1;
    return PDMPC_OK;
}

int pdmpc_select_bank(pdmpc_handle* h, int32_t bank) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (bank < 0 || bank >= 4096) return fail(PDMPC_ERR_INVALID, "bank out of range");
    if ((size_t)bank >= h->banks.size()) h->banks.resize((size_t)bank + 1);
    h->bank = bank;
    return PDMPC_OK;
}

int pdmpc_reset_stats(pdmpc_handle* h) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    ON_DEVICE(h->cfg.device);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timer.reset();
    HIPCHK(hipMemsetAsync(h->d_tie_count.p, 0, 4 * sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(h->d_work_count.p, 0, 16 * sizeof(unsigned long long), h->stream));
    return PDMPC_OK;
}

int pdmpc_launch_range(pdmpc_handle* h, int32_t first, int32_t count) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    ON_DEVICE(h->cfg.device);
    return launch_range(h, first, count, h->safe_launches);
}

int pdmpc_synchronize(pdmpc_handle* h) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    ON_DEVICE(h->cfg.device);
    HIPCHK(sync_stream(h));
    return PDMPC_OK;
}

int pdmpc_fetch_results(pdmpc_handle* h, int32_t n, pdmpc_vehicle_out* out) {
    if (!h || (n > 0 && !out)) return fail(PDMPC_ERR_INVALID, "null argument");
    if (n < 0 || n > h->max_vehicles) return fail(PDMPC_ERR_INVALID, "bad record count");
    ON_DEVICE(h->cfg.device);
    PackedStep& B = h->banks[h->bank];
    const bool permuted = !B.perm.empty();
    if (permuted && n != B.n_packed) return fail(PDMPC_ERR_INVALID, "a batch that pdmpc_pack_step put into level order is fetched as a whole");
    if (h->h_out.ensure((size_t)std::max(n, 1))) return fail(PDMPC_ERR_HIP, "hipHostMalloc failed");
    if (n > 0) HIPCHK(hipMemcpyAsync(h->h_out.p, h->d_out.p, (size_t)n * sizeof(pdmpc_vehicle_out), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    // counters + SURVEY.md 8(d) algorithmic bytes of one pass over the packed batch (read where the records landed: pinned memory, slot order)
    const pdmpc_vehicle_out* rec = h->h_out.p;
    pdmpc_stats& s = h->stats;
    const int Hp = h->cfg.Hp;
    const int m = std::min(n, B.n_packed);
    s.n_vehicles = m;
    s.nodes_popped = s.nodes_generated = s.obstacle_columns = 0;
    int64_t bytes = h->mpa_alg_bytes;
    for (int i = 0; i < m; ++i) {
        const pdmpc_vehicle_out& o = rec[i];
        const DevVehicle& d = B.host.veh[i];
        int64_t cols = B.lit_cols[i];
        for (int q = 0; q < d.n_pred; ++q) {
            const int ps = B.host.pred[d.pred_off + q];
            if (ps < n)
                for (int k = 0; k < Hp; ++k) cols += rec[ps].shape_cols[k] + 1;
        }
        const int64_t P = o.n_popped, C = std::max(o.n_expanded - 1, 0);
        s.nodes_popped += P;
        s.nodes_generated += C;
        s.obstacle_columns += cols;
        bytes += 8 * (4 + 3 * Hp) + 16 * cols;                             // B_in
        bytes += P * (60 + 16);                                            // B_pop
        bytes += C * (60 + 16);                                            // B_child
        bytes += 8 * (3 * Hp + Hp + (Hp + 1)) + 16 * PDMPC_VMAX * Hp;      // B_out
    }
    s.algorithmic_bytes = bytes;
    // ONE pass from pinned memory into the caller's array, in the caller's order (the tree_path ids are per search: nothing else refers to slots)
    if (permuted) {
        for (int sl = 0; sl < n; ++sl) out[B.perm[(size_t)sl]] = rec[sl];
    } else if (n > 0) {
        std::memcpy(out, rec, (size_t)n * sizeof(pdmpc_vehicle_out));
    }
    return PDMPC_OK;
}

int pdmpc_fetch_records_at(pdmpc_handle* h, int32_t count, const int32_t* vehicles, pdmpc_vehicle_out* out) {
    if (!h || count < 0 || (count > 0 && (!vehicles || !out))) return fail(PDMPC_ERR_INVALID, "null argument");
    ON_DEVICE(h->cfg.device);
    PackedStep& B = h->banks[h->bank];
    if (h->h_out.ensure((size_t)std::max(count, 1))) return fail(PDMPC_ERR_HIP, "hipHostMalloc failed");
    for (int i = 0; i < count; ++i) {
        const int v = vehicles[i];
        if (v < 0 || v >= B.n_packed) return fail(PDMPC_ERR_INVALID, "vehicle index outside the packed batch");
        const int sl = B.perm.empty() ? v : B.inv[(size_t)v];
        HIPCHK(hipMemcpyAsync(h->h_out.p + i, h->d_out.p + sl, sizeof(pdmpc_vehicle_out), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(sync_stream(h));
    if (count > 0) std::memcpy(out, h->h_out.p, (size_t)count * sizeof(pdmpc_vehicle_out));
    return PDMPC_OK;
}

namespace {
// What a caller that keeps only a few of a batch's plans needs of ALL of them (the explorative step: the choice among the
// prioritizations rests on the cost-to-come of every vehicle's final node, PrioritizedExplorativeController.m:94-112): status and
// path_nodes[Hp][4] per vehicle, as two strided copies — 12 bytes per record instead of 2.9 KB.  Caller's order.
int fetch_lean(pdmpc_handle* h, int32_t n, int32_t* status, double* cost) {
    PackedStep& B = h->banks[h->bank];
    const bool permuted = !B.perm.empty();
    if (permuted && n != B.n_packed) return fail(PDMPC_ERR_INVALID, "a batch that pdmpc_pack_step put into its own order is fetched as a whole");
    if (h->h_lean.ensure((size_t)std::max(n, 1) * 2)) return fail(PDMPC_ERR_HIP, "hipHostMalloc failed");
    if (h->d_lean.ensure((size_t)std::max(n, 1) * 2)) return fail(PDMPC_ERR_HIP, "hipMalloc failed");
    if (n > 0) {
        const int lrc = pdmpc_launch_gather_lean(h->d_out.p, n, h->cfg.Hp, h->d_lean.p, (void*)h->stream);
        if (lrc) return fail(PDMPC_ERR_HIP, "gather kernel launch failed");
        HIPCHK(hipMemcpyAsync(h->h_lean.p, h->d_lean.p, (size_t)n * 16, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(sync_stream(h));
    for (int sl = 0; sl < n; ++sl) {
        const int v = permuted ? B.perm[(size_t)sl] : sl;
        cost[v] = h->h_lean.p[2 * (size_t)sl];
        std::memcpy(&status[v], &h->h_lean.p[2 * (size_t)sl + 1], sizeof(int32_t));
    }
    return PDMPC_OK;
}

// ---- the choice among the plans of a batch (pdmpc_choice, include/pdmpc.h; choice_kernel.hip)

// The lists of a checked choice on the n records of the current bank, staged in pinned memory with the caller's slots mapped to the
// bank's (a batch that pack_common put into its own order) and queued for the device; A: what the kernels take.
int stage_choice(pdmpc_handle* h, int32_t n, const pdmpc_choice& ch, const ChoiceLayout& L, ChoiceArgs& A) {
    const PackedStep& B = h->banks[h->bank];
    const bool permuted = !B.perm.empty();
    if (permuted ? n != B.n_packed : n > h->max_vehicles) return fail(PDMPC_ERR_INVALID, "pdmpc_choice: the batch is not the one resident in this bank");
    ChoiceState& S = h->choice;
    const ChoiceLists W(ch);
    const bool first_use = !S.tally.p;
    if (S.h_in.ensure(W.words) || S.h_out.ensure(L.bytes)) return fail(PDMPC_ERR_HIP, "hipHostMalloc failed for the choice");
    if (S.in.ensure(W.words) || S.out.ensure(L.bytes) || S.tally.ensure(PDMPC_CHOICE_COUNTERS)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the choice");
    if (first_use) HIPCHK(hipMemsetAsync(S.tally.p, 0, PDMPC_CHOICE_COUNTERS * sizeof(int32_t), h->stream));
    stage_choice_lists(ch, W, S.h_in.p, [&](const int32_t* slot, int count, int32_t* to) {
        for (int q = 0; q < count; ++q) to[q] = permuted ? B.inv[(size_t)slot[q]] : slot[q];
    });
    HIPCHK(hipMemcpyAsync(S.in.p, S.h_in.p, W.words * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    A = ChoiceArgs{};
    A.rec = h->d_out.p;
    A.n = n;
    A.Hp = h->cfg.Hp;
    A.n_cells = ch.n_cells;
    A.n_graphs = ch.n_graphs;
    A.n_picks = ch.n_picks;
    A.first_graph_cell = ch.n_graphs > 0 ? ch.graph_offset[0] : 0;
    A.end_graph_cell = ch.n_graphs > 0 ? ch.graph_offset[ch.n_graphs] : 0;
    A.cell_offset = S.in.p + W.cell_offset;
    A.cell_slot = S.in.p + W.cell_slot;
    A.graph_offset = S.in.p + W.graph_offset;
    A.pick_graph = S.in.p + W.pick_graph;
    A.pick_offset = S.in.p + W.pick_offset;
    A.pick_slot = S.in.p + W.pick_slot;
    A.tally = S.tally.p;
    A.counters = (int32_t*)S.out.p;
    A.chosen = (int32_t*)(S.out.p + L.chosen);
    A.cell_cost = (double*)(S.out.p + L.cell_cost);
    A.picks = (pdmpc_vehicle_out*)(S.out.p + L.picks);
    return PDMPC_OK;
}

// the two launches behind whatever the stream holds (the search's launch: no host synchronisation in between), ONE copy back, one wait
int fetch_choice(pdmpc_handle* h, const ChoiceArgs& A, const ChoiceLayout& L) {
    ChoiceState& S = h->choice;
    for (hipEvent_t& e : S.timed.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(S.timed.ev[0], h->stream));
    const int lrc = pdmpc_launch_choice(&A, (void*)h->stream);
    if (lrc) return fail(PDMPC_ERR_HIP, std::string("choice kernel launch failed: ") + hipGetErrorString((hipError_t)lrc));
    HIPCHK(hipEventRecord(S.timed.ev[1], h->stream));
    HIPCHK(hipMemcpyAsync(S.h_out.p, S.out.p, L.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    S.timed.fold();
    return PDMPC_OK;
}

// a fetched choice into the caller's arrays (choice_host.hpp), or why it is none
int deliver_fetched(const pdmpc_handle* h, const pdmpc_choice& ch, const ChoiceLayout& L, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks) {
    std::string err;
    return deliver_choice(ch, L, h->choice.h_out.p, chosen, cell_cost, picks, err) ? PDMPC_OK : fail(PDMPC_ERR_HIP, err);
}

// Where a plan's read-back lands: every record, (lean) the (status, cost) pair of every vehicle (fetch_lean), or (chosen) the block of
// a choice made on the device (fetch_choice).  Caller's order.
struct Sink {
    enum Kind { kRecords, kLean, kChosen } kind;
    pdmpc_vehicle_out* out;
    int32_t* status;
    double* cost;
    const ChoiceArgs* choice;
    const ChoiceLayout* layout;
    static Sink records(pdmpc_vehicle_out* out) { return {kRecords, out, nullptr, nullptr, nullptr, nullptr}; }
    static Sink lean_pair(int32_t* status, double* cost) { return {kLean, nullptr, status, cost, nullptr, nullptr}; }
    static Sink chosen(const ChoiceArgs* choice, const ChoiceLayout* layout) { return {kChosen, nullptr, nullptr, nullptr, choice, layout}; }
    int fetch(pdmpc_handle* h, int32_t n) const {
        if (kind == kChosen) return fetch_choice(h, *choice, *layout);
        return kind == kLean ? fetch_lean(h, n, status, cost) : pdmpc_fetch_results(h, n, out);
    }
    // which of the batch's records outgrew their arena / gave up waiting for a predecessor: from the records' statuses, or (chosen)
    // from the counters the choice kept on the device
    void verdict(const pdmpc_handle* h, int32_t n, bool& overflow, bool& timed_out) const {
        overflow = timed_out = false;
        if (kind == kChosen) {
            const int32_t* counters = (const int32_t*)h->choice.h_out.p;
            overflow = counters[PDMPC_CHOICE_OVERFLOW] != 0;
            timed_out = counters[PDMPC_CHOICE_TIMED_OUT] != 0;
            return;
        }
        for (int i = 0; i < n; ++i) {
            const int st = kind == kLean ? status[i] : out[i].status;
            overflow = overflow || st == PDMPC_ARENA_OVERFLOW;
            timed_out = timed_out || st == PDMPC_ERR_HIP;
        }
    }
};

// Arenas of `nodes` nodes per vehicle, or (grown == false) the ones there were if HBM has no room for them.
int realloc_arenas(pdmpc_handle* h, uint32_t nodes, bool& grown) {
    HIPCHK(hipStreamSynchronize(h->stream));
    const uint32_t before = h->arena.max_nodes;
    grown = h->arena.alloc(h->max_vehicles, nodes, h->cfg.Hp) == 0;
    if (!grown && h->arena.alloc(h->max_vehicles, before, h->cfg.Hp)) return fail(PDMPC_ERR_HIP, "hipMalloc failed while restoring the arenas");
    return PDMPC_OK;
}

// The reference's tree grows without bound (Tree.m:54-70); the arenas here are finite.  A call whose search outgrows them
// is planned again from scratch with arenas twice as large (searches are deterministic, so the vehicles that did fit
// produce the same records again) until it fits, the limit set with pdmpc_set_arena_limit is reached, or HBM runs out.
// grown == false: the arenas stay as they are and the records' statuses report the overflow.
int grow_after_overflow(pdmpc_handle* h, bool& grown) {
    grown = false;
    const uint64_t next = (uint64_t)h->arena.max_nodes * 2u;
    if ((h->max_nodes_limit && next > h->max_nodes_limit) || next > (1ull << 30)) return PDMPC_OK;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const size_t per_node = h->arena.bytes_per_node(h->cfg.Hp);
    const size_t have = (size_t)h->max_vehicles * h->arena.max_nodes * per_node;
    if ((size_t)h->max_vehicles * next * per_node > free_b + have) return PDMPC_OK;  // no room to grow
    const int rc = realloc_arenas(h, (uint32_t)next, grown);
    if (grown) h->arena_regrows += 1;
    return rc;
}

// `launch(safe)` enqueues what the call plans.  search: the searches (or sampled plans) of the packed bank, whose records can carry the
// watchdog's status; else pdmpc_plan_joint's problems, which have no predecessors to wait for, no time-out path and no debug lines.
extern "C++" template <class Launch>  // (this namespace sits inside the extern "C" block)
int plan_growing(pdmpc_handle* h, int32_t n, const Sink& sink, bool search, Launch&& launch) {
    bool safe = h->safe_launches;
    for (;;) {
        const bool dbg = search && h->tune.debug_host == 1;
        if (dbg) fprintf(stderr, "pdmpc: launching %d vehicles, arena %u nodes%s\n", n, h->arena.max_nodes, safe ? " (resident slices)" : "");
        ON_DEVICE(h->cfg.device);
        const auto t0 = std::chrono::steady_clock::now();
        int rc = launch(safe);
        if (rc) return rc;
        const auto t1 = std::chrono::steady_clock::now();
        rc = sink.fetch(h, n);
        if (rc) return rc;
        h->last_us[1] += std::chrono::duration<double, std::micro>(t1 - t0).count();
        h->last_us[2] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
        if (search && h->tune.debug_host == 2) {  // (PDMPC_DEBUG_HOST=2: where a call's host time goes, printed by pdmpc_plan_step_literal)
            h->dbg_us[1] += std::chrono::duration<double, std::micro>(t1 - t0).count();
            h->dbg_us[2] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
            float ms = 0.f;
            if (h->timer.last_ms(ms)) h->dbg_us[3] += 1e3 * ms;
        }
        bool overflow = false, timed_out = false;
        sink.verdict(h, n, overflow, timed_out);
        timed_out = timed_out && search;
        if (dbg) fprintf(stderr, "pdmpc: fetched, overflow %d, timed out %d\n", (int)overflow, (int)timed_out);
        if (timed_out && safe)
            return fail(PDMPC_ERR_HIP, "a search gave up waiting for a predecessor although the call was planned in resident slices without helper workgroups (records carry PDMPC_ERR_HIP)");
        if (timed_out && !safe) {
            // A search gave up waiting for a predecessor of the same launch (the kernel's watchdog): the launch was
            // oversubscribed and the dispatch order starved a predecessor, or a helper sat where a search should have run.  Plan
            // the call again in slices that are resident as a whole: forward progress then rests on nothing but slot order.
            safe = true;
            h->safe_replans += 1;
            continue;
        }
        if (!overflow) return PDMPC_OK;
        bool grown = false;
        if ((rc = grow_after_overflow(h, grown))) return rc;
        if (!grown) return PDMPC_OK;  // statuses tell
    }
}

// ... of the bank's searches: every attempt is a new step
int plan_packed_growing(pdmpc_handle* h, int32_t n, const Sink& sink) {
    return plan_growing(h, n, sink, true, [h](bool safe) {
        h->epoch += 1;  // a new step: results of earlier launches no longer satisfy predecessor waits
        return launch_range(h, 0, h->banks[h->bank].n_packed, safe);
    });
}

// The prologue of pdmpc_plan_batch / _step / _step_lean / _joint: the pack, timed for pdmpc_last_call_timing.
int timed_pack(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index, const pdmpc_polygon_set* fallback_shapes) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = pdmpc_pack_step(h, n, in, pred_offset, pred_index, fallback_shapes);
    if (rc) return rc;
    h->last_us[0] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    h->last_us[1] = h->last_us[2] = 0;
    return PDMPC_OK;
}
}  // namespace

int pdmpc_plan_batch(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, pdmpc_vehicle_out* out) {
    if (n > 0 && !out) return fail(PDMPC_ERR_INVALID, "null argument");
    const int rc = timed_pack(h, n, in, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (h->tune.debug_host == 2) h->dbg_us[0] += h->last_us[0];
    return plan_packed_growing(h, n, Sink::records(out));
}

int pdmpc_plan_step(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                    const pdmpc_polygon_set* fallback_shapes, pdmpc_vehicle_out* out) {
    if (n > 0 && !out) return fail(PDMPC_ERR_INVALID, "null argument");
    const int rc = timed_pack(h, n, in, pred_offset, pred_index, fallback_shapes);
    return rc ? rc : plan_packed_growing(h, n, Sink::records(out));
}

int pdmpc_plan_step_lean(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index, const pdmpc_polygon_set* fallback_shapes,
                         int32_t* status, double* final_cost) {
    if (!h || n < 0 || (n > 0 && (!status || !final_cost))) return fail(PDMPC_ERR_INVALID, "null argument");
    const int rc = timed_pack(h, n, in, pred_offset, pred_index, fallback_shapes);
    return rc ? rc : plan_packed_growing(h, n, Sink::lean_pair(status, final_cost));
}

int pdmpc_choose_host(int32_t n, const int32_t* status, const double* final_cost, const pdmpc_choice* ch, int32_t* chosen, double* cell_cost) {
    if (n > 0 && (!status || !final_cost)) return fail(PDMPC_ERR_INVALID, "null argument");
    if (const int rc = checked_choice(n, ch)) return rc;
    for (int i = 0; i < n; ++i)
        if (status[i] != PDMPC_OK && status[i] != PDMPC_EXHAUSTED) return fail(PDMPC_ERR_HIP, "a result record carries an error status: not a planning result");
    choose_host(status, final_cost, ch, chosen, cell_cost);
    return PDMPC_OK;
}

int pdmpc_choose_resident(pdmpc_handle* h, int32_t n, const pdmpc_choice* ch, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks) {
    if (!h || (ch && ch->n_picks > 0 && !picks)) return fail(PDMPC_ERR_INVALID, "null argument");
    if (const int rc = checked_choice(n, ch)) return rc;
    ON_DEVICE(h->cfg.device);
    const ChoiceLayout L(*ch);
    ChoiceArgs A;
    int rc = stage_choice(h, n, *ch, L, A);
    if (!rc) rc = fetch_choice(h, A, L);
    return rc ? rc : deliver_fetched(h, *ch, L, chosen, cell_cost, picks);
}

int pdmpc_plan_step_chosen(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index, const pdmpc_polygon_set* fallback_shapes,
                           const pdmpc_choice* ch, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks) {
    if (!h || (ch && ch->n_picks > 0 && !picks)) return fail(PDMPC_ERR_INVALID, "null argument");
    if (const int rc = checked_choice(n, ch)) return rc;
    int rc = timed_pack(h, n, in, pred_offset, pred_index, fallback_shapes);
    if (rc) return rc;
    ON_DEVICE(h->cfg.device);
    const ChoiceLayout L(*ch);
    ChoiceArgs A;
    rc = stage_choice(h, n, *ch, L, A);  // (once: a launch that is repeated with larger arenas or in slices chooses on the same lists)
    if (!rc) rc = plan_packed_growing(h, n, Sink::chosen(&A, &L));
    return rc ? rc : deliver_fetched(h, *ch, L, chosen, cell_cost, picks);
}

int pdmpc_choice_kernel_ms(pdmpc_handle* h, double* ms) {
    if (!h || !ms) return fail(PDMPC_ERR_INVALID, "null argument");
    *ms = h->choice.timed.ms;
    return PDMPC_OK;
}

int pdmpc_last_call_timing(pdmpc_handle* h, double* us3) {
    if (!h || !us3) return fail(PDMPC_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; ++i) us3[i] = h->last_us[i];
    return PDMPC_OK;
}

// The step as an UNMODIFIED reference controller drives this backend (GraphSearchHip.m behind OptimizerInterface): one
// run_optimizer call per vehicle (PrioritizedController.m:335-341) in kahn order (PrioritizedSequentialController.m:77-94), every
// call a pdmpc_plan_batch of one vehicle -- pack, H2D, launch, D2H -- and the hand-over of solved areas on the host
// (PrioritizedController.m:476-491: the predecessors' info.shapes(1, :), or their published fallback areas, appended to the
// vehicle's dynamic obstacles).  Same arguments and records as pdmpc_plan_step; slots must be in level order.
int pdmpc_plan_step_literal(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                            const pdmpc_polygon_set* fallback_shapes, pdmpc_vehicle_out* out) {
    if (!h || n < 0 || (n > 0 && (!in || !out))) return fail(PDMPC_ERR_INVALID, "null argument");
    if (pred_offset && !pred_index) return fail(PDMPC_ERR_INVALID, "pred_index missing");
    const int Hp = h->cfg.Hp;
    std::vector<int32_t> off;
    std::vector<double> xs, ys;
    for (int s = 0; s < n; ++s) {
        pdmpc_vehicle_in v = in[s];
        const int np = pred_offset ? pred_offset[s + 1] - pred_offset[s] : 0;
        if (np > 0) {
            const pdmpc_polygon_set& d = in[s].dynamic_obstacles;
            if (d.n_polygons % Hp) return fail(PDMPC_ERR_INVALID, "dynamic_obstacles must hold n_d * Hp polygons");
            off.assign(1, 0);
            xs.clear();
            ys.clear();
            auto push_poly = [&](const double* px, const double* py, int cnt) {
                xs.insert(xs.end(), px, px + cnt);
                ys.insert(ys.end(), py, py + cnt);
                off.push_back((int32_t)xs.size());
            };
            for (int p = 0; p < d.n_polygons; ++p) push_poly(d.x + d.offset[p], d.y + d.offset[p], d.offset[p + 1] - d.offset[p]);
            int rows = d.n_polygons / Hp;
            for (int e = pred_offset[s]; e < pred_offset[s + 1]; ++e) {
                const int ps = pred_index[e];
                if (ps < 0 || ps >= s) return fail(PDMPC_ERR_INVALID, "pdmpc_plan_step_literal needs the slots in level order");
                const pdmpc_vehicle_out& po = out[ps];
                if (po.status == PDMPC_OK) {
                    for (int k = 0; k < Hp; ++k) push_poly(po.shapes[k][0], po.shapes[k][1], po.shape_cols[k]);
                    rows += 1;
                } else if (fallback_shapes && fallback_shapes[ps].n_polygons == Hp) {
                    const pdmpc_polygon_set& fb = fallback_shapes[ps];
                    for (int k = 0; k < Hp; ++k) push_poly(fb.x + fb.offset[k], fb.y + fb.offset[k], fb.offset[k + 1] - fb.offset[k]);
                    rows += 1;
                }
            }
            static const double zero = 0.0;
            v.dynamic_obstacles.n_polygons = rows * Hp;
            v.dynamic_obstacles.offset = off.data();
            v.dynamic_obstacles.x = xs.empty() ? &zero : xs.data();
            v.dynamic_obstacles.y = ys.empty() ? &zero : ys.data();
        }
        int rc = pdmpc_plan_batch(h, 1, &v, out + s);
        if (rc) return rc;
        // the single-launch path publishes the fallback areas of an exhausted vehicle in its record: the same record here
        if (out[s].status == PDMPC_EXHAUSTED && fallback_shapes && fallback_shapes[s].n_polygons == Hp) {
            const pdmpc_polygon_set& fb = fallback_shapes[s];
            for (int k = 0; k < Hp; ++k) {
                const int cnt = std::min(fb.offset[k + 1] - fb.offset[k], (int32_t)PDMPC_VMAX);
                out[s].shape_cols[k] = cnt;
                for (int c = 0; c < cnt; ++c) {
                    out[s].shapes[k][0][c] = fb.x[fb.offset[k] + c];
                    out[s].shapes[k][1][c] = fb.y[fb.offset[k] + c];
                }
            }
        }
    }
    if (h->tune.debug_host == 2) {
        fprintf(stderr, "pdmpc: literal step of %d calls: pack %.0f us, launch %.0f us, fetch (incl. waiting for the kernel) %.0f us, kernels %.0f us\n", n, h->dbg_us[0], h->dbg_us[1],
                h->dbg_us[2], h->dbg_us[3]);
        h->dbg_us[0] = h->dbg_us[1] = h->dbg_us[2] = h->dbg_us[3] = 0;
    }
    return PDMPC_OK;
}

int pdmpc_get_config(pdmpc_handle* h, pdmpc_config* config, int32_t* mpa_uploaded) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (config) {
        *config = h->cfg;
        config->max_vehicles = h->max_vehicles;
        config->max_nodes = (int32_t)h->arena.max_nodes;
    }
    if (mpa_uploaded) *mpa_uploaded = h->has_mpa ? 1 : 0;
    return PDMPC_OK;
}

int pdmpc_set_arena_limit(pdmpc_handle* h, int32_t max_nodes_limit) {
    if (!h || max_nodes_limit < 0) return fail(PDMPC_ERR_INVALID, "bad argument");
    h->max_nodes_limit = (uint32_t)max_nodes_limit;
    return PDMPC_OK;
}

int pdmpc_grow_arena(pdmpc_handle* h, int32_t max_nodes) {
    if (!h || max_nodes <= 0) return fail(PDMPC_ERR_INVALID, "bad argument");
    ON_DEVICE(h->cfg.device);
    if ((uint32_t)max_nodes <= h->arena.max_nodes) return PDMPC_OK;
    bool grown = false;
    const int rc = realloc_arenas(h, (uint32_t)max_nodes, grown);
    if (rc || grown) return rc;
    return fail(PDMPC_ERR_CAPACITY, "not enough HBM for arenas of that size");
}

int pdmpc_arena_nodes(pdmpc_handle* h, int32_t* max_nodes, int64_t* regrows) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (max_nodes) *max_nodes = (int32_t)h->arena.max_nodes;
    if (regrows) *regrows = h->arena_regrows;
    return PDMPC_OK;
}

// One computation level: a sampled bank without predecessors (the kernel draws every slot's random numbers itself).
int pdmpc_plan_batch_sampled(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const uint32_t* seeds, pdmpc_vehicle_out* out) {
    if (!h || n < 0 || (n > 0 && (!in || !seeds || !out))) return fail(PDMPC_ERR_INVALID, "null argument");
    int rc = pdmpc_set_step_seeds(h, n, seeds);
    if (rc) return rc;
    if ((rc = pdmpc_pack_batch(h, n, in))) return rc;
    if (n == 0) return PDMPC_OK;
    ON_DEVICE(h->cfg.device);
    return plan_packed_growing(h, n, Sink::records(out));
}

// A whole time step of the sampled optimizer: seeds for the next pack, then pdmpc_plan_step (one launch; predecessors' areas handed
// over on the device; the recovery in resident slices after a watchdog time-out).
int pdmpc_plan_step_sampled(pdmpc_handle* h, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                            const pdmpc_polygon_set* fallback_shapes, const uint32_t* seeds, pdmpc_vehicle_out* out) {
    if (!h || n < 0 || (n > 0 && (!seeds || !out))) return fail(PDMPC_ERR_INVALID, "pdmpc_plan_step_sampled: bad argument");
    const int rc = pdmpc_set_step_seeds(h, n, seeds);
    return rc ? rc : pdmpc_plan_step(h, n, in, pred_offset, pred_index, fallback_shapes, out);
}

int pdmpc_plan_joint(pdmpc_handle* h, int32_t n_problems, const int32_t* problem_offset, const pdmpc_vehicle_in* in, pdmpc_vehicle_out* out) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (h->cfg.checker != PDMPC_CHECK_SAT) return fail(PDMPC_ERR_INVALID, "pdmpc_plan_joint: joint searches use the separating-axis checker (PDMPC_CHECK_SAT)");
    if (n_problems < 0 || (n_problems > 0 && !problem_offset)) return fail(PDMPC_ERR_INVALID, "pdmpc_plan_joint: bad problem list");
    if (n_problems > 0 && problem_offset[0] != 0) return fail(PDMPC_ERR_INVALID, "pdmpc_plan_joint: problem_offset[0] must be 0");
    for (int p = 0; p < n_problems; ++p) {
        const int m = problem_offset[p + 1] - problem_offset[p];
        if (m < 1 || m > PDMPC_JOINT_MAX) return fail(PDMPC_ERR_INVALID, "pdmpc_plan_joint: a problem holds 1 to PDMPC_JOINT_MAX vehicles");
    }
    const int n = n_problems > 0 ? problem_offset[n_problems] : 0;
    if (n > 0 && (!in || !out)) return fail(PDMPC_ERR_INVALID, "pdmpc_plan_joint: null vehicle or record array");
    ON_DEVICE(h->cfg.device);
    int rc = timed_pack(h, n, in, nullptr, nullptr, nullptr);
    if (rc || n == 0) return rc;
    PackedStep& B = h->banks[h->bank];
    LaunchDims dims = launch_dims(h, B);
    dims.soup_cap = 0;
    // every distinct soup and boundary of a problem once: what the kernel's prologue stages (pdmpc_device.h: the rule of both)
    for (int p = 0; p < n_problems; ++p)
        dims.soup_cap = std::max(dims.soup_cap, pdmpc_joint_soup_columns(B.host.veh + problem_offset[p], problem_offset[p + 1] - problem_offset[p], dims.Hp));
    dims.soup_cap += 2;
    LaunchPlan plan;
    std::string err;
    if ((rc = plan_launch(h->tune, dims, kPlanJoint, n_problems, 0, false, plan, err))) return fail(rc, err);
    if (h->d_joint_off.ensure((size_t)n_problems + 1)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the problem offsets");
    HIPCHK(hipMemcpyAsync(h->d_joint_off.p, problem_offset, ((size_t)n_problems + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    // (an arena too small for some problem: the call is planned again with arenas twice as large, pdmpc_plan_batch's rule)
    rc = plan_growing(h, n, Sink::records(out), false, [&](bool) -> int {
        JointArgs a{};
        set_batch_args(h, B, plan.areas_in_lds, a);
        a.dt = h->cfg.dt_seconds;
        a.max_nodes = h->arena.max_nodes;
        a.problem_off = h->d_joint_off.p;
        a.nodes = h->arena.nodes.p;
        a.far_key = h->arena.far_key.p;
        a.far_id = h->arena.far_id.p;
        a.heap_lds = plan.heap_lds;
        a.lds = plan.joint;
        if (const int trc = h->timer.begin(h->stream, kLaunchJoint)) return trc;
        const int lrc = pdmpc_launch_joint(&a, n_problems, (void*)h->stream);
        if (lrc != 0) {
            char buf[256];
            snprintf(buf, sizeof buf, "joint kernel launch failed: %s (LDS %u B)", hipGetErrorString((hipError_t)lrc), plan.joint.total);
            return fail(PDMPC_ERR_HIP, buf);
        }
        return h->timer.end(h->stream);
    });
    if (rc) return rc;
    // counters per problem (every vehicle's record carries its problem's n_popped / n_expanded); the per-plan byte formula and
    // obstacle-column count that pdmpc_fetch_results evaluates are the single-vehicle search's and do not
    // describe a joint search: they are reported as 0
    pdmpc_stats& s = h->stats;
    s.n_vehicles = n;
    s.obstacle_columns = 0;
    s.algorithmic_bytes = 0;
    s.nodes_popped = s.nodes_generated = 0;
    for (int p = 0; p < n_problems; ++p) {
        const pdmpc_vehicle_out& o = out[problem_offset[p]];
        s.nodes_popped += o.n_popped;
        s.nodes_generated += std::max(o.n_expanded - 1, 0);
    }
    s.lds_bytes = plan.joint.total;
    s.lds_nodes = 0;
    return PDMPC_OK;
}

int pdmpc_result_device_buffer(pdmpc_handle* h, void** dev_ptr, size_t* nbytes) {
    if (!h || !dev_ptr || !nbytes) return fail(PDMPC_ERR_INVALID, "null argument");
    if (int rc = check_result_slots(h, 0, 0)) return rc;
    *dev_ptr = h->d_out.p;
    *nbytes = (size_t)h->max_vehicles * sizeof(pdmpc_vehicle_out);
    return PDMPC_OK;
}

int pdmpc_import_results(pdmpc_handle* h, int32_t first, int32_t n, const void* dev_records) {
    if (!h || (n > 0 && !dev_records)) return fail(PDMPC_ERR_INVALID, "null argument");
    if (int rc = check_result_slots(h, first, n)) return rc;
    ON_DEVICE(h->cfg.device);
    if (n == 0) return PDMPC_OK;
    const void* dst = (const void*)(h->d_out.p + first);
    if (dev_records != dst)
        HIPCHK(hipMemcpyAsync(h->d_out.p + first, dev_records, (size_t)n * sizeof(pdmpc_vehicle_out), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(h->d_flag.p + first), (int)h->epoch, (size_t)n, h->stream));
    return PDMPC_OK;
}

int pdmpc_export_results(pdmpc_handle* h, int32_t first, int32_t n, void* dev_records) {
    const int rc = pdmpc_export_results_async(h, first, n, dev_records);
    if (rc) return rc;
    ON_DEVICE(h->cfg.device);
    HIPCHK(hipStreamSynchronize(h->stream));
    return PDMPC_OK;
}

int pdmpc_export_results_async(pdmpc_handle* h, int32_t first, int32_t n, void* dev_records) {
    if (!h || (n > 0 && !dev_records)) return fail(PDMPC_ERR_INVALID, "null argument");
    if (int rc = check_result_slots(h, first, n)) return rc;
    ON_DEVICE(h->cfg.device);
    if (n > 0) HIPCHK(hipMemcpyAsync(dev_records, h->d_out.p + first, (size_t)n * sizeof(pdmpc_vehicle_out), hipMemcpyDeviceToDevice, h->stream));
    return PDMPC_OK;
}

int pdmpc_stream(pdmpc_handle* h, void** hip_stream) {
    if (!h || !hip_stream) return fail(PDMPC_ERR_INVALID, "null argument");
    *hip_stream = (void*)h->stream;
    return PDMPC_OK;
}

int pdmpc_debug_counters(pdmpc_handle* h, uint64_t* out16) {
    if (!h || !out16) return fail(PDMPC_ERR_INVALID, "null argument");
    ON_DEVICE(h->cfg.device);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out16, h->d_work_count.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PDMPC_OK;
}

int pdmpc_debug_packed_offsets(pdmpc_handle* h, int32_t vehicle, int32_t* lit_off, int32_t* hdv_off, int32_t* ll2) {
    if (!h || !lit_off || !hdv_off || !ll2) return fail(PDMPC_ERR_INVALID, "null argument");
    const PackedStep& B = h->banks[h->bank];
    if (B.pack_failed || vehicle < 0 || vehicle >= B.n_packed) return fail(PDMPC_ERR_INVALID, "pdmpc_debug_packed_offsets: no such vehicle in the packed batch");
    const DevVehicle& d = B.host.veh[B.inv.empty() ? vehicle : B.inv[(size_t)vehicle]];
    for (int k = 0; k <= h->cfg.Hp; ++k) {
        lit_off[k] = d.lit_off[k];
        hdv_off[k] = d.hdv_off[k];
    }
    ll2[0] = d.ll_off;
    ll2[1] = d.ll_len;
    return PDMPC_OK;
}

int pdmpc_get_last_stats(pdmpc_handle* h, pdmpc_stats* stats) {
    if (!h || !stats) return fail(PDMPC_ERR_INVALID, "null argument");
    ON_DEVICE(h->cfg.device);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (int rc = h->timer.total(h->stats.kernel_ms, h->stats.n_launches)) return rc;
    int32_t ctr[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(ctr, h->d_tie_count.p, sizeof ctr, hipMemcpyDeviceToHost));
    h->stats.queue_fallbacks = ctr[0];
    h->stats.speculation_arrivals = ctr[2];
    unsigned long long work[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpy(work, h->d_work_count.p, sizeof work, hipMemcpyDeviceToHost));
    h->stats.edge_checks = (int64_t)work[0];
    h->stats.segment_pair_tests = (int64_t)work[1];
    h->stats.kernel = h->timer.kind;
    h->stats.nodes_processed = (int64_t)work[2];
    h->stats.rounds = (int64_t)work[3];
    h->stats.shared_rounds = (int64_t)work[4];
    h->stats.helper_checked = (int64_t)work[5];
    h->stats.safe_replans = h->safe_replans;
    h->stats.bad_status_plans = (int64_t)work[6];
    *stats = h->stats;
    return PDMPC_OK;
}

// ---- the debug calls that run one kernel on the caller's arrays: pdmpc_debug_random_numbers, _heap_script, _edge_check, _interx_soups, _sincos
namespace {
// One array of such a call: n elements of the caller's, copied to the device before the launch (T const: an operand) or back from it after the
// launch (an output); on the device it has max(n, count) elements, exactly (DevBuf::ensure_exact).
extern "C++" template <class T>  // (this namespace sits inside the extern "C" block)
struct Staged {
    T* host;
    size_t n, count = 0;
    DevBuf<std::remove_const_t<T>> dev;
};

// The recipe of those calls: the device buffers, the non-empty operands up, `launch` on the handle's stream, a wait for it, the outputs back.
extern "C++" template <class Launch, class... T>
int run_staged(pdmpc_handle* h, const char* malloc_failed, const char* launch_failed, Launch&& launch, Staged<T>&... bufs) {
    if ((0 | ... | bufs.dev.ensure_exact(std::max(bufs.n, bufs.count)))) return fail(PDMPC_ERR_HIP, malloc_failed);
    hipError_t e = hipSuccess;
    auto copy = [&e](auto& b, bool up) {
        typedef std::remove_pointer_t<decltype(b.host)> Elem;
        if (e != hipSuccess || !b.n || up != std::is_const<Elem>::value) return;
        e = up ? hipMemcpy(b.dev.p, b.host, b.n * sizeof(Elem), hipMemcpyHostToDevice) : hipMemcpy((void*)b.host, b.dev.p, b.n * sizeof(Elem), hipMemcpyDeviceToHost);
    };
    (copy(bufs, true), ...);
    HIPCHK(e);
    if (launch() != 0) return fail(PDMPC_ERR_HIP, launch_failed);
    HIPCHK(hipStreamSynchronize(h->stream));
    (copy(bufs, false), ...);
    HIPCHK(e);
    return PDMPC_OK;
}
}  // namespace

int pdmpc_debug_random_numbers(pdmpc_handle* h, int32_t count, const uint32_t* seeds, int32_t n, double* out) {
    if (!h || count < 0 || n < 0 || n > 4000 || (count > 0 && n > 0 && (!seeds || !out))) return fail(PDMPC_ERR_INVALID, "pdmpc_debug_random_numbers: bad argument");
    if (count == 0 || n == 0) return PDMPC_OK;
    ON_DEVICE(h->cfg.device);
    Staged<const uint32_t> d_seeds{seeds, (size_t)count};
    Staged<double> d_out{out, (size_t)count * n};
    auto launch = [&] { return pdmpc_launch_debug_mt19937(d_seeds.dev.p, count, n, d_out.dev.p, (void*)h->stream); };
    return run_staged(h, "hipMalloc failed for the generator test", "generator launch failed", launch, d_seeds, d_out);
}

int pdmpc_debug_random_stream(pdmpc_handle* h, int32_t count, const uint32_t* seeds, int32_t n, double* out) {
    if (!h || count < 0 || n < 0 || (count > 0 && n > 0 && (!seeds || !out))) return fail(PDMPC_ERR_INVALID, "pdmpc_debug_random_stream: bad argument");
    if (count == 0 || n == 0) return PDMPC_OK;
    ON_DEVICE(h->cfg.device);
    Staged<const uint32_t> d_seeds{seeds, (size_t)count};
    Staged<double> d_out{out, (size_t)count * n};
    auto launch = [&] { return pdmpc_launch_debug_random_stream(d_seeds.dev.p, count, n, d_out.dev.p, (void*)h->stream); };
    return run_staged(h, "hipMalloc failed for the generator test", "generator launch failed", launch, d_seeds, d_out);
}

int pdmpc_debug_heap_script(pdmpc_handle* h, int32_t n, const int32_t* op, const int32_t* id, const double* key, int32_t lds_entries,
                            int32_t* popped, int32_t* n_popped, double* cycles_per_pop, double* cycles_per_push) {
    if (!h || n < 0 || (n > 0 && (!op || !id || !key)) || !popped || !n_popped) return fail(PDMPC_ERR_INVALID, "null argument");
    if (lds_entries < 64 || lds_entries > 8192 || (lds_entries & 1)) return fail(PDMPC_ERR_INVALID, "lds_entries must be even and in 64..8192");
    ON_DEVICE(h->cfg.device);
    const size_t m = (size_t)std::max(n, 1);
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += op[i] == 1;
    unsigned long long st[4];
    Staged<const int32_t> d_op{op, (size_t)n, m}, d_id{id, (size_t)n, m};
    Staged<const double> d_key{key, (size_t)n, m};
    Staged<int32_t> d_out{popped, (size_t)cnt, m};
    Staged<double> d_gkey{nullptr, 0, m + 2};  // (the heap's part in HBM: on the device only)
    Staged<uint32_t> d_gid{nullptr, 0, m + 2};
    Staged<unsigned long long> d_stats{st, 4};
    auto launch = [&] { return pdmpc_launch_heap_script(d_op.dev.p, d_id.dev.p, d_key.dev.p, n, d_out.dev.p, d_stats.dev.p, d_gkey.dev.p, d_gid.dev.p, lds_entries, (void*)h->stream); };
    if (const int rc = run_staged(h, "hipMalloc failed for the heap script", "heap script launch failed", launch, d_op, d_id, d_out, d_key, d_gkey, d_gid, d_stats)) return rc;
    *n_popped = cnt;
    if (cycles_per_pop) *cycles_per_pop = st[1] ? (double)st[0] / (double)st[1] : 0.0;
    if (cycles_per_push) *cycles_per_push = st[3] ? (double)st[2] / (double)st[3] : 0.0;
    return PDMPC_OK;
}

int pdmpc_debug_edge_check(pdmpc_handle* h, int32_t mode, int32_t n_cases, const int32_t* a_off, const double* a_x, const double* a_y, const int32_t* b_off,
                           const double* b_x, const double* b_y, int32_t* hit) {
    if (!h || n_cases < 0 || (n_cases > 0 && (!a_off || !a_x || !a_y || !b_off || !b_x || !b_y || !hit))) return fail(PDMPC_ERR_INVALID, "null argument");
    if (mode < 0 || mode > 3) return fail(PDMPC_ERR_INVALID, "mode must be 0 (InterX), 1 (intersect_sat), 2 (intersect_lanelet_boundary) or 3 (intersect_sat against a soup)");
    if (n_cases == 0) return PDMPC_OK;
    for (int c = 0; c < n_cases; ++c) {
        const int na = a_off[c + 1] - a_off[c], nb = b_off[c + 1] - b_off[c];
        if (na < 0 || na > PDMPC_VMAX) return fail(PDMPC_ERR_INVALID, "first operand: at most PDMPC_VMAX columns");
        if (nb < 0 || nb > 1024) return fail(PDMPC_ERR_INVALID, "second operand: at most 1024 columns");
    }
    ON_DEVICE(h->cfg.device);
    const size_t nc = (size_t)n_cases, ta = (size_t)a_off[n_cases], tb = (size_t)b_off[n_cases];
    Staged<const int32_t> d_ao{a_off, nc + 1}, d_bo{b_off, nc + 1};
    Staged<const double> d_ax{a_x, ta}, d_ay{a_y, ta}, d_bx{b_x, tb}, d_by{b_y, tb};
    Staged<int32_t> d_hit{hit, nc};
    auto launch = [&] { return pdmpc_launch_edge_check(mode, n_cases, d_ao.dev.p, d_ax.dev.p, d_ay.dev.p, d_bo.dev.p, d_bx.dev.p, d_by.dev.p, d_hit.dev.p, (void*)h->stream); };
    return run_staged(h, "hipMalloc failed for the edge-check cases", "edge-check launch failed", launch, d_ao, d_bo, d_hit, d_ax, d_ay, d_bx, d_by);
}

int pdmpc_debug_interx_soups(pdmpc_handle* h, int32_t n_cases, const int32_t* a_off, const double* a_x, const double* a_y, const double* b_x, const double* b_y,
                             const int32_t* s_off, const double* s_x, const double* s_y, int32_t* hit) {
    if (!h || n_cases < 0 || (n_cases > 0 && (!a_off || !a_x || !a_y || !b_x || !b_y || !s_off || !s_x || !s_y || !hit))) return fail(PDMPC_ERR_INVALID, "null argument");
    if (n_cases == 0) return PDMPC_OK;
    for (int c = 0; c < n_cases; ++c) {
        const int V = a_off[c + 1] - a_off[c];
        if (V < 0 || V > PDMPC_VMAX) return fail(PDMPC_ERR_INVALID, "shapes: at most PDMPC_VMAX columns");
        for (int q = 0; q < 3; ++q)
            if (s_off[3 * c + q + 1] < s_off[3 * c + q]) return fail(PDMPC_ERR_INVALID, "soup offsets must not decrease");
        if (s_off[3 * c + 3] - s_off[3 * c] > 1024) return fail(PDMPC_ERR_INVALID, "the three soups of a case: at most 1024 columns together");
    }
    if (a_off[0] < 0 || s_off[0] < 0) return fail(PDMPC_ERR_INVALID, "negative offset");
    ON_DEVICE(h->cfg.device);
    const size_t nc = (size_t)n_cases, ta = (size_t)a_off[n_cases], ts = (size_t)s_off[3 * n_cases];
    Staged<const int32_t> d_ao{a_off, nc + 1}, d_so{s_off, 3 * nc + 1};
    Staged<const double> d_ax{a_x, ta}, d_ay{a_y, ta}, d_bx{b_x, ta}, d_by{b_y, ta}, d_sx{s_x, ts}, d_sy{s_y, ts};
    Staged<int32_t> d_hit{hit, nc};
    auto launch = [&] { return pdmpc_launch_interx_soups(n_cases, d_ao.dev.p, d_ax.dev.p, d_ay.dev.p, d_bx.dev.p, d_by.dev.p, d_so.dev.p, d_sx.dev.p, d_sy.dev.p, d_hit.dev.p, (void*)h->stream); };
    return run_staged(h, "hipMalloc failed for the edge-check cases", "edge-check launch failed", launch, d_ao, d_so, d_hit, d_ax, d_ay, d_bx, d_by, d_sx, d_sy);
}

int pdmpc_debug_sincos(pdmpc_handle* h, int32_t n, const double* x, double* s, double* c) {
    if (!h || n < 0 || (n > 0 && (!x || !s || !c))) return fail(PDMPC_ERR_INVALID, "pdmpc_debug_sincos: bad argument");
    if (n == 0) return PDMPC_OK;
    ON_DEVICE(h->cfg.device);
    Staged<const double> d_x{x, (size_t)n};
    Staged<double> d_s{s, (size_t)n}, d_c{c, (size_t)n};
    auto launch = [&] { return pdmpc_launch_debug_sincos(d_x.dev.p, n, d_s.dev.p, d_c.dev.p, (void*)h->stream); };
    return run_staged(h, "hipMalloc failed for the sin/cos test", "sin/cos launch failed", launch, d_x, d_s, d_c);
}

// ---- the debug read-backs of a slot's tree
namespace {
// the slot a debug read-back's vehicle was planned in (the packer may have put the batch into level order)
int debug_slot(const pdmpc_handle* h, int vehicle) {
    const PackedStep& B = h->banks[h->bank];
    return !B.inv.empty() && vehicle < B.n_packed ? B.inv[(size_t)vehicle] : vehicle;
}

// the first min(sz, capacity) records of a slot's arena as they are (and their keys / validity bytes where asked for)
int copy_raw_tree(pdmpc_handle* h, int slot, int32_t sz, int32_t capacity, const TreeColumns& cols, double* key, uint8_t* validity, int32_t* n) {
    *n = sz;
    const size_t m = (size_t)std::max(std::min(sz, capacity), 0);
    if (m == 0) return PDMPC_OK;
    const size_t off = (size_t)slot * h->arena.max_nodes;
    std::vector<NodeRec> rec(m);
    HIPCHK(hipMemcpy(rec.data(), h->arena.nodes.p + off, m * sizeof(NodeRec), hipMemcpyDeviceToHost));
    if (key) HIPCHK(hipMemcpy(key, h->arena.key.p + off, m * 8, hipMemcpyDeviceToHost));
    if (validity) HIPCHK(hipMemcpy(validity, h->arena.vstate.p + off, m, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; ++i) cols.put(i, rec[i], (int32_t)rec[i].parent);
    return PDMPC_OK;
}

// A slot's raw arena (tree_size word sz, PDMPC_TREE_FRONTIER set) copied to the host — rec: its records — and read as the reference's tree
// (reference_tree.hpp: the five copies happen here, the arithmetic there).
int fetch_reference_tree(pdmpc_handle* h, int slot, int32_t sz, std::vector<NodeRec>& rec, RefTree& T) {
    const uint32_t raw_n = (uint32_t)PDMPC_TREE_SIZE(sz);
    if (raw_n > h->arena.max_nodes) return fail(PDMPC_ERR_INVALID, "the slot's tree is larger than its arena");
    const size_t off = (size_t)slot * h->arena.max_nodes;
    rec.resize(raw_n);
    std::vector<double> key(raw_n);
    std::vector<uint8_t> vs(raw_n);
    HIPCHK(hipMemcpy(rec.data(), h->arena.nodes.p + off, (size_t)raw_n * sizeof(NodeRec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(key.data(), h->arena.key.p + off, (size_t)raw_n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(vs.data(), h->arena.vstate.p + off, (size_t)raw_n, hipMemcpyDeviceToHost));
    pdmpc_vehicle_out out;
    HIPCHK(hipMemcpy(&out, h->d_out.p + slot, sizeof out, hipMemcpyDeviceToHost));
    const bool replayed = (sz & PDMPC_TREE_REPLAYED) != 0;
    std::vector<uint32_t> pops;  // (replayed: the binary heap's pop sequence, which the kernel's replay left in the mid list's array)
    if (replayed) {
        if (out.n_popped > (int32_t)h->arena.max_nodes) return fail(PDMPC_ERR_INVALID, "the slot's record counts more pops than its arena holds nodes");
        pops.resize((size_t)std::max(out.n_popped, 0));
        if (!pops.empty()) HIPCHK(hipMemcpy(pops.data(), h->arena.mid_id.p + off, pops.size() * 4, hipMemcpyDeviceToHost));
    }
    std::string err;
    return failed(reconstruct_reference_tree(rec.data(), raw_n, key.data(), vs.data(), h->cfg.Hp, out.status, replayed ? &pops : nullptr, T, err), err);
}
}  // namespace

int pdmpc_debug_pop_trace(pdmpc_handle* h, int32_t vehicle, int32_t capacity, int32_t* ids, int32_t* n) {
    if (!h || !ids || !n) return fail(PDMPC_ERR_INVALID, "null argument");
    if (vehicle < 0 || vehicle >= h->max_vehicles) return fail(PDMPC_ERR_INVALID, "vehicle slot out of range");
    vehicle = debug_slot(h, vehicle);
    ON_DEVICE(h->cfg.device);
    HIPCHK(hipStreamSynchronize(h->stream));
    int32_t sz = 0;
    HIPCHK(hipMemcpy(&sz, h->d_tree_size.p + vehicle, 4, hipMemcpyDeviceToHost));
    if (sz & PDMPC_TREE_FRONTIER) {
        std::vector<NodeRec> rec;
        RefTree T;
        int rc = fetch_reference_tree(h, vehicle, sz, rec, T);
        if (rc) return rc;
        *n = (int32_t)T.pops.size();
        for (size_t i = 0; i < T.pops.size() && (int)i < capacity; ++i) ids[i] = (int32_t)T.ref_id[T.pops[i]];
        return PDMPC_OK;
    }
    return fail(PDMPC_ERR_INVALID, "no graph search has run in that slot");
}

int pdmpc_debug_raw_tree(pdmpc_handle* h, int32_t vehicle, int32_t capacity, double* x, double* y, double* yaw, double* g, double* hh, int32_t* trim,
                         int32_t* k, int32_t* parent, double* key, uint8_t* validity, int32_t* n) {
    if (!h || !n) return fail(PDMPC_ERR_INVALID, "null argument");
    if (vehicle < 0 || vehicle >= h->max_vehicles) return fail(PDMPC_ERR_INVALID, "vehicle slot out of range");
    vehicle = debug_slot(h, vehicle);
    ON_DEVICE(h->cfg.device);
    HIPCHK(hipStreamSynchronize(h->stream));
    int32_t sz = 0;
    HIPCHK(hipMemcpy(&sz, h->d_tree_size.p + vehicle, 4, hipMemcpyDeviceToHost));
    return copy_raw_tree(h, vehicle, PDMPC_TREE_SIZE(sz), capacity, {x, y, yaw, g, hh, trim, k, parent}, key, validity, n);
}

int pdmpc_debug_progress(pdmpc_handle* h, int32_t vehicle, uint32_t* words16) {
    if (!h || !words16 || vehicle < 0 || vehicle >= h->max_vehicles) return fail(PDMPC_ERR_INVALID, "bad argument");
    vehicle = debug_slot(h, vehicle);
    for (int i = 0; i < 32; ++i) words16[i] = h->progress ? ((volatile uint32_t*)h->progress)[vehicle * 64 + i] : 0u;
    return PDMPC_OK;
}

int pdmpc_debug_tree(pdmpc_handle* h, int32_t vehicle, int32_t capacity, double* x, double* y, double* yaw, double* g, double* hh,
                     int32_t* trim, int32_t* k, int32_t* parent, int32_t* n) {
    if (!h || !n) return fail(PDMPC_ERR_INVALID, "null argument");
    if (vehicle < 0 || vehicle >= h->max_vehicles) return fail(PDMPC_ERR_INVALID, "vehicle slot out of range");
    vehicle = debug_slot(h, vehicle);
    ON_DEVICE(h->cfg.device);
    HIPCHK(hipStreamSynchronize(h->stream));
    int32_t sz = 0;
    HIPCHK(hipMemcpy(&sz, h->d_tree_size.p + vehicle, 4, hipMemcpyDeviceToHost));
    const TreeColumns cols{x, y, yaw, g, hh, trim, k, parent};
    if (sz & PDMPC_TREE_FRONTIER) {
        std::vector<NodeRec> rec;
        RefTree T;
        int rc = fetch_reference_tree(h, vehicle, sz, rec, T);
        if (rc) return rc;
        *n = (int32_t)T.ref_nodes.size();
        for (size_t i = 0; i < T.ref_nodes.size() && (int)i < capacity; ++i) {
            const NodeRec& r = rec[T.ref_nodes[i]];
            cols.put(i, r, r.parent ? (int32_t)T.ref_id[r.parent - 1] : 0);
        }
        return PDMPC_OK;
    }
    return copy_raw_tree(h, vehicle, sz, capacity, cols, nullptr, nullptr, n);
}

}  // extern "C"

