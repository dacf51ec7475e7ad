// group.cpp — several GPUs behind the C ABI (include/pdmpc.h: pdmpc_group_*).
//
// What is exchanged.  In the reference every vehicle publishes its solved areas after it has planned and every coupled vehicle reads
// them before it plans (hlc/communication/PredictionsCommunication.m:34-63: send_message / read_message on the Predictions topic;
// called from PrioritizedController.publish_predictions, hlc/controller/prioritized/PrioritizedController.m:356-365, read back in
// consider_predecessors, :476-491).  Between GPUs that broadcast is an all-gather of the fixed-stride result records
// (pdmpc_vehicle_out, 2.9 KB per vehicle) on the handles' own streams: RCCL over xGMI, one communicator per device of ONE process
// (ncclCommInitAll), every collective issued for all devices inside ncclGroupStart / ncclGroupEnd by the calling thread.
//
// How a step is split (the twin of p-dmpc_amd/pdmpc/distributed.py, which drives the same protocol from one process per GPU
// through torch.distributed; tests/test_group.py compares the partitions):
//   - the weakly connected components of the step's coupling graph exchange nothing within the step (the reference's vehicles do
//     not even subscribe to uncoupled ones, PrioritizedController.m:208-255): a device takes whole components, longest processing
//     time first, plans them with ONE launch (hand-off between levels on the device) and one all-gather ends the step;
//   - a component that outweighs the mean load per device (or every component, PDMPC_SHARD_LEVELS) is planned by all devices level
//     by level: the level's slots block-partitioned, pdmpc_launch_range per device, all-gather, pdmpc_import_results of the other
//     devices' blocks, next level — everything enqueued on the streams, the host waits once per step.
// librccl is loaded with dlopen when the first group that needs it is created: the single-GPU library has no link-time dependency on it.
//
// The exchange sits behind a function table (struct Collective): RCCL's all-gather between the distinct devices of a group, or the
// same all-gather as peer copies ordered by events on the handles' streams (PDMPC_COLLECTIVE_COPY) — which also works between
// LOGICAL ranks that share a physical device (two handles, two streams, two sets of arenas on one GPU), so every line of the
// multi-rank protocol (slot remapping, block partition of a level, import of the other ranks' blocks) runs on a 1-GPU box
// (tests/test_group.py).  Every entry point leaves the caller's current device as it found it (DeviceGuard, hip_host.hpp).
//
// What need not be exchanged.  A caller that keeps a few of a batch's plans (the explorative and the optimal-priority step, a sweep of
// them) gets the three read-backs of a handle over the group: the step's launches without the end-of-step
// all-gather leave every record with the rank that planned it (group_route.hpp says which, and where), and then either 16 bytes per
// record reach the host and the wanted records follow from their holders (pdmpc_group_plan_step_lean, _fetch_records_at), or the ranks
// all-gather those 16-byte entries, each makes the same choice and copies the picked records it holds into one block of host memory
// (pdmpc_group_plan_step_chosen; kernels in group_choice_kernel.hip).
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/pdmpc.h"
#include "choice_host.hpp"
#include "coupling_order.hpp"
#include "group_choice.h"
#include "group_route.hpp"
#include "hip_host.hpp"  // (the handles are driven through the C ABI: no handle.hpp, no struct pdmpc_handle here)
#include "launch_plan.hpp"  // (host only: PendingSeeds)

namespace {

struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
std::mutex g_rccl_mutex;
Rccl g_rccl;

bool load_rccl(std::string& err) {
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.lib) return true;
    // (a librccl.so.1 the process has loaded already — torch ships one — is the one dlopen returns: never two copies)
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* lib = nullptr;
    for (const char* n : names) {
        lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (lib) break;
    }
    if (!lib) {
        err = std::string("librccl could not be loaded: ") + (dlerror() ? dlerror() : "not found");
        return false;
    }
    Rccl r;
    r.lib = lib;
    r.CommInitAll = (decltype(r.CommInitAll))dlsym(lib, "ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(lib, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(lib, "ncclAllGather");
    r.GroupStart = (decltype(r.GroupStart))dlsym(lib, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(lib, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!r.CommInitAll || !r.CommDestroy || !r.AllGather || !r.GroupStart || !r.GroupEnd) {
        err = "librccl lacks ncclCommInitAll / ncclAllGather / ncclGroupStart";
        return false;
    }
    g_rccl = r;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// The partition and the route are pure host logic (group_route.hpp; pdmpc_group_partition and pdmpc_group_route_host expose them).
using Partition = GroupPartition;
int make_partition(int n, const int32_t* off, const int32_t* idx, const double* weights, int world, int mode, Partition& P) {
    std::string err;
    return failed(::make_partition(n, off, idx, weights, world, mode, P, err), err);
}

// the step problem restricted to `slots`: predecessor indices remapped to positions (predecessors outside the selection cannot occur:
// the selection is made of whole components)
struct SubProblem {
    std::vector<pdmpc_vehicle_in> in;
    std::vector<int32_t> pred_off, pred_idx;
    std::vector<pdmpc_polygon_set> fallback;
    bool any_fallback = false;
};
void make_sub(const std::vector<int>& slots, int n, const pdmpc_vehicle_in* in, const int32_t* off, const int32_t* idx, const pdmpc_polygon_set* fb, SubProblem& S) {
    std::vector<int> pos((size_t)n, -1);
    for (size_t i = 0; i < slots.size(); ++i) pos[(size_t)slots[i]] = (int)i;
    S.in.clear();
    S.pred_off.assign(1, 0);
    S.pred_idx.clear();
    S.fallback.clear();
    S.any_fallback = fb != nullptr;
    for (int s : slots) {
        S.in.push_back(in[s]);
        if (off)
            for (int q = off[s]; q < off[s + 1]; ++q)
                if (idx[q] >= 0 && idx[q] < n && pos[(size_t)idx[q]] >= 0) S.pred_idx.push_back(pos[(size_t)idx[q]]);
        S.pred_off.push_back((int32_t)S.pred_idx.size());
        if (fb) S.fallback.push_back(fb[s]);
    }
    if (S.pred_idx.empty()) S.pred_idx.push_back(0);
}

const size_t kRec = sizeof(pdmpc_vehicle_out);

}  // namespace

struct pdmpc_group;
namespace {
using Bytes = DevBuf<unsigned char>;
// what a rank owns on its device; grown on that device (grow_on_ranks) and released there, before the rank's handle goes
struct RankBufs {
    Bytes send, recv;                    // its block of records / every rank's block
    Bytes esend, erecv;                  // its block of entries / every rank's block
    DevBuf<int32_t> lists;               // the staged lists of a choice (ChoiceLists)
    Bytes made;                          // chosen and cell_cost as the cells pass leaves them (ChoiceLayout's offsets)
    DevBuf<pdmpc_vehicle_out> placed;    // records placed by pdmpc_group_debug_choose
    DevBuf<pdmpc_vehicle_out> shared;    // rank 0 alone: the records of the component planned by levels
    unsigned char* pin_out = nullptr;    // the group's pin_out as this rank's kernels address it
};
// the exchange between the ranks of a group: `bytes` bytes from every rank's send buffer into every rank's receive buffer
// (rank r's block at r * bytes), enqueued on the handles' streams.  Whole records between the levels of a shared component and at
// the end of pdmpc_group_plan_step; 16-byte entries for a choice over the ranks.
struct Collective {
    const char* name;
    int (*all_gather)(pdmpc_group* g, Bytes RankBufs::*send, Bytes RankBufs::*recv, size_t bytes);
};
}  // namespace

struct pdmpc_group {
    std::vector<int> dev;
    std::vector<pdmpc_handle*> h;
    std::vector<hipStream_t> stream;
    std::vector<ncclComm_t> comm;
    const Collective* coll = nullptr;
    std::vector<hipEvent_t> ev_sent, ev_got;  // copy collective: rank r's block is ready / rank r has copied every block
    int last_bank = -1;                       // the bank whose records the ranks' recv / rank 0's shared hold (pdmpc_group_fetch)
    std::vector<RankBufs> buf;                // per rank
    std::vector<unsigned char> host;          // read-back staging
    double timing[6] = {0, 0, 0, 0, 0, 0};
    // ---- lean read-back and the choice over the ranks
    int32_t Hp = 0;                           // the handles' prediction horizon: the row of path_nodes whose g is a plan's cost
    int resident_bank = -1;                   // the bank whose records the ranks HOLD (group_route.hpp) since the last launch of either kind
    std::vector<const pdmpc_vehicle_out*> rec;  // per rank: its handle's record buffer
    PendingSeeds seeds;                       // pdmpc_group_set_step_seeds: taken by the next pack
    int64_t xchg[4] = {0, 0, 0, 0};           // pdmpc_group_last_exchange
    PinnedBuf<int32_t> pin_lists{hipHostMallocPortable};  // the lists on their way to the ranks
    // mapped into every device: what kernels write for the host, and the staging of record copies (RankBufs::pin_out: the ranks' views)
    PinnedBuf<unsigned char> pin_out{hipHostMallocPortable | hipHostMallocMapped};
    struct Plan {                             // a packed step (pdmpc_group_pack_step): how it is split and how large its blocks are
        bool valid = false;
        int n = 0;
        Partition P;
        GroupRoute route;                     // who holds which record after its launches
        size_t per_w = 0;
    };
    std::vector<Plan> plans;
};

namespace {

#define GNCCL(expr)                                                                                                             \
    do {                                                                                                                        \
        ncclResult_t r__ = (expr);                                                                                              \
        if (r__ != ncclSuccess) {                                                                                               \
            char b__[512];                                                                                                      \
            snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString ? g_rccl.GetErrorString(r__) : "?", __FILE__, __LINE__); \
            return fail(PDMPC_ERR_HIP, b__);                                                                                   \
        }                                                                                                                       \
    } while (0)
#define GRC(expr)                \
    do {                         \
        const int rc__ = (expr); \
        if (rc__) return rc__;   \
    } while (0)

// HBM banks of the two sub-problems of group bank b (pdmpc_select_bank): the handles' own banks 0 .. 2047 stay the caller's
const int kGroupBanks = 1000;
inline int bank_shared(int b) { return 2048 + 2 * b; }
inline int bank_whole(int b) { return 2049 + 2 * b; }

// Rank r's buffer of at least n elements, grown on its device and zero-filled when it grows (DevBuf's head room).  The rank's stream is
// idle by then: a buffer moves between the calls that enqueue on it, never under one.
template <class T>
int grow_on_rank(pdmpc_group* g, size_t r, DevBuf<T>& b, size_t n) {
    if (n <= b.cap) return PDMPC_OK;
    HIPCHK(hipSetDevice(g->dev[r]));
    HIPCHK(hipStreamSynchronize(g->stream[r]));
    if (b.ensure(n)) return fail(PDMPC_ERR_HIP, "no device memory for a buffer of the group");
    HIPCHK(hipMemset(b.p, 0, b.cap * sizeof(T)));
    return PDMPC_OK;
}
// ... of every rank
template <class T>
int grow_on_ranks(pdmpc_group* g, DevBuf<T> RankBufs::*member, size_t n) {
    for (size_t r = 0; r < g->h.size(); ++r) GRC(grow_on_rank(g, r, g->buf[r].*member, n));
    return PDMPC_OK;
}

// one all-gather of `per` records per device over the whole group, on the handles' streams: RCCL ...
int all_gather_rccl(pdmpc_group* g, Bytes RankBufs::*send, Bytes RankBufs::*recv, size_t bytes) {
    const size_t world = g->h.size();
    GNCCL(g_rccl.GroupStart());
    for (size_t r = 0; r < world; ++r) GNCCL(g_rccl.AllGather((g->buf[r].*send).p, (g->buf[r].*recv).p, bytes, ncclChar, g->comm[r], g->stream[r]));
    GNCCL(g_rccl.GroupEnd());
    return PDMPC_OK;
}
// ... or peer copies.  Rank q's stream waits for every rank's block (an event per rank, recorded behind its export), copies the
// blocks into its own receive buffer, and says so; a rank's stream goes on (its next export overwrites its send buffer) once
// everybody has copied.  Nothing waits on the host.
int all_gather_copy(pdmpc_group* g, Bytes RankBufs::*send, Bytes RankBufs::*recv, size_t bytes) {
    const size_t world = g->h.size();
    for (size_t r = 0; r < world; ++r) {
        HIPCHK(hipSetDevice(g->dev[r]));
        HIPCHK(hipEventRecord(g->ev_sent[r], g->stream[r]));
    }
    for (size_t q = 0; q < world; ++q) {
        HIPCHK(hipSetDevice(g->dev[q]));
        for (size_t r = 0; r < world; ++r) {
            if (r != q) HIPCHK(hipStreamWaitEvent(g->stream[q], g->ev_sent[r], 0));
            unsigned char* dst = (g->buf[q].*recv).p + r * bytes;
            const unsigned char* src = (g->buf[r].*send).p;
            if (g->dev[q] == g->dev[r])
                HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g->stream[q]));
            else
                HIPCHK(hipMemcpyPeerAsync(dst, g->dev[q], src, g->dev[r], bytes, g->stream[q]));
        }
        HIPCHK(hipEventRecord(g->ev_got[q], g->stream[q]));
    }
    for (size_t r = 0; r < world; ++r) {
        HIPCHK(hipSetDevice(g->dev[r]));
        for (size_t q = 0; q < world; ++q)
            if (q != r) HIPCHK(hipStreamWaitEvent(g->stream[r], g->ev_got[q], 0));
    }
    return PDMPC_OK;
}
const Collective kCollRccl = {"rccl", all_gather_rccl};
const Collective kCollCopy = {"copy", all_gather_copy};
// ... of `per` records per rank, and of a block of entries per rank; both counted for pdmpc_group_last_exchange
inline int all_gather(pdmpc_group* g, size_t per) {
    g->xchg[0] += (int64_t)(per * kRec);
    return g->coll->all_gather(g, &RankBufs::send, &RankBufs::recv, per * kRec);
}
inline int all_gather_entries(pdmpc_group* g, size_t per) {
    g->xchg[0] += (int64_t)((per + 1) * sizeof(GroupEntry));
    return g->coll->all_gather(g, &RankBufs::esend, &RankBufs::erecv, (per + 1) * sizeof(GroupEntry));
}

using clk = std::chrono::steady_clock;
inline double ms_between(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// partition the step, build the sub-problems and make them resident on the devices (group bank `bank`)
int group_pack(pdmpc_group* g, int bank, int n, const pdmpc_vehicle_in* in, const int32_t* off, const int32_t* idx, const pdmpc_polygon_set* fb, const double* weights, int mode) {
    const auto t0 = clk::now();
    const int world = (int)g->h.size();
    if ((size_t)bank >= g->plans.size()) g->plans.resize((size_t)bank + 1);
    pdmpc_group::Plan& L = g->plans[(size_t)bank];
    L.valid = false;
    if (g->last_bank == bank) g->last_bank = -1;
    if (g->resident_bank == bank) g->resident_bank = -1;
    // the seeds set for this pack are consumed by it, also if it fails (as a handle's: pack.cpp)
    std::vector<uint32_t> seeds;
    const bool sampled = g->seeds.take(seeds);
    if (sampled && (int)seeds.size() != n) return fail(PDMPC_ERR_INVALID, "pdmpc_group_set_step_seeds: the seeds are not one per vehicle of the packed step");
    if (sampled) {
        // one budget for the step: the ranks plan shares of ONE sampled step (pdmpc_group_set_sampled_budget sets them all)
        int32_t first = 0, other = 0;
        GRC(pdmpc_get_sampled_budget(g->h[0], &first));
        for (int r = 1; r < world; ++r) {
            GRC(pdmpc_get_sampled_budget(g->h[(size_t)r], &other));
            if (other != first) return fail(PDMPC_ERR_INVALID, "the ranks of the group have different sampled budgets (pdmpc_group_set_sampled_budget sets every rank)");
        }
        // ... and one ensemble size
        GRC(pdmpc_get_sampled_ensemble(g->h[0], &first));
        for (int r = 1; r < world; ++r) {
            GRC(pdmpc_get_sampled_ensemble(g->h[(size_t)r], &other));
            if (other != first) return fail(PDMPC_ERR_INVALID, "the ranks of the group have different ensemble sizes (pdmpc_group_set_sampled_ensemble sets every rank)");
        }
    }
    L.n = n;
    Partition& P = L.P;
    GRC(make_partition(n, off, idx, weights, world, mode, P));
    route_partition(P, n, L.route);
    SubProblem S;
    std::vector<SubProblem> W((size_t)world);
    if (!P.shared.empty()) make_sub(P.shared, n, in, off, idx, fb, S);
    size_t per_w = 0, per_l = 0;
    for (int r = 0; r < world; ++r) {
        if (!P.parts[(size_t)r].empty()) make_sub(P.parts[(size_t)r], n, in, off, idx, fb, W[(size_t)r]);
        per_w = std::max(per_w, P.parts[(size_t)r].size());
    }
    for (int sz : P.level_sizes) per_l = std::max(per_l, (size_t)((sz + world - 1) / world));
    L.per_w = std::max<size_t>(per_w, 1);
    const auto t1 = clk::now();
    // the shared component on every device, a device's whole components on that device
    const int nS = (int)P.shared.size();
    for (int r = 0; r < world; ++r) {
        // (a sampled bank: the seeds travel with the slots, so every rank packs them for its share)
        if (nS) {
            GRC(pdmpc_select_bank(g->h[(size_t)r], bank_shared(bank)));
            if (sampled) {
                const std::vector<uint32_t> sub = route_seeds(P.shared, seeds);
                GRC(pdmpc_set_step_seeds(g->h[(size_t)r], nS, sub.data()));
            }
            GRC(pdmpc_pack_step(g->h[(size_t)r], nS, S.in.data(), S.pred_off.data(), S.pred_idx.data(), S.any_fallback ? S.fallback.data() : nullptr));
        }
        const SubProblem& w = W[(size_t)r];
        if (!w.in.empty()) {
            GRC(pdmpc_select_bank(g->h[(size_t)r], bank_whole(bank)));
            if (sampled) {
                const std::vector<uint32_t> sub = route_seeds(P.parts[(size_t)r], seeds);
                GRC(pdmpc_set_step_seeds(g->h[(size_t)r], (int)w.in.size(), sub.data()));
            }
            GRC(pdmpc_pack_step(g->h[(size_t)r], (int)w.in.size(), w.in.data(), w.pred_off.data(), w.pred_idx.data(), w.any_fallback ? w.fallback.data() : nullptr));
        }
        GRC(pdmpc_select_bank(g->h[(size_t)r], 0));
    }
    // a block of the largest exchange of records to send, every rank's block to receive; the shared component's records on rank 0
    const size_t block = std::max<size_t>(std::max(per_w, per_l), 1) * kRec;
    GRC(grow_on_ranks(g, &RankBufs::send, block));
    GRC(grow_on_ranks(g, &RankBufs::recv, block * (size_t)world));
    GRC(grow_on_rank(g, 0, g->buf[0].shared, (size_t)nS));
    L.valid = true;
    g->timing[1] = ms_between(t0, t1);
    g->timing[2] = ms_between(t1, clk::now());
    return PDMPC_OK;
}

// one wait of the host, on all streams
int group_wait(pdmpc_group* g) {
    for (size_t r = 0; r < g->h.size(); ++r) GRC(pdmpc_synchronize(g->h[r]));
    g->xchg[2] += 1;
    return PDMPC_OK;
}

// The launches of a packed step enqueued on the handles' streams: the shared component level by level with its exchanges, then the
// whole components.  gather_records: the all-gather of the whole components' records that pdmpc_group_fetch reads; without it the
// records stay with the ranks that planned them (Plan::route) and nothing but the level exchanges has moved a record.
int group_enqueue(pdmpc_group* g, int bank, bool gather_records) {
    if ((size_t)bank >= g->plans.size() || !g->plans[(size_t)bank].valid) return fail(PDMPC_ERR_INVALID, "pdmpc_group_launch: nothing packed in that bank");
    g->last_bank = g->resident_bank = -1;
    const int world = (int)g->h.size();
    const pdmpc_group::Plan& L = g->plans[(size_t)bank];
    const Partition& P = L.P;
    const int nS = (int)P.shared.size();
    // ---- the shared component, level by level (PredictionsCommunication.m:34-63 per level)
    if (nS) {
        for (int r = 0; r < world; ++r) {
            GRC(pdmpc_select_bank(g->h[(size_t)r], bank_shared(bank)));
            GRC(pdmpc_begin_step(g->h[(size_t)r]));
        }
        int first = 0;
        for (int size : P.level_sizes) {
            const int per = (size + world - 1) / world;
            auto block = [&](int r, int& lo, int& hi) {
                lo = std::min(first + r * per, first + size);
                hi = std::min(lo + per, first + size);
            };
            for (int r = 0; r < world; ++r) {
                int lo, hi;
                block(r, lo, hi);
                if (hi > lo) {
                    GRC(pdmpc_launch_range(g->h[(size_t)r], lo, hi - lo));
                    GRC(pdmpc_export_results_async(g->h[(size_t)r], lo, hi - lo, g->buf[(size_t)r].send.p));
                }
            }
            GRC(all_gather(g, (size_t)per));
            for (int r = 0; r < world; ++r)
                for (int q = 0; q < world; ++q) {
                    int lo, hi;
                    block(q, lo, hi);
                    if (q != r && hi > lo) GRC(pdmpc_import_results(g->h[(size_t)r], lo, hi - lo, g->buf[(size_t)r].recv.p + (size_t)q * per * kRec));
                }
            first += size;
        }
        GRC(pdmpc_export_results_async(g->h[0], 0, nS, g->buf[0].shared.p));  // (before the next launch overwrites the slots)
    }
    // ---- whole components: one launch per device, one all-gather
    bool any_whole = false;
    for (int r = 0; r < world; ++r) {
        const int nr = (int)P.parts[(size_t)r].size();
        if (!nr) continue;
        any_whole = true;
        GRC(pdmpc_select_bank(g->h[(size_t)r], bank_whole(bank)));
        GRC(pdmpc_launch_packed(g->h[(size_t)r]));
        if (gather_records) GRC(pdmpc_export_results_async(g->h[(size_t)r], 0, nr, g->buf[(size_t)r].send.p));
    }
    if (any_whole && gather_records) GRC(all_gather(g, L.per_w));
    return PDMPC_OK;
}

// what every launch ends with, after the wait: the handles back on their bank 0, the bank's records held by the ranks
int group_launched(pdmpc_group* g, int bank, bool gathered_records) {
    for (size_t r = 0; r < g->h.size(); ++r) GRC(pdmpc_select_bank(g->h[r], 0));
    g->resident_bank = bank;
    if (gathered_records) g->last_bank = bank;
    return PDMPC_OK;
}

// plan the packed step: everything enqueued on the handles' streams, one wait at the end
int group_launch(pdmpc_group* g, int bank) {
    const auto t2 = clk::now();
    GRC(group_enqueue(g, bank, true));
    const auto t3 = clk::now();
    GRC(group_wait(g));
    GRC(group_launched(g, bank, true));
    g->timing[3] = ms_between(t2, t3);
    g->timing[4] = ms_between(t3, clk::now());
    return PDMPC_OK;
}

// the records of the step planned last (every device holds every block: read from device 0), in the caller's order
int group_fetch(pdmpc_group* g, int bank, int n, pdmpc_vehicle_out* out) {
    if ((size_t)bank >= g->plans.size() || !g->plans[(size_t)bank].valid) return fail(PDMPC_ERR_INVALID, "pdmpc_group_fetch: nothing packed in that bank");
    const auto t4 = clk::now();
    const pdmpc_group::Plan& L = g->plans[(size_t)bank];
    if (n != L.n) return fail(PDMPC_ERR_INVALID, "pdmpc_group_fetch: the bank holds another number of vehicles");
    // the gathered records are those of the bank launched last, whatever bank is asked for
    if (bank != g->last_bank) return fail(PDMPC_ERR_INVALID, "pdmpc_group_fetch: the records on the devices are those of the bank launched last; launch this bank first");
    const Partition& P = L.P;
    const int world = (int)g->h.size(), nS = (int)P.shared.size();
    bool any_whole = false;
    for (int r = 0; r < world; ++r) any_whole = any_whole || !P.parts[(size_t)r].empty();
    HIPCHK(hipSetDevice(g->dev[0]));
    if (any_whole) {
        g->host.resize(L.per_w * kRec * (size_t)world);
        HIPCHK(hipMemcpy(g->host.data(), g->buf[0].recv.p, g->host.size(), hipMemcpyDeviceToHost));
        g->xchg[1] += (int64_t)g->host.size();
        g->xchg[2] += 1;
        for (int r = 0; r < world; ++r)
            for (size_t i = 0; i < P.parts[(size_t)r].size(); ++i) std::memcpy(&out[P.parts[(size_t)r][i]], g->host.data() + ((size_t)r * L.per_w + i) * kRec, kRec);
    }
    if (nS) {
        g->host.resize((size_t)nS * kRec);
        HIPCHK(hipMemcpy(g->host.data(), g->buf[0].shared.p, g->host.size(), hipMemcpyDeviceToHost));
        g->xchg[1] += (int64_t)g->host.size();
        g->xchg[2] += 1;
        for (int i = 0; i < nS; ++i) std::memcpy(&out[P.shared[(size_t)i]], g->host.data() + (size_t)i * kRec, kRec);
    }
    g->timing[5] = ms_between(t4, clk::now());
    return PDMPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Lean read-back and the choice over the ranks (group_route.hpp; group_choice_kernel.hip).

// The reference's tree is unbounded (Tree.m:54-70): after a step in which some search outgrew its arena, arenas twice as large on every
// device (as pdmpc_plan_step does for one).  grown == false: no room, the arenas stay and the statuses tell.
int grow_all(pdmpc_group* g, const char* who, bool& grown) {
    grown = false;
    // (the devices' arenas may differ after a failed attempt to grow: the step fits when the SMALLEST arena holds every search)
    int32_t nodes = 0;
    for (pdmpc_handle* h : g->h) {
        int32_t nr = 0;
        GRC(pdmpc_arena_nodes(h, &nr, nullptr));
        nodes = nodes ? std::min(nodes, nr) : nr;
    }
    if ((int64_t)nodes * 2 > (1ll << 30)) return PDMPC_OK;
    for (size_t r = 0; r < g->h.size(); ++r) {
        int32_t nr = 0;
        GRC(pdmpc_arena_nodes(g->h[r], &nr, nullptr));
        if (nr >= nodes * 2) continue;
        if (pdmpc_grow_arena(g->h[r], nodes * 2) != PDMPC_OK) {
            // no room to grow on this device: the records keep their PDMPC_ARENA_OVERFLOW statuses AND the error string says why
            char b[192];
            snprintf(b, sizeof b, "%s: the arenas of rank %zu (device %d) cannot grow to %d nodes per vehicle", who, r, g->dev[r], nodes * 2);
            pdmpc_set_last_error(b);
            return PDMPC_OK;
        }
    }
    grown = true;
    return PDMPC_OK;
}

// the records rank r holds (GroupRoute's positions index them): n_a in rec_a, the rest in rec_b
struct Held {
    const pdmpc_vehicle_out* rec_a;
    const pdmpc_vehicle_out* rec_b;
    int32_t n_a, n_b;
};
Held held_of_bank(const pdmpc_group* g, const pdmpc_group::Plan& L, size_t r) {
    const int32_t n_a = (int32_t)L.P.parts[r].size();
    return {g->rec[r], r == 0 ? g->buf[0].shared.p : nullptr, n_a, L.route.held[r] - n_a};
}
Held held_placed(const pdmpc_group* g, const GroupRoute& R, size_t r) { return {g->buf[r].placed.p, nullptr, R.held[r], 0}; }

// pin_out of at least `bytes` bytes; no stream has work in flight when a group call begins, so it may move, and the ranks' views with it
int grow_pin_out(pdmpc_group* g, size_t bytes) {
    if (bytes <= g->pin_out.cap) return PDMPC_OK;
    if (g->pin_out.ensure(bytes)) return fail(PDMPC_ERR_HIP, "no pinned memory for the block the group reads back");
    hipError_t e = hipSuccess;
    for (size_t r = 0; r < g->h.size() && e == hipSuccess; ++r) {
        e = hipSetDevice(g->dev[r]);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&g->buf[r].pin_out, g->pin_out.p, 0);
    }
    if (e != hipSuccess) g->pin_out.release();  // (no view of the old block outlives it: the next call derives them all again)
    HIPCHK(e);
    return PDMPC_OK;
}

// a block of header + per entries to send, every rank's block to receive
int grow_entries(pdmpc_group* g, int32_t per) {
    const size_t block = ((size_t)per + 1) * sizeof(GroupEntry);
    GRC(grow_on_ranks(g, &RankBufs::esend, block));
    return grow_on_ranks(g, &RankBufs::erecv, block * g->h.size());
}

// every rank's block of entries (header + the records it holds) into `to(r)`
template <class HeldOf, class To>
int enqueue_entries(pdmpc_group* g, HeldOf&& held_of, To&& to) {
    for (size_t r = 0; r < g->h.size(); ++r) {
        const Held H = held_of(r);
        GroupEntriesArgs A{H.rec_a, H.rec_b, H.n_a, H.n_b, g->Hp, 0, (GroupEntry*)to(r)};
        HIPCHK(hipSetDevice(g->dev[r]));
        const int lrc = pdmpc_launch_group_entries(&A, (void*)g->stream[r]);
        if (lrc) return fail(PDMPC_ERR_HIP, std::string("the entries kernel's launch failed: ") + hipGetErrorString((hipError_t)lrc));
    }
    return PDMPC_OK;
}

// A checked choice staged for the ranks: its lists with slots as entry indices (route_slots), uploaded to every rank on its stream.
struct StagedChoice {
    const pdmpc_choice* ch;
    ChoiceLayout L;
    ChoiceLists W;
    explicit StagedChoice(const pdmpc_choice& c) : ch(&c), L(c), W(c) {}
};
int stage_group_choice(pdmpc_group* g, const GroupRoute& R, const StagedChoice& S) {
    if (g->pin_lists.ensure(S.W.words)) return fail(PDMPC_ERR_HIP, "no pinned memory for the lists of the group's choice");
    GRC(grow_on_ranks(g, &RankBufs::lists, S.W.words));
    GRC(grow_on_ranks(g, &RankBufs::made, S.L.picks));
    GRC(grow_pin_out(g, S.L.bytes));
    GRC(grow_entries(g, R.per));
    stage_choice_lists(*S.ch, S.W, g->pin_lists.p, [&R](const int32_t* slot, int count, int32_t* entry) { route_slots(R, slot, count, entry); });
    for (size_t r = 0; r < g->h.size(); ++r) {
        HIPCHK(hipSetDevice(g->dev[r]));
        HIPCHK(hipMemcpyAsync(g->buf[r].lists.p, g->pin_lists.p, S.W.words * sizeof(int32_t), hipMemcpyHostToDevice, g->stream[r]));
    }
    return PDMPC_OK;
}

// The choice behind whatever the streams hold: every rank's entries, ONE all-gather of them (16 bytes per record), the cells and first
// minima on every rank, the gather of the picks each rank holds into the one block the host reads.  Nothing waits on the host.
template <class HeldOf>
int enqueue_group_choice(pdmpc_group* g, const GroupRoute& R, const StagedChoice& S, HeldOf&& held_of) {
    const pdmpc_choice& ch = *S.ch;
    GRC(enqueue_entries(g, held_of, [&](size_t r) { return g->buf[r].esend.p; }));
    GRC(all_gather_entries(g, (size_t)R.per));
    for (size_t r = 0; r < g->h.size(); ++r) {
        const Held H = held_of(r);
        const RankBufs& B = g->buf[r];
        GroupChoiceArgs A{};
        A.gathered = (const GroupEntry*)B.erecv.p;
        A.world = (int32_t)g->h.size();
        A.per = R.per;
        A.rank = (int32_t)r;
        A.n_cells = ch.n_cells;
        A.n_graphs = ch.n_graphs;
        A.n_picks = ch.n_picks;
        A.first_graph_cell = ch.n_graphs > 0 ? ch.graph_offset[0] : 0;
        A.end_graph_cell = ch.n_graphs > 0 ? ch.graph_offset[ch.n_graphs] : 0;
        A.cell_offset = B.lists.p + S.W.cell_offset;
        A.cell_entry = B.lists.p + S.W.cell_slot;
        A.graph_offset = B.lists.p + S.W.graph_offset;
        A.pick_graph = B.lists.p + S.W.pick_graph;
        A.pick_offset = B.lists.p + S.W.pick_offset;
        A.pick_entry = B.lists.p + S.W.pick_slot;
        A.chosen = (int32_t*)(B.made.p + S.L.chosen);
        A.cell_cost = (double*)(B.made.p + S.L.cell_cost);
        A.rec_a = H.rec_a;
        A.rec_b = H.rec_b;
        A.n_a = H.n_a;
        A.host_block = B.pin_out;
        A.off_chosen = S.L.chosen;
        A.off_cell_cost = S.L.cell_cost;
        A.off_picks = S.L.picks;
        HIPCHK(hipSetDevice(g->dev[r]));
        int lrc = pdmpc_launch_group_cells(&A, (void*)g->stream[r]);
        if (!lrc && (r == 0 || ch.n_picks > 0)) lrc = pdmpc_launch_group_gather(&A, (void*)g->stream[r]);
        if (lrc) return fail(PDMPC_ERR_HIP, std::string("a choice kernel's launch failed: ") + hipGetErrorString((hipError_t)lrc));
    }
    g->xchg[1] += (int64_t)S.L.bytes;
    return PDMPC_OK;
}

// a choice the host has waited for into the caller's arrays (choice_host.hpp), or why it is none
int deliver_group_choice(const pdmpc_group* g, const StagedChoice& S, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks) {
    std::string err;
    return deliver_choice(*S.ch, S.L, g->pin_out.p, chosen, cell_cost, picks, err) ? PDMPC_OK : fail(PDMPC_ERR_HIP, err);
}

// the bank whose records the ranks hold, or a refusal
int resident_plan(pdmpc_group* g, int bank, const char* who, const pdmpc_group::Plan** L) {
    if (bank < 0 || (size_t)bank >= g->plans.size() || !g->plans[(size_t)bank].valid || bank != g->resident_bank)
        return fail(PDMPC_ERR_INVALID, std::string(who) + ": the ranks hold the records of the bank launched last; launch this bank first");
    *L = &g->plans[(size_t)bank];
    return PDMPC_OK;
}

inline void new_call(pdmpc_group* g) { g->xchg[0] = g->xchg[1] = g->xchg[2] = g->xchg[3] = 0; }  // pdmpc_group_last_exchange counts from here
inline bool known_mode(int mode) { return mode == PDMPC_SHARD_AUTO || mode == PDMPC_SHARD_COMPONENTS || mode == PDMPC_SHARD_LEVELS; }

// what every call that takes a step's coupling graph and a sharding mode checks first; null_argument: what the call itself requires
// is missing (`refusal` says so in its name)
int check_step_args(const char* refusal, bool null_argument, const int32_t* pred_offset, const int32_t* pred_index, int mode) {
    if (null_argument) return fail(PDMPC_ERR_INVALID, refusal);
    if (pred_offset && !pred_index) return fail(PDMPC_ERR_INVALID, "pred_index missing");
    if (!known_mode(mode)) return fail(PDMPC_ERR_INVALID, "unknown sharding mode");
    return PDMPC_OK;
}

// The reference's tree is unbounded (Tree.m:54-70): a step in which some search outgrew its arena is planned again with arenas twice as
// large on every device (as pdmpc_plan_step does for one).  attempt(overflow) plans the step once and says whether one did; the
// attempts end when none did or nothing could grow (the statuses tell).
template <class Attempt>
int plan_growing(pdmpc_group* g, const char* who, Attempt&& attempt) {
    for (;;) {
        bool overflow = false, grown = false;
        GRC(attempt(overflow));
        if (!overflow) return PDMPC_OK;
        GRC(grow_all(g, who, grown));
        if (!grown) return PDMPC_OK;
        g->xchg[3] += 1;
    }
}

// create: the devices, the collective, a handle per rank and what the collective needs, into an empty group; a failure leaves what
// there is to pdmpc_group_destroy
int group_init(pdmpc_group* g, const pdmpc_config* config, int32_t n_devices, const int32_t* devices, int32_t collective, int ndev) {
    g->Hp = config->Hp;
    bool repeated = false;
    for (int r = 0; r < n_devices; ++r) {
        const int d = devices ? devices[r] : r;
        if (d < 0 || d >= ndev) return fail(PDMPC_ERR_NO_DEVICE, "pdmpc_group_create: device ordinal out of range");
        repeated = repeated || std::find(g->dev.begin(), g->dev.end(), d) != g->dev.end();
        g->dev.push_back(d);
    }
    // ranks that share a device are logical ranks: RCCL has one rank per device, the copy collective does not care
    if (collective == PDMPC_COLLECTIVE_AUTO) {
        const char* e = getenv("PDMPC_GROUP_COLLECTIVE");
        collective = repeated ? PDMPC_COLLECTIVE_COPY : ((e && std::strcmp(e, "copy") == 0) ? PDMPC_COLLECTIVE_COPY : PDMPC_COLLECTIVE_RCCL);
    }
    if (repeated && collective == PDMPC_COLLECTIVE_RCCL)
        return fail(PDMPC_ERR_NO_DEVICE, "pdmpc_group_create: a device listed twice needs PDMPC_COLLECTIVE_COPY (RCCL has one rank per device)");
    g->coll = collective == PDMPC_COLLECTIVE_COPY ? &kCollCopy : &kCollRccl;
    std::string err;
    if (g->coll == &kCollRccl && !load_rccl(err)) return fail(PDMPC_ERR_NO_DEVICE, err);
    g->buf.resize((size_t)n_devices);
    for (int r = 0; r < n_devices; ++r) {
        pdmpc_config c = *config;
        c.device = g->dev[(size_t)r];
        pdmpc_handle* h = nullptr;
        GRC(pdmpc_create(&c, &h));
        g->h.push_back(h);
        const int share = (int)std::count(g->dev.begin(), g->dev.end(), g->dev[(size_t)r]);
        if (share > 1) (void)pdmpc_set_device_share(h, share);  // (logical ranks: their launches run side by side on one GPU)
        void* st = nullptr;
        (void)pdmpc_stream(h, &st);
        g->stream.push_back((hipStream_t)st);
        void* records = nullptr;  // (allocated with the handle for max_vehicles records: it does not move)
        size_t nbytes = 0;
        (void)pdmpc_result_device_buffer(h, &records, &nbytes);
        g->rec.push_back((const pdmpc_vehicle_out*)records);
    }
    if (g->coll == &kCollRccl) {
        g->comm.assign((size_t)n_devices, nullptr);
        const ncclResult_t nr = g_rccl.CommInitAll(g->comm.data(), n_devices, g->dev.data());
        if (nr != ncclSuccess) {
            g->comm.clear();
            return fail(PDMPC_ERR_HIP, std::string("ncclCommInitAll failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(nr) : "?"));
        }
        return PDMPC_OK;
    }
    for (int r = 0; r < n_devices; ++r) {
        // (an event the group holds is destroyed with it: each is pushed as soon as it exists)
        for (auto* events : {&g->ev_sent, &g->ev_got}) {
            hipEvent_t e = nullptr;
            if (hipSetDevice(g->dev[(size_t)r]) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
                return fail(PDMPC_ERR_HIP, "pdmpc_group_create: hipEventCreate failed");
            events->push_back(e);
        }
        // peer access between the distinct devices of the group (a copy between devices without it goes through the host)
        for (int q = 0; q < n_devices; ++q)
            if (g->dev[(size_t)q] != g->dev[(size_t)r]) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, g->dev[(size_t)r], g->dev[(size_t)q]) == hipSuccess && can) {
                    const hipError_t pe = hipDeviceEnablePeerAccess(g->dev[(size_t)q], 0);
                    if (pe != hipSuccess) (void)hipGetLastError();  // (already enabled: fine)
                }
            }
    }
    return PDMPC_OK;
}

}  // namespace

extern "C" {

int pdmpc_group_partition(int32_t n, const int32_t* pred_offset, const int32_t* pred_index, const double* weights, int32_t n_devices, int32_t mode, int32_t* rank_of,
                          int32_t* level_of, int32_t* block_rank) {
    if (n < 0 || n_devices < 1 || !rank_of) return fail(PDMPC_ERR_INVALID, "pdmpc_group_partition: bad argument");
    if (!known_mode(mode)) return fail(PDMPC_ERR_INVALID, "unknown sharding mode");
    Partition P;
    GRC(make_partition(n, pred_offset, pred_index, weights, n_devices, mode, P));
    for (int v = 0; v < n; ++v) {
        rank_of[v] = -1;
        if (level_of) level_of[v] = 0;
        if (block_rank) block_rank[v] = -1;
    }
    for (int r = 0; r < n_devices; ++r)
        for (int s : P.parts[(size_t)r]) rank_of[s] = r;
    int first = 0;
    for (size_t l = 0; l < P.level_sizes.size(); ++l) {
        const int size = P.level_sizes[l], per = (size + n_devices - 1) / n_devices;
        for (int i = 0; i < size; ++i) {
            const int s = P.shared[(size_t)(first + i)];
            if (level_of) level_of[s] = (int32_t)l + 1;
            if (block_rank) block_rank[s] = i / per;
        }
        first += size;
    }
    return PDMPC_OK;
}

int pdmpc_group_create_ex(const pdmpc_config* config, int32_t n_devices, const int32_t* devices, int32_t collective, pdmpc_group** out_group) {
    if (!config || !out_group || n_devices < 1 || n_devices > 64) return fail(PDMPC_ERR_INVALID, "pdmpc_group_create: bad argument");
    if (collective != PDMPC_COLLECTIVE_AUTO && collective != PDMPC_COLLECTIVE_RCCL && collective != PDMPC_COLLECTIVE_COPY)
        return fail(PDMPC_ERR_INVALID, "pdmpc_group_create_ex: unknown collective");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PDMPC_ERR_NO_DEVICE, "no HIP device visible: this backend has no CPU fallback");
    DeviceGuard keep;
    pdmpc_group* g = new pdmpc_group();
    const int rc = group_init(g, config, n_devices, devices, collective, ndev);
    if (rc) {
        const std::string why = pdmpc_last_error();  // (what the group's end reports is not why it was not made)
        pdmpc_group_destroy(g);
        return fail(rc, why);
    }
    *out_group = g;
    return PDMPC_OK;
}

int pdmpc_group_create(const pdmpc_config* config, int32_t n_devices, const int32_t* devices, pdmpc_group** out_group) {
    return pdmpc_group_create_ex(config, n_devices, devices, PDMPC_COLLECTIVE_AUTO, out_group);
}

int pdmpc_group_collective(pdmpc_group* g, int32_t* collective) {
    if (!g || !collective) return fail(PDMPC_ERR_INVALID, "null argument");
    *collective = g->coll == &kCollCopy ? PDMPC_COLLECTIVE_COPY : PDMPC_COLLECTIVE_RCCL;
    return PDMPC_OK;
}

int pdmpc_group_destroy(pdmpc_group* g) {
    if (!g) return PDMPC_OK;
    DeviceGuard keep;
    for (size_t r = 0; r < g->h.size(); ++r) (void)pdmpc_synchronize(g->h[r]);
    for (hipEvent_t e : g->ev_sent) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev_got) (void)hipEventDestroy(e);
    for (ncclComm_t c : g->comm)
        if (c && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c);
    // the buffers while the handles' streams still exist, each rank's on its device
    while (!g->buf.empty()) {
        (void)hipSetDevice(g->dev[g->buf.size() - 1]);
        g->buf.pop_back();
    }
    g->pin_lists.release();
    g->pin_out.release();
    for (pdmpc_handle* h : g->h) (void)pdmpc_destroy(h);
    delete g;
    return PDMPC_OK;
}

int pdmpc_group_size(pdmpc_group* g, int32_t* n_devices) {
    if (!g || !n_devices) return fail(PDMPC_ERR_INVALID, "null argument");
    *n_devices = (int32_t)g->h.size();
    return PDMPC_OK;
}

int pdmpc_group_handle(pdmpc_group* g, int32_t rank, pdmpc_handle** handle) {
    if (!g || !handle || rank < 0 || rank >= (int32_t)g->h.size()) return fail(PDMPC_ERR_INVALID, "pdmpc_group_handle: bad argument");
    *handle = g->h[(size_t)rank];
    return PDMPC_OK;
}

int pdmpc_group_upload_mpa(pdmpc_group* g, const pdmpc_mpa* mpa) {
    if (!g || !mpa) return fail(PDMPC_ERR_INVALID, "null argument");
    DeviceGuard keep;
    for (pdmpc_handle* h : g->h) GRC(pdmpc_upload_mpa(h, mpa));
    return PDMPC_OK;
}

int pdmpc_group_plan_step(pdmpc_group* g, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index, const pdmpc_polygon_set* fallback_shapes,
                          const double* weights, int32_t mode, pdmpc_vehicle_out* out) {
    GRC(check_step_args("pdmpc_group_plan_step: null argument", !g || n < 0 || (n > 0 && (!in || !out)), pred_offset, pred_index, mode));
    if (n == 0) return PDMPC_OK;
    DeviceGuard keep;
    new_call(g);
    // (a sampled step is packed again with the seeds its first pack consumed)
    const PendingSeeds pending = g->seeds;
    return plan_growing(g, "pdmpc_group_plan_step", [&](bool& overflow) {
        const auto t0 = clk::now();
        g->seeds = pending;
        GRC(group_pack(g, 0, n, in, pred_offset, pred_index, fallback_shapes, weights, mode));
        GRC(group_launch(g, 0));
        GRC(group_fetch(g, 0, n, out));
        g->timing[0] = ms_between(t0, clk::now());
        for (int i = 0; i < n; ++i) overflow = overflow || out[i].status == PDMPC_ARENA_OVERFLOW;
        return (int)PDMPC_OK;
    });
}

int pdmpc_group_pack_step(pdmpc_group* g, int32_t bank, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                          const pdmpc_polygon_set* fallback_shapes, const double* weights, int32_t mode) {
    const bool null_argument = !g || n < 0 || (n > 0 && !in);
    if (!null_argument && (bank < 0 || bank >= kGroupBanks)) return fail(PDMPC_ERR_INVALID, "pdmpc_group_pack_step: bank out of range");
    GRC(check_step_args("pdmpc_group_pack_step: null argument", null_argument, pred_offset, pred_index, mode));
    DeviceGuard keep;
    return group_pack(g, bank, n, in, pred_offset, pred_index, fallback_shapes, weights, mode);
}

int pdmpc_group_launch(pdmpc_group* g, int32_t bank) {
    if (!g || bank < 0) return fail(PDMPC_ERR_INVALID, "pdmpc_group_launch: bad argument");
    DeviceGuard keep;
    new_call(g);
    return group_launch(g, bank);
}

int pdmpc_group_fetch(pdmpc_group* g, int32_t bank, int32_t n, pdmpc_vehicle_out* out) {
    if (!g || bank < 0 || (n > 0 && !out)) return fail(PDMPC_ERR_INVALID, "pdmpc_group_fetch: bad argument");
    DeviceGuard keep;
    new_call(g);
    return group_fetch(g, bank, n, out);
}

int pdmpc_group_grow_arena(pdmpc_group* g, int32_t max_nodes) {
    if (!g || max_nodes <= 0) return fail(PDMPC_ERR_INVALID, "pdmpc_group_grow_arena: bad argument");
    DeviceGuard keep;
    for (pdmpc_handle* h : g->h) {
        int32_t nodes = 0;
        GRC(pdmpc_arena_nodes(h, &nodes, nullptr));
        if (nodes < max_nodes) GRC(pdmpc_grow_arena(h, max_nodes));
    }
    return PDMPC_OK;
}

int pdmpc_group_last_timing(pdmpc_group* g, double* ms6) {
    if (!g || !ms6) return fail(PDMPC_ERR_INVALID, "null argument");
    for (int i = 0; i < 6; ++i) ms6[i] = g->timing[i];
    return PDMPC_OK;
}

int pdmpc_group_last_exchange(pdmpc_group* g, int64_t* out4) {
    if (!g || !out4) return fail(PDMPC_ERR_INVALID, "null argument");
    for (int i = 0; i < 4; ++i) out4[i] = g->xchg[i];
    return PDMPC_OK;
}

int pdmpc_group_route_host(int32_t n, const int32_t* pred_offset, const int32_t* pred_index, const double* weights, int32_t n_devices, int32_t mode, int32_t* rank,
                           int32_t* position) {
    GRC(check_step_args("pdmpc_group_route_host: bad argument", n < 0 || n_devices < 1 || (n > 0 && (!rank || !position)), pred_offset, pred_index, mode));
    Partition P;
    GRC(make_partition(n, pred_offset, pred_index, weights, n_devices, mode, P));
    GroupRoute R;
    route_partition(P, n, R);
    for (int v = 0; v < n; ++v) {
        rank[v] = R.rank[(size_t)v];
        position[v] = R.pos[(size_t)v];
    }
    return PDMPC_OK;
}

int pdmpc_group_set_step_seeds(pdmpc_group* g, int32_t n, const uint32_t* seeds) {
    if (!g || n < 0 || (n > 0 && !seeds)) return fail(PDMPC_ERR_INVALID, "pdmpc_group_set_step_seeds: bad argument");
    g->seeds.assign(seeds, n);
    return PDMPC_OK;
}

int pdmpc_group_set_sampled_budget(pdmpc_group* g, int32_t n_expansions_max) {
    if (!g) return fail(PDMPC_ERR_INVALID, "pdmpc_group_set_sampled_budget: null group");
    if (n_expansions_max < 1 || n_expansions_max > PDMPC_SAMPLED_BUDGET_MAX) return fail(PDMPC_ERR_INVALID, "pdmpc_group_set_sampled_budget: the budget must be in 1..PDMPC_SAMPLED_BUDGET_MAX");
    for (pdmpc_handle* h : g->h) GRC(pdmpc_set_sampled_budget(h, n_expansions_max));
    return PDMPC_OK;
}

int pdmpc_group_set_sampled_ensemble(pdmpc_group* g, int32_t n_members) {
    if (!g) return fail(PDMPC_ERR_INVALID, "pdmpc_group_set_sampled_ensemble: null group");
    if (n_members < 1 || n_members > PDMPC_SAMPLED_ENSEMBLE_MAX) return fail(PDMPC_ERR_INVALID, "pdmpc_group_set_sampled_ensemble: the ensemble size must be in 1..PDMPC_SAMPLED_ENSEMBLE_MAX");
    for (pdmpc_handle* h : g->h) GRC(pdmpc_set_sampled_ensemble(h, n_members));
    return PDMPC_OK;
}

int pdmpc_group_plan_step_lean(pdmpc_group* g, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                               const pdmpc_polygon_set* fallback_shapes, const double* weights, int32_t mode, int32_t* status, double* final_cost) {
    GRC(check_step_args("pdmpc_group_plan_step_lean: null argument", !g || n < 0 || (n > 0 && (!in || !status || !final_cost)), pred_offset, pred_index, mode));
    DeviceGuard keep;
    new_call(g);
    const auto t0 = clk::now();
    GRC(group_pack(g, 0, n, in, pred_offset, pred_index, fallback_shapes, weights, mode));
    if (n == 0) return PDMPC_OK;
    const GroupRoute& R = g->plans[0].route;
    const size_t world = g->h.size(), block = ((size_t)R.per + 1) * sizeof(GroupEntry);
    GRC(grow_pin_out(g, world * block));
    return plan_growing(g, "pdmpc_group_plan_step_lean", [&](bool& overflow) {
        // every rank writes the entries of the records it holds straight into host memory: no record and no collective ends this step
        const auto t2 = clk::now();
        GRC(group_enqueue(g, 0, false));
        GRC(enqueue_entries(g, [&](size_t r) { return held_of_bank(g, g->plans[0], r); }, [&](size_t r) { return g->buf[r].pin_out + r * block; }));
        const auto t3 = clk::now();
        GRC(group_wait(g));
        GRC(group_launched(g, 0, false));
        const auto t4 = clk::now();
        g->xchg[1] += (int64_t)(((size_t)n + world) * sizeof(GroupEntry));
        const GroupEntry* ent = (const GroupEntry*)g->pin_out.p;
        for (int v = 0; v < n; ++v) {
            const GroupEntry& e = ent[R.entry(v)];
            status[v] = e.status;
            final_cost[v] = e.cost;
            overflow = overflow || e.status == PDMPC_ARENA_OVERFLOW;
        }
        g->timing[3] = ms_between(t2, t3);
        g->timing[4] = ms_between(t3, t4);
        g->timing[5] = ms_between(t4, clk::now());
        g->timing[0] = ms_between(t0, clk::now());
        return (int)PDMPC_OK;
    });
}

int pdmpc_group_fetch_records_at(pdmpc_group* g, int32_t count, const int32_t* vehicles, pdmpc_vehicle_out* out) {
    if (!g || count < 0 || (count > 0 && (!vehicles || !out))) return fail(PDMPC_ERR_INVALID, "pdmpc_group_fetch_records_at: null argument");
    const pdmpc_group::Plan* L = nullptr;
    GRC(resident_plan(g, g->resident_bank, "pdmpc_group_fetch_records_at", &L));
    for (int i = 0; i < count; ++i)
        if (vehicles[i] < 0 || vehicles[i] >= L->n) return fail(PDMPC_ERR_INVALID, "vehicle index outside the packed step");
    DeviceGuard keep;
    new_call(g);
    const auto t4 = clk::now();
    if (count == 0) return PDMPC_OK;
    GRC(grow_pin_out(g, (size_t)count * kRec));
    // each wanted record from the rank that holds it, on that rank's stream
    for (int i = 0; i < count; ++i) {
        const size_t r = (size_t)L->route.rank[(size_t)vehicles[i]];
        const int32_t p = L->route.pos[(size_t)vehicles[i]];
        const Held H = held_of_bank(g, *L, r);
        const pdmpc_vehicle_out* src = p < H.n_a ? H.rec_a + p : H.rec_b + (p - H.n_a);
        HIPCHK(hipSetDevice(g->dev[r]));
        HIPCHK(hipMemcpyAsync(g->pin_out.p + (size_t)i * kRec, src, kRec, hipMemcpyDeviceToHost, g->stream[r]));
    }
    GRC(group_wait(g));
    g->xchg[1] += (int64_t)((size_t)count * kRec);
    std::memcpy(out, g->pin_out.p, (size_t)count * kRec);
    g->timing[5] = ms_between(t4, clk::now());
    return PDMPC_OK;
}

int pdmpc_group_plan_step_chosen(pdmpc_group* g, int32_t n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index,
                                 const pdmpc_polygon_set* fallback_shapes, const double* weights, int32_t mode, const pdmpc_choice* ch, int32_t* chosen,
                                 double* cell_cost, pdmpc_vehicle_out* picks) {
    GRC(check_step_args("pdmpc_group_plan_step_chosen: null argument", !g || n < 0 || (n > 0 && !in) || (ch && ch->n_picks > 0 && !picks), pred_offset, pred_index, mode));
    GRC(checked_choice(n, ch));
    DeviceGuard keep;
    new_call(g);
    const auto t0 = clk::now();
    GRC(group_pack(g, 0, n, in, pred_offset, pred_index, fallback_shapes, weights, mode));
    const pdmpc_group::Plan& L = g->plans[0];
    const StagedChoice S(*ch);
    GRC(stage_group_choice(g, L.route, S));  // (once: a step that is planned again with larger arenas chooses on the same lists)
    // (an overflow that cannot grow fails the choice below: a record that outgrew its arena is no planning result)
    GRC(plan_growing(g, "pdmpc_group_plan_step_chosen", [&](bool& overflow) {
        const auto t2 = clk::now();
        GRC(group_enqueue(g, 0, false));
        GRC(enqueue_group_choice(g, L.route, S, [&](size_t r) { return held_of_bank(g, L, r); }));
        const auto t3 = clk::now();
        GRC(group_wait(g));
        GRC(group_launched(g, 0, false));
        g->timing[3] = ms_between(t2, t3);
        g->timing[4] = ms_between(t3, clk::now());
        overflow = ((const int32_t*)g->pin_out.p)[PDMPC_CHOICE_OVERFLOW] != 0;
        return (int)PDMPC_OK;
    }));
    const auto t4 = clk::now();
    const int rc = deliver_group_choice(g, S, chosen, cell_cost, picks);
    g->timing[5] = ms_between(t4, clk::now());
    g->timing[0] = ms_between(t0, clk::now());
    return rc;
}

int pdmpc_group_choose_resident(pdmpc_group* g, int32_t bank, int32_t n, const pdmpc_choice* ch, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks) {
    if (!g || (ch && ch->n_picks > 0 && !picks)) return fail(PDMPC_ERR_INVALID, "pdmpc_group_choose_resident: null argument");
    GRC(checked_choice(n, ch));
    const pdmpc_group::Plan* L = nullptr;
    GRC(resident_plan(g, bank, "pdmpc_group_choose_resident", &L));
    if (n != L->n) return fail(PDMPC_ERR_INVALID, "pdmpc_group_choose_resident: the bank holds another number of vehicles");
    DeviceGuard keep;
    new_call(g);
    const StagedChoice S(*ch);
    GRC(stage_group_choice(g, L->route, S));
    GRC(enqueue_group_choice(g, L->route, S, [&](size_t r) { return held_of_bank(g, *L, r); }));
    GRC(group_wait(g));
    return deliver_group_choice(g, S, chosen, cell_cost, picks);
}

int pdmpc_group_debug_choose(pdmpc_group* g, int32_t n, const pdmpc_vehicle_out* records, const int32_t* rank_of, const pdmpc_choice* ch, int32_t* chosen,
                             double* cell_cost, pdmpc_vehicle_out* picks) {
    if (!g || n < 0 || (n > 0 && (!records || !rank_of)) || (ch && ch->n_picks > 0 && !picks)) return fail(PDMPC_ERR_INVALID, "pdmpc_group_debug_choose: null argument");
    GRC(checked_choice(n, ch));
    GroupRoute R;
    const size_t world = g->h.size();
    if (!route_placed(n, rank_of, (int)world, R)) return fail(PDMPC_ERR_INVALID, "pdmpc_group_debug_choose: rank_of outside [-1, world)");
    DeviceGuard keep;
    // the records where the route says they are: a rank's own in ascending order; the records of every rank (rank_of == -1) behind
    // them on EVERY rank, as the level exchange leaves a shared component's (rank 0 is their holder)
    std::vector<pdmpc_vehicle_out> own, everywhere;
    for (int v = 0; v < n; ++v)
        if (rank_of[v] < 0) everywhere.push_back(records[v]);
    GRC(grow_on_ranks(g, &RankBufs::placed, (size_t)R.per + everywhere.size() + 1));
    for (size_t r = 0; r < world; ++r) {
        own.clear();
        for (int v = 0; v < n; ++v)
            if (rank_of[v] == (int32_t)r) own.push_back(records[v]);
        HIPCHK(hipSetDevice(g->dev[r]));
        if (!own.empty()) HIPCHK(hipMemcpy(g->buf[r].placed.p, own.data(), own.size() * kRec, hipMemcpyHostToDevice));
        if (!everywhere.empty()) HIPCHK(hipMemcpy(g->buf[r].placed.p + own.size(), everywhere.data(), everywhere.size() * kRec, hipMemcpyHostToDevice));
    }
    // ... and from here on exactly what a step's choice runs
    new_call(g);
    const StagedChoice S(*ch);
    GRC(stage_group_choice(g, R, S));
    GRC(enqueue_group_choice(g, R, S, [&](size_t r) { return held_placed(g, R, r); }));
    GRC(group_wait(g));
    return deliver_group_choice(g, S, chosen, cell_cost, picks);
}

}  // extern "C"
