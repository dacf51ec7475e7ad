// sampled_launch.hpp — the sampled optimizer's host side on a handle (SampledState, handle.hpp): the scratch a pack reserves for its
// bank (pack.cpp) and the launch of a sampled bank (api.cpp: launch_range and timed_launch, which keep the checks, the timing and the
// failure text it shares with the graph search).  Everything a sampled kernel is given is put together here, in sampled_args: no sampled launch
// touches KernelArgs, the helper boards or the search's launch counter.  Private to the library.
#pragma once
#include <algorithm>
#include <string>

#include "handle.hpp"

// What a sampled bank needs besides its batch (SampledNeed): the handle's scratch grown to it by the pack, once the bank's size is
// known.  The reference's budget with one member needs none and is not planned for.
inline int reserve_sampled_scratch(pdmpc_handle* h, const PackedStep& B) {
    if (!B.sampled.on || B.sampled.reference()) return PDMPC_OK;
    LaunchPlan plan;
    SampledExtra extra;
    std::string err;
    if (const int rc = plan_sampled(h->tune, launch_dims(h, B), B.sampled.budget, B.sampled.members, std::max(B.n_packed, 1), false, plan, extra, err)) return fail(rc, err);
    const SampledNeed need = sampled_need(B.sampled, B.n_packed, extra);
    SampledState& S = h->sampled;
    if (S.holds_trees(need) && S.holds_members(need)) return PDMPC_OK;
    HIPCHK(sync_stream(h));  // (a launch of a resident bank may still use a buffer that is freed)
    if (S.grow_trees(need)) return fail(PDMPC_ERR_CAPACITY, "not enough HBM for the sampled optimizer's trees at this budget");
    if (S.grow_members(need)) return fail(PDMPC_ERR_CAPACITY, "not enough HBM for the records of the sampled optimizer's ensemble members");
    return PDMPC_OK;
}

// The arguments of a sampled launch of slots [first, first + count) of bank B: the record of all three kernels, from the handle, the
// bank, the plan and what plan_sampled decided besides it.
inline SampledArgs sampled_args(const pdmpc_handle* h, const PackedStep& B, const LaunchPlan& plan, const SampledExtra& extra, int first, int count) {
    SampledArgs a{};
    set_batch_args(h, B, plan.areas_in_lds, a);
    a.checker = h->cfg.checker;
    a.pred = B.dev.pred;
    a.done_flag = h->d_flag.p;
    a.epoch = h->epoch;
    a.first = first;
    a.n_searches = count;
    a.reverse_dispatch = plan.reverse_dispatch;
    a.spin_limit = plan.spin_limit;
    a.lds = plan.lds;
    a.budget = B.sampled.budget;
    a.node_cap = extra.node_cap;
    a.tree = extra.tree_in_lds ? nullptr : h->sampled.tree.p;
    return a;
}

// One launch of a sampled bank, in the two steps timed_launch times: prepare (everything that can be refused, and what the stream does
// ahead of the kernels) and go (the kernels).
struct SampledLaunch {
    SampledEnsembleArgs en{};  // en.s: what every sampled kernel takes; around it what an ensemble's kernels take (members > 1)

    // The bank plans with the budget and the ensemble size it was packed with: the first launch, a resident one and the re-plan in
    // slices alike.
    int prepare(pdmpc_handle* h, const PackedStep& B, int first, int count, bool safe, LaunchPlan& plan) {
        SampledExtra extra;
        std::string err;
        if (const int rc = plan_sampled(h->tune, launch_dims(h, B), B.sampled.budget, B.sampled.members, count, safe, plan, extra, err)) return fail(rc, err);
        SampledState& S = h->sampled;
        const SampledNeed need = sampled_need(B.sampled, B.n_packed, extra);
        if (!S.holds_trees(need)) return fail(PDMPC_ERR_CAPACITY, "the sampled optimizer's trees in HBM were not allocated by this bank's pack");
        if (!S.holds_members(need)) return fail(PDMPC_ERR_CAPACITY, "the records of the ensemble's members were not allocated by this bank's pack");
        en = SampledEnsembleArgs{sampled_args(h, B, plan, extra, first, count), B.sampled.members, S.member_out.p, S.member_entry.p, S.ticket.p, S.member_nodes.p, S.chosen.p};
        if (en.n_members > 1) {
            // every slot's ticket is zero when its members start, whatever the last launch of these slots left: a launch that failed, a
            // resident re-launch and the re-plan in slices all pass here
            HIPCHK(hipMemsetAsync(S.ticket.p + first, 0, (size_t)count * sizeof(uint32_t), h->stream));
            S.ensemble_bank = h->bank;
        }
        S.last_kernel = plan.kernel;
        return PDMPC_OK;
    }

    // The kernel launches, plan.slice slots each (the safe mode: a slice is resident as a whole, an ensemble's with all its members);
    // returns the hipError_t of the first that failed.  The kernel: the reference's for a bank that is one (SampledBank::reference),
    // else the ensemble's for two or more members, else the run-time budget's.
    int go(const pdmpc_handle* h, const LaunchPlan& plan) const {
        const bool reference = en.n_members == 1 && en.s.budget == PDMPC_SAMPLED_BUDGET_DEFAULT;
        int lrc = 0;
        for (int done = 0; done < en.s.n_searches && lrc == 0; done += plan.slice) {
            SampledEnsembleArgs part = en;
            part.s.first = en.s.first + done;
            part.s.n_searches = std::min(plan.slice, en.s.n_searches - done);
            if (reference)
                lrc = pdmpc_launch_sampled(&part.s, part.s.n_searches, (void*)h->stream);
            else if (en.n_members > 1)
                lrc = pdmpc_launch_sampled_ensemble(&part, part.s.n_searches, (void*)h->stream);
            else
                lrc = pdmpc_launch_sampled_budget(&part.s, part.s.n_searches, (void*)h->stream);
        }
        return lrc;
    }
};
