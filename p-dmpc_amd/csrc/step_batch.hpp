// step_batch.hpp — the batch of prioritizations of an explorative or optimal-priority step (step_controller.cpp, stage 7 of 9): its
// instances, kept and flattened, and the choice among their plans as data.
#pragma once
#include <algorithm>

#include "step_assembly.hpp"

namespace {
// ---- the batch of prioritizations of an explorative or optimal-priority step: its instances, kept and flattened
// the batch of K instances: sized before the first keep_instance (copies into vectors that are kept from step to step: no allocation
// once warm)
inline void begin_instances(pdmpc_controller* c, int K) {
    if (c->x.inst_prob.size() < (size_t)K) c->x.inst_prob.resize((size_t)K);
    if (c->x.inst.size() != (size_t)K) c->x.inst.resize((size_t)K);
}

// the problem assemble_step just left in the controller becomes instance p
inline void keep_instance(pdmpc_controller* c, int p) {
    c->x.inst_prob[(size_t)p] = c->prob;
    c->x.inst_prob[(size_t)p].seeds.clear();  // (they are those of the step's own slot order, which need not be the instance's)
    c->x.inst[(size_t)p] = c->pri;
}

// flatten instances 0 .. K-1 into one batch, slots ordered by (level, instance, slot), and seed it; then instance 0 is the controller's
// problem again
inline void flatten_instances(pdmpc_controller* c, int K) {
    const int n = c->sc.n;
    StepProblem& X = c->x.prob;
    struct Key {
        int32_t level, p, s;
    };
    std::vector<Key> flat;
    for (int p = 0; p < K; ++p)
        for (int s = 0; s < n; ++s) flat.push_back(Key{c->x.inst[(size_t)p].levels[(size_t)c->x.inst[(size_t)p].order[(size_t)s]], p, s});
    std::stable_sort(flat.begin(), flat.end(), [](const Key& a, const Key& b) { return a.level < b.level; });  // (generated in (p, s) order)
    const int N = K * n;
    std::vector<int32_t> slot_of((size_t)N);  // [p * n + s]
    for (int i = 0; i < N; ++i) slot_of[(size_t)flat[(size_t)i].p * n + flat[(size_t)i].s] = i;
    X.in.resize((size_t)N);
    X.fb.resize((size_t)N);
    X.pred_offset.assign((size_t)N + 1, 0);
    X.pred_index.clear();
    c->x.instance.resize((size_t)N);
    c->x.vehicle.resize((size_t)N);
    c->x.level.resize((size_t)N);
    c->x.slot.assign((size_t)N, 0);
    for (int i = 0; i < N; ++i) {
        const Key& k = flat[(size_t)i];
        const StepProblem& P = c->x.inst_prob[(size_t)k.p];
        X.in[(size_t)i] = P.in[(size_t)k.s];
        X.fb[(size_t)i] = P.fb[(size_t)k.s];
        for (int32_t q = P.pred_offset[(size_t)k.s]; q < P.pred_offset[(size_t)k.s + 1]; ++q) X.pred_index.push_back(slot_of[(size_t)k.p * n + P.pred_index[(size_t)q]]);
        X.pred_offset[(size_t)i + 1] = (int32_t)X.pred_index.size();
        c->x.instance[(size_t)i] = k.p;
        c->x.vehicle[(size_t)i] = c->x.inst[(size_t)k.p].order[(size_t)k.s];
        c->x.level[(size_t)i] = k.level;
        c->x.slot[(size_t)k.p * n + c->x.vehicle[(size_t)i]] = i;
    }
    X.pred_index.push_back(0);
    set_seeds(c->tr.k, X, c->x.vehicle);
    c->x.built_last = true;
    // the controller's own problem again (instance 0), with the seeds of its slots
    c->prob = c->x.inst_prob[0];
    c->pri = c->x.inst[0];
    set_seeds(c->tr.k, c->prob, c->pri.order);
}

// pdmpc_controller_explore_build behind its pdmpc_controller_build_step (build_members runs that part for all its members at once, then
// this one per member): the step just built is instance 0, instances 1 .. n_perm - 1 permute its computation levels
inline int permute_instances(pdmpc_controller* c, int32_t n_perm, uint32_t seed) {
    int rc = PDMPC_OK;
    const int n = c->sc.n;
    // base levels: the computation levels of the controller's own prioritization -- kahn of the sequential coupling the step was
    // just built with, whatever the priority strategy (PrioritizedExplorativeController.m prepare_permutation :42-58 permutes
    // kahn(iter.directed_coupling_sequential))
    const std::vector<int32_t> levels0 = c->pri.levels;
    const int n_levels = *std::max_element(levels0.begin(), levels0.end());
    std::vector<int32_t> perms((size_t)n_perm * n_levels);
    rc = pdmpc_exploration_permutations(n_levels, n_perm, seed, perms.data());
    if (rc) return rc;
    begin_instances(c, n_perm);
    keep_instance(c, 0);
    std::vector<int32_t> where;
    for (int p = 1; p < n_perm; ++p) {
        where.assign((size_t)n_levels + 1, 0);
        for (int j = 0; j < n_levels; ++j) where[(size_t)perms[(size_t)p * n_levels + j]] = j + 1;
        // prepare_permutation (:64-77): every coupling i -> j of the base prioritization whose permuted levels invert it is swapped
        // in ALL coupling matrices (swap_entries_all_coupling_matrices): a sequential coupling stays sequential, a parallel one
        // (cut by the grouping, or between vehicles of one level) stays parallel and keeps its direction
        const Instance& I0 = c->x.inst[0];
        c->pri.take_couplings(I0);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (at(I0.directed, n, i, j) && where[(size_t)levels0[i]] > where[(size_t)levels0[j]]) {
                    at(c->pri.directed, n, i, j) = 0;
                    at(c->pri.directed, n, j, i) = 1;
                    if (at(I0.directed_seq, n, i, j)) {
                        at(c->pri.directed_seq, n, i, j) = 0;
                        at(c->pri.directed_seq, n, j, i) = 1;
                    }
                }
        rc = assemble_step(c, true);
        if (rc) return rc;
        keep_instance(c, p);
    }
    flatten_instances(c, n_perm);
    return PDMPC_OK;
}

// pdmpc_controller_optimal_build behind its pdmpc_controller_build_step and the enumeration (build_members runs those for all its
// members at once, then this one per member): the step's traffic state under each of the K unique prioritizations (masks, K x n priorities)
inline int optimal_instances(pdmpc_controller* c, int64_t K, const uint32_t* masks, const int32_t* priorities) {
    const int n = c->sc.n;
    c->x.o_masks.assign(masks, masks + K);
    c->x.o_prio.assign(priorities, priorities + K * n);
    begin_instances(c, (int)K);
    for (int p = 0; p < (int)K; ++p) {
        // ConstantPrioritizer on the given priorities + directed_coupling_from_priorities; then assemble_step groups (cuts to
        // max_num_CLs levels) per instance
        direct_by(c->in.adjacency, n, c->x.o_prio.data() + (size_t)p * n, c->pri.directed);
        if (const int rc = assemble_step(c)) return rc;
        keep_instance(c, p);
    }
    flatten_instances(c, (int)K);
    return PDMPC_OK;
}

// ---- the choice among the plans of a batch, and the step over a batch
// The explorative choice as data: graph g = a weakly connected sub-graph (ordered by smallest vehicle), its candidates the n_perm
// instances, cell (g, p) = the slots of instance p whose vehicles belong to g in ascending slot order (the order the twin adds in).
inline void explore_describe(pdmpc_controller* c, ChoiceLists& D) {
    const int n = c->sc.n, K = (int)c->x.inst.size();
    std::vector<int> label((size_t)n);
    for (int i = 0; i < n; ++i) label[(size_t)i] = i;
    auto find = [&](int a) {
        while (label[(size_t)a] != a) a = label[(size_t)a] = label[(size_t)label[(size_t)a]];
        return a;
    };
    const std::vector<uint8_t>& seq0 = c->x.inst[0].directed_seq;  // conncomp(directed_coupling_sequential) of the base prioritization (:94-112)
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (at(seq0, n, i, j) || at(seq0, n, j, i)) {
                const int a = find(i), b = find(j);
                if (a != b) label[(size_t)std::max(a, b)] = std::min(a, b);
            }
    std::vector<int> roots;
    for (int i = 0; i < n; ++i)
        if (find(i) == i) roots.push_back(i);  // ascending: the graphs ordered by their smallest vehicle
    D.graph_of.resize((size_t)n);
    for (int i = 0; i < n; ++i) D.graph_of[(size_t)i] = (int32_t)(std::lower_bound(roots.begin(), roots.end(), find(i)) - roots.begin());
    const int G = (int)roots.size(), N = K * n;
    D.graph_offset.resize((size_t)G + 1);
    for (int g = 0; g <= G; ++g) D.graph_offset[(size_t)g] = g * K;
    // cell (g, p) at g * K + p: counted, then filled in slot order
    D.cell_offset.assign((size_t)G * K + 1, 0);
    auto cell_of = [&](int s) { return D.graph_of[(size_t)c->x.vehicle[(size_t)s]] * K + c->x.instance[(size_t)s]; };
    for (int s = 0; s < N; ++s) D.cell_offset[(size_t)cell_of(s) + 1] += 1;
    for (int q = 0; q < G * K; ++q) D.cell_offset[(size_t)q + 1] += D.cell_offset[(size_t)q];
    D.cell_slot.resize((size_t)N);
    std::vector<int32_t> fill(D.cell_offset.begin(), D.cell_offset.end() - 1);
    for (int s = 0; s < N; ++s) D.cell_slot[(size_t)fill[(size_t)cell_of(s)]++] = s;
    D.clear_picks();
}
// every vehicle goes on with the couplings of the instance it chose (obj.iter = obj.iter_array_tmp{chosen_solution},
// PrioritizedExplorativeController.m:157-158, PrioritizedOptimalController.m:100): its rows of both matrices -- follow_own (the step
// applies the plans of the controller's OWN prioritization whatever was chosen): the couplings of instance 0 again, which is what
// apply's fallback handling then sees
inline void adopt_chosen_couplings(pdmpc_controller* c, bool follow_own) {
    if (follow_own) return c->pri.take_couplings(c->x.inst[0]);
    const size_t n = (size_t)c->sc.n;
    for (size_t i = 0; i < n; ++i) {
        const Instance& I = c->x.inst[(size_t)c->x.chosen[i]];
        std::copy_n(I.directed.begin() + i * n, n, c->pri.directed.begin() + i * n);
        std::copy_n(I.directed_seq.begin() + i * n, n, c->pri.directed_seq.begin() + i * n);
    }
}
// ... and what the sub-graphs chose becomes the controller's: cost table n_perm x n_graphs, the instance per vehicle, its couplings
inline void explore_adopt(pdmpc_controller* c, const ChoiceLists& D, const int32_t* chosen, const double* cell_cost, bool follow_own) {
    const int n = c->sc.n, K = (int)c->x.inst.size(), G = D.n_graphs();
    c->x.graphs = G;
    c->x.cost.resize((size_t)K * G);
    for (int p = 0; p < K; ++p)
        for (int g = 0; g < G; ++g) c->x.cost[(size_t)p * G + g] = cell_cost[(size_t)g * K + p];
    c->x.chosen.resize((size_t)n);
    for (int i = 0; i < n; ++i) c->x.chosen[(size_t)i] = chosen[(size_t)D.graph_of[(size_t)i]];
    adopt_chosen_couplings(c, follow_own);
}

// How a step over a batch of prioritizations chooses: the description of its choice (cells and graphs) and what adopts the result.
struct BatchChoice {
    void (*describe)(pdmpc_controller*, ChoiceLists&);
    void (*adopt)(pdmpc_controller*, const ChoiceLists&, const int32_t*, const double*, bool follow_own);
    bool graph_per_vehicle;  // the optimal-priority choice: vehicle v's graph is graph v (else its sub-graph)
};
// the choice on the host twin (status and cost-to-come of the final node per slot of the batch: all the choice looks at)
inline int choose_on_host(pdmpc_controller* c, const BatchChoice& how, const int32_t* status, const double* final_cost, bool follow_own) {
    ChoiceLists& D = c->x.choice;
    how.describe(c, D);
    c->x.choice_chosen.resize((size_t)D.n_graphs());
    c->x.choice_cost.resize((size_t)D.n_cells());
    const pdmpc_choice ch = D.view();
    const int rc = pdmpc_choose_host(c->x.prob.n(), status, final_cost, &ch, c->x.choice_chosen.data(), c->x.choice_cost.data());
    if (rc) return cfail(c, rc, pdmpc_last_error());
    how.adopt(c, D, c->x.choice_chosen.data(), c->x.choice_cost.data(), follow_own);
    return PDMPC_OK;
}
// ... from the first N records of the batch: their status and the cost-to-come of their final node
inline int choose_from_records(pdmpc_controller* c, const BatchChoice& how, const pdmpc_vehicle_out* recs, int N, bool follow_own) {
    c->x.status.resize((size_t)N);
    c->x.final_cost.resize((size_t)N);
    for (int s = 0; s < N; ++s) {
        c->x.status[(size_t)s] = recs[s].status;
        c->x.final_cost[(size_t)s] = recs[s].path_nodes[c->sc.Hp][4];
    }
    return choose_on_host(c, how, c->x.status.data(), c->x.final_cost.data(), follow_own);
}

// Reading a batch's records back into the controller's own slot order.  The slot in the batch of the record vehicle v keeps if it goes
// on with instance p -- follow_own: the record of instance 0, whatever it goes on with
inline int32_t kept_slot(const pdmpc_controller* c, bool follow_own, int p, int v) { return c->x.slot[(size_t)(follow_own ? 0 : p) * c->sc.n + v]; }
// ... once the choice is made: of the vehicle in slot s of the controller's own order
inline int32_t kept_slot_at(const pdmpc_controller* c, bool follow_own, int s) {
    const int v = c->pri.order[(size_t)s];
    return kept_slot(c, follow_own, c->x.chosen[(size_t)v], v);
}
// ... those records out of the records of the whole batch (c->x.out) as the step's records (c->out)
inline void gather_kept_records(pdmpc_controller* c, bool follow_own) {
    c->out.resize((size_t)c->sc.n);
    for (int s = 0; s < c->sc.n; ++s) c->out[(size_t)s] = c->x.out[(size_t)kept_slot_at(c, follow_own, s)];
}
// ... and before the choice is made, the picks of a step that chooses on the device and keeps the chosen plans only: per slot of the
// controller's own order the records its vehicle may keep, one per instance
inline void pick_chosen_plans(pdmpc_controller* c, ChoiceLists& D, bool follow_own, bool graph_per_vehicle) {
    const int n = c->sc.n, K = (int)c->x.inst.size();
    D.clear_picks();
    for (int s = 0; s < n; ++s) {
        const int v = c->pri.order[(size_t)s];
        D.pick_graph.push_back(follow_own ? -1 : (graph_per_vehicle ? v : D.graph_of[(size_t)v]));
        for (int p = 0; p < (follow_own ? 1 : K); ++p) D.pick_slot.push_back(kept_slot(c, follow_own, p, v));
        D.pick_offset.push_back((int32_t)D.pick_slot.size());
    }
}

const BatchChoice kExploreChoice = {explore_describe, explore_adopt, false};

// compute_solution_cost / receive_solution_cost / choose_solution (:56-114): every vehicle sums the solution costs of ALL vehicles per
// instance (its own first, then the others' messages in ascending index), rounds to 8 decimals and takes the first minimum
// The optimal-priority choice as data: graph v = vehicle v, its candidates the K instances, cell (v, p) = vehicle v's slot of instance p,
// then the other vehicles' slots of instance p in ascending vehicle index
inline void optimal_describe(pdmpc_controller* c, ChoiceLists& D) {
    const int n = c->sc.n, K = (int)c->x.inst.size();
    D.graph_of.clear();
    D.graph_offset.resize((size_t)n + 1);
    for (int v = 0; v <= n; ++v) D.graph_offset[(size_t)v] = v * K;
    D.cell_offset.resize((size_t)n * K + 1);
    for (int q = 0; q <= n * K; ++q) D.cell_offset[(size_t)q] = q * n;
    D.cell_slot.resize((size_t)n * K * n);
    int32_t* slot = D.cell_slot.data();
    for (int v = 0; v < n; ++v)
        for (int p = 0; p < K; ++p) {
            *slot++ = c->x.slot[(size_t)p * n + v];
            for (int j = 0; j < n; ++j)
                if (j != v) *slot++ = c->x.slot[(size_t)p * n + j];
        }
    D.clear_picks();
}
inline void optimal_adopt(pdmpc_controller* c, const ChoiceLists&, const int32_t* chosen, const double* cell_cost, bool follow_own) {
    const int n = c->sc.n, K = (int)c->x.inst.size();
    c->x.cost.assign(cell_cost, cell_cost + (size_t)n * K);  // row v = vehicle v's sums
    c->x.chosen.assign(chosen, chosen + n);
    c->x.graphs = K;
    adopt_chosen_couplings(c, follow_own);
}
const BatchChoice kOptimalChoice = {optimal_describe, optimal_adopt, true};
}  // namespace
