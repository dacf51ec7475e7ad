// choice_host.hpp — the choice among the plans of a batch (pdmpc_choice, include/pdmpc.h) as far as the host makes it: what a
// choice must promise before anything is launched or summed (check_choice), the words its lists are staged in for the kernels (ChoiceLists,
// stage_choice_lists), the block a device choice reads back and its delivery (ChoiceLayout, deliver_choice), and the sums, rounding and first
// minima of pdmpc_choose_host, the twin and checker of choice_kernel.hip.  Host only: no device header, no device — api.cpp (one device) and
// group.cpp (the ranks of a group) allocate, copy and launch.  `make host-parts` compiles this header alone with the host compiler.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pdmpc_device.h"

// what pdmpc_choice promises, checked before anything is launched or summed
inline int check_choice(int32_t n, const pdmpc_choice* ch, std::string& err) {
    auto refuse = [&err](const char* msg) {
        err = msg;
        return (int)PDMPC_ERR_INVALID;
    };
    if (!ch || n < 0 || ch->n_cells < 0 || ch->n_graphs < 0 || ch->n_picks < 0) return refuse("pdmpc_choice: bad argument");
    if ((ch->n_cells > 0 && !ch->cell_offset) || (ch->n_graphs > 0 && !ch->graph_offset) || (ch->n_picks > 0 && (!ch->pick_graph || !ch->pick_offset)))
        return refuse("pdmpc_choice: null list");
    auto monotone = [](const int32_t* off, int count) {
        if (off[0] < 0) return false;
        for (int i = 0; i < count; ++i)
            if (off[i + 1] < off[i]) return false;
        return true;
    };
    auto slots_within = [n](const int32_t* slot, int first, int end) {
        if (end > first && !slot) return false;
        for (int q = first; q < end; ++q)
            if (slot[q] < 0 || slot[q] >= n) return false;
        return true;
    };
    if (ch->n_cells > 0) {
        if (!monotone(ch->cell_offset, ch->n_cells)) return refuse("pdmpc_choice: cell offsets are negative or decrease");
        if (!slots_within(ch->cell_slot, 0, ch->cell_offset[ch->n_cells])) return refuse("pdmpc_choice: a cell lists a slot outside the batch");
    }
    if (ch->n_graphs > 0) {
        if (!monotone(ch->graph_offset, ch->n_graphs)) return refuse("pdmpc_choice: graph offsets are negative or decrease");
        if (ch->graph_offset[ch->n_graphs] > ch->n_cells) return refuse("pdmpc_choice: a graph's candidates lie outside the cells");
    }
    if (ch->n_picks > 0) {
        if (!monotone(ch->pick_offset, ch->n_picks)) return refuse("pdmpc_choice: pick offsets are negative or decrease");
        for (int i = 0; i < ch->n_picks; ++i) {
            const int g = ch->pick_graph[i];
            if (g < -1 || g >= ch->n_graphs) return refuse("pdmpc_choice: pick_graph outside [-1, n_graphs)");
            const int want = g < 0 ? 1 : ch->graph_offset[g + 1] - ch->graph_offset[g];
            if (want < 1 || ch->pick_offset[i + 1] - ch->pick_offset[i] != want) return refuse("pdmpc_choice: a pick lists another number of slots than its graph has candidates");
        }
        if (!slots_within(ch->pick_slot, 0, ch->pick_offset[ch->n_picks])) return refuse("pdmpc_choice: a pick lists a slot outside the batch");
    }
    return PDMPC_OK;
}

extern "C" void pdmpc_set_last_error(const char* msg);  // api.cpp: the string pdmpc_last_error returns
// ... as the library's entry points report it
inline int checked_choice(int32_t n, const pdmpc_choice* ch) {
    std::string err;
    const int rc = check_choice(n, ch, err);
    if (rc) pdmpc_set_last_error(err.c_str());
    return rc;
}

// Where the lists of a checked choice lie in the int32 words the kernels read (the argument structs of choice_kernel.hip and
// group_choice_kernel.hip point into them): cell_offset | cell slots | graph_offset | pick_graph | pick_offset | pick slots.
struct ChoiceLists {
    size_t cell_offset = 0, cell_slot = 0, graph_offset = 0, pick_graph = 0, pick_offset = 0, pick_slot = 0, words = 0;
    explicit ChoiceLists(const pdmpc_choice& ch) {
        cell_slot = cell_offset + (size_t)ch.n_cells + 1;
        graph_offset = cell_slot + (size_t)(ch.n_cells > 0 ? ch.cell_offset[ch.n_cells] : 0);
        pick_graph = graph_offset + (size_t)ch.n_graphs + 1;
        pick_offset = pick_graph + (size_t)ch.n_picks;
        pick_slot = pick_offset + (size_t)ch.n_picks + 1;
        words = pick_slot + (size_t)(ch.n_picks > 0 ? ch.pick_offset[ch.n_picks] : 0);
    }
};

// ... and the lists in w[L.words]; map_slots(slot, count, to) writes where the kernel finds the records of `count` of the caller's slots
template <class MapSlots>
inline void stage_choice_lists(const pdmpc_choice& ch, const ChoiceLists& L, int32_t* w, MapSlots&& map_slots) {
    w[L.cell_offset] = w[L.graph_offset] = w[L.pick_offset] = 0;  // (an empty list is its offset 0)
    if (ch.n_cells > 0) {
        std::memcpy(w + L.cell_offset, ch.cell_offset, ((size_t)ch.n_cells + 1) * sizeof(int32_t));
        map_slots(ch.cell_slot, ch.cell_offset[ch.n_cells], w + L.cell_slot);
    }
    if (ch.n_graphs > 0) std::memcpy(w + L.graph_offset, ch.graph_offset, ((size_t)ch.n_graphs + 1) * sizeof(int32_t));
    if (ch.n_picks > 0) {
        std::memcpy(w + L.pick_graph, ch.pick_graph, (size_t)ch.n_picks * sizeof(int32_t));
        std::memcpy(w + L.pick_offset, ch.pick_offset, ((size_t)ch.n_picks + 1) * sizeof(int32_t));
        map_slots(ch.pick_slot, ch.pick_offset[ch.n_picks], w + L.pick_slot);
    }
}

// The block a choice reads back in one copy: the status counters, chosen[n_graphs], cell_cost[n_cells], the picked records.
struct ChoiceLayout {
    size_t chosen = 0, cell_cost = 0, picks = 0, bytes = 0;  // (the counters are at 0)
    explicit ChoiceLayout(const pdmpc_choice& ch) {
        chosen = PDMPC_CHOICE_COUNTERS * sizeof(int32_t);
        cell_cost = (chosen + (size_t)ch.n_graphs * sizeof(int32_t) + 7) & ~(size_t)7;
        picks = cell_cost + (size_t)ch.n_cells * sizeof(double);
        bytes = picks + (size_t)ch.n_picks * sizeof(pdmpc_vehicle_out);
    }
};

// A block the host has read back into the caller's arrays (chosen and cell_cost may be null).  False and the reason in err: a record that is
// no planning result fails the choice as it fails the choice on the host.
inline bool deliver_choice(const pdmpc_choice& ch, const ChoiceLayout& L, const unsigned char* blk, int32_t* chosen, double* cell_cost, pdmpc_vehicle_out* picks, std::string& err) {
    const int32_t* counters = (const int32_t*)blk;
    if (counters[PDMPC_CHOICE_OVERFLOW] || counters[PDMPC_CHOICE_TIMED_OUT] || counters[PDMPC_CHOICE_OTHER]) {
        err = "a result record carries an error status: not a planning result";
        return false;
    }
    if (chosen && ch.n_graphs > 0) std::memcpy(chosen, blk + L.chosen, (size_t)ch.n_graphs * sizeof(int32_t));
    if (cell_cost && ch.n_cells > 0) std::memcpy(cell_cost, blk + L.cell_cost, (size_t)ch.n_cells * sizeof(double));
    if (ch.n_picks > 0) std::memcpy(picks, blk + L.picks, (size_t)ch.n_picks * sizeof(pdmpc_vehicle_out));
    return true;
}

// The choice on the host, of a checked pdmpc_choice on records that are all planning results: cell_cost[n_cells] and chosen[n_graphs] (either may
// be null) from the records' status[n] and final_cost[n].
inline void choose_host(const int32_t* status, const double* final_cost, const pdmpc_choice* ch, int32_t* chosen, double* cell_cost) {
    std::vector<double> sums((size_t)ch->n_cells);
    for (int c = 0; c < ch->n_cells; ++c) {
        double sum = 0.0;
        for (int q = ch->cell_offset[c]; q < ch->cell_offset[c + 1]; ++q) {  // (list order: the order of addition)
            const int s = ch->cell_slot[q];
            sum += status[s] == PDMPC_OK ? final_cost[s] : std::numeric_limits<double>::infinity();
        }
        sums[(size_t)c] = std::nearbyint(sum * 1e8) / 1e8;
    }
    if (chosen)
        for (int g = 0; g < ch->n_graphs; ++g) {
            const double* cand = sums.data() + ch->graph_offset[g];
            const int count = ch->graph_offset[g + 1] - ch->graph_offset[g];
            int best = 0;
            for (int p = 1; p < count; ++p)
                if (cand[p] < cand[best]) best = p;  // [~, i] = min(.): the first minimum
            chosen[g] = best;
        }
    if (cell_cost && ch->n_cells > 0) std::memcpy(cell_cost, sums.data(), sums.size() * sizeof(double));
}
