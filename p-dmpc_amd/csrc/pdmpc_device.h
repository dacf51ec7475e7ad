// pdmpc_device.h — HBM data layout shared by the host packer (pack.cpp) and the search kernel.
//
// Everything the kernel reads is a flat, pointer-free blob so one hipMemcpyAsync moves a whole batch:
//
//   DevVehicle veh[n]      fixed-stride record per vehicle (pose, reference, offsets into the pools)
//   double2    points[]    every literal polygon vertex of the batch, already in the "NaN-separated
//                          soup" order of vectorize_all_obstacles.m:36-62 (step-major per vehicle), so a
//                          workgroup stages its obstacles with one coalesced, fully pipelined copy
//   int32      pred[]      CSR list of predecessor slots (their solved areas are appended on the device)
//
// MPA tables (uploaded once):
//   uint64  succ_mask[Hp][n][n_words]   bit j of word w set <=> transition_matrix_single(i, 64w+j, k) ~= 0
//   int16   man_index[n][n]            index into the maneuver arrays or -1
//   DevManPose man_pose[T]             dx, dy, dyaw, n_cols
//   double2 man_area[T][3][VMAX]       area, area_without_offset, area_large_offset as (x, y) pairs
#ifndef PDMPC_DEVICE_H
#define PDMPC_DEVICE_H

#include <stdint.h>

#include "../../include/pdmpc.h"
#include "../../include/pdmpc_hdv.h"

#define PDMPC_WAVE 64
/* Wavefronts per workgroup follow the kernel's registers: 128 VGPRs or fewer give four wavefronts per SIMD, sixteen per workgroup; up to
 * 168 give three and twelve (`make resources` prints what each kernel needs today). */
#define PDMPC_MAX_WAVES 16     /* wavefronts per workgroup of the InterX search kernels (126 VGPRs: four per SIMD) */
#define PDMPC_MAX_WAVES_SAT 12 /* ... of the separating-axis kernel (150 VGPRs: three per SIMD) */
#define PDMPC_SH_WORDS 128 /* 32-bit LDS words shared by the waves of a workgroup (state, counters of the search) */

struct DevManPose {
    double dx, dy, dyaw;
    int32_t n_cols;
    int32_t pad;
};

struct DevVehicle {
    double x0, y0, yaw0;
    double ref_x[PDMPC_HP_MAX];
    double ref_y[PDMPC_HP_MAX];
    double v_ref[PDMPC_HP_MAX];
    int32_t trim0;                      // 1-based
    int32_t n_pred;                     // predecessors whose solved areas become dynamic obstacles
    int32_t pred_off;                   // into pred[]
    int32_t ll_off, ll_len;             // lanelet soup [left, NaN, right, NaN] in points[]
    int32_t lit_off[PDMPC_HP_MAX + 1];  // literal vehicle-obstacle soup of step k: points[lit_off[k] .. lit_off[k+1])
    int32_t hdv_off[PDMPC_HP_MAX + 1];  // literal HDV soup of step k
    int32_t fb_off[PDMPC_HP_MAX + 1];   // fallback areas (one polygon per step, no separators); fb_off[0] < 0: none
    uint32_t seed;                      // sampled optimizer: RandStream('mt19937ar', Seed = seed) (MonteCarloTreeSearch.m:32)
};

// One search-tree node (Tree.m:3-13 row + what the check of this node's children needs), 64 bytes so a node is four
// 16-byte accesses and the children of an expansion form one contiguous, coalesced store.
struct NodeRec {
    double x, y, yaw, g;  // Tree.x/y/yaw/g
    double cs, sn;        // cos/sin(yaw), filled when the node is checked (expand_node.m:50-51); its children's
                          // edge checks read them (GraphSearch.m:155-156); a goal candidate keeps its path's largest key here
    double h;             // Tree.h
    uint32_t parent;      // Tree.parent (1-based id, 0 for the root)
    uint32_t packed;      // trim (10 bit, 1-based) | k << 10 (5 bit) | maneuver index << 15 (12 bit) | area columns << 27 (4 bit)
};
#define NODE_TRIM(p) ((int)((p) & 1023u))
#define NODE_K(p) ((int)(((p) >> 10) & 31u))
#define NODE_MAN(p) ((int)(((p) >> 15) & 4095u))
#define NODE_COLS(p) ((int)(((p) >> 27) & 15u))

// byte offsets of the regions of the dynamic LDS allocation (all multiples of 16; launch_plan.hpp: layout_bulk / compute_lds_sampled)
struct LdsLayout {
    uint32_t mask, man_index, pose, area;  // MPA tables
    uint32_t ref;                          // ref_x[16], ref_y[16], dtv[16]
    uint32_t shape;                        // sampled optimizer: shape A [8], shape B [8] (double2) + the wave's tally
    uint32_t path;                         // uint32 path[HP_MAX+2], soup / HDV offsets, the shared words, literal soup lengths
    uint32_t soup;                         // double2[soup_cap]
    uint32_t cand;                         // phase B's chunk state (12 B per thread); sampled optimizer: candidate segments of one edge check
    uint32_t vstate;                       // uint8[NV]: validity bytes
    uint32_t expand;                       // d_traveled table: dcum[16][16] doubles (+ the sampled optimizer's expansion scratch)
    uint32_t tree16;                       // sampled optimizer: its tree (children, parent, trim as uint16)
    uint32_t rand;                         // sampled optimizer: its Hp * 250 random numbers (double)
    uint32_t nodes;                        // NodeRec[NL]
    uint32_t total;
    uint32_t bk_near_key, bk_near_id;      // double[BK_PER * threads], uint32[BK_PER * threads]: the LDS part of the open set (the heap of a replay)
    uint32_t bk_ready;                     // uint32[bk_ready_cap] nodes of the round + uint32[bk_ready_cap] their collision flags
    uint32_t bk_hist;                      // uint32[3072]: refill histogram [2048] | goal list [1024], expansion groups [1024], their children's offsets [1024]
    uint32_t bk_misc;                      // 2 KB: path tables of the best goal candidate, scan partials, chunk table, tick counters, the reference's ids along the path | the selection's 256-bin histogram
    uint32_t bk_pshape;                    // double2[Hp][VMAX] + uint32[HP_MAX] + uint64[HP_MAX]: the areas along the path of the record written last and their column counts (what an arrival is checked against first); per step the predecessors whose areas differ from the expected ones
    uint32_t reach_shared;                 // 1: the boundary has ONE reach list for every step, a superset of each step's own (the layout of last resort, launch_plan.hpp: layout_bulk)
    uint32_t bk_reach;                     // the rectangles, counts and root of the reach lists (PDMPC_LK_REACH_*)
    uint32_t reach;                        // uint16[soup columns + (Hp - 1) * boundary columns] at PDMPC_LK_FIXED_END, in front of the MPA tables: per step and soup the segments in
                                           // reach, ascending (a step's vehicle obstacles / HDV sets at the index of that soup's first column, the boundary's list of step k at ll_base + (k - 1) * ll_len)
};

// The `path` region (LdsLayout::path): what the prologue of a search carves it into (search_common.hpp; a helper workgroup likewise)
struct LdsPathRegion {
    uint32_t path[PDMPC_HP_MAX + 2];   // scratch of the epilogue: the nodes of the plan's path; [HP_MAX + 1]: where the lanelet soup begins
    int32_t soff[PDMPC_HP_MAX + 1];    // where each step's vehicle-obstacle soup begins ([Hp]: where the last one ends)
    int32_t hoff[PDMPC_HP_MAX + 1];    // ... each step's HDV soup
    uint32_t shared[PDMPC_SH_WORDS];   // the shared words (lds_layout.hpp)
    int32_t lit[PDMPC_HP_MAX];         // literal soup length per step
};
#define PDMPC_LK_PATH_BYTES PDMPC_LK_ALIGN16((uint32_t)sizeof(LdsPathRegion)) /* (the sampled optimizer reserves the same) */

// The regions of the graph search's layout whose sizes do not depend on the automaton or on the obstacles come first, at offsets that
// are compile-time constants (sized for PDMPC_MAX_WAVES wavefronts and the largest ready list): the kernel addresses them with
// immediates instead of holding two dozen LDS pointers in scalar registers it does not have (layout_bulk fills LdsLayout with the
// same numbers; the automaton's tables, the soup, the validity bytes and the nodes follow at run-time offsets).
#define PDMPC_LK_ALIGN16(x) (((x) + 15u) & ~15u)
// (W = wavefronts the layout is sized for, RC = entries of its ready list.  The product kernels: PDMPC_MAX_WAVES and 2048 — one
// workgroup per CU; bulk_kernel_compact.hip: 8 wavefronts, 512 ready entries and two near entries per thread, which with the automaton's
// areas left in L2 fits 80 KB — TWO workgroups per CU.  A translation unit sets PDMPC_LK_WAVES / PDMPC_LK_READY_CAP / PDMPC_BK_PER
// before it includes this header; the host lays out with pdmpc_lk_fixed().)
#ifndef PDMPC_LK_WAVES
#define PDMPC_LK_WAVES PDMPC_MAX_WAVES
#endif
#ifndef PDMPC_LK_READY_CAP
#define PDMPC_LK_READY_CAP 2048u
#endif
#define PDMPC_LK_COMPACT_WAVES 8
#define PDMPC_LK_COMPACT_READY_CAP 512u
#define PDMPC_LK_COMPACT_BK_PER 2
#define PDMPC_LKX_THREADS(W) ((uint32_t)(W) * PDMPC_WAVE)
#define PDMPC_LKX_REF 0u
#define PDMPC_LKX_SHAPE (PDMPC_LKX_REF + 3u * PDMPC_HP_MAX * 8u)
#define PDMPC_LKX_PATH(W) (PDMPC_LKX_SHAPE + (uint32_t)(W) * (2u * PDMPC_VMAX + 1u) * 16u)
#define PDMPC_LKX_CAND(W) (PDMPC_LKX_PATH(W) + PDMPC_LK_PATH_BYTES)
#define PDMPC_LKX_EXPAND(W) (PDMPC_LKX_CAND(W) + PDMPC_LK_ALIGN16(12u * PDMPC_LKX_THREADS(W)))
#define PDMPC_LKX_NEAR_KEY(W) (PDMPC_LKX_EXPAND(W) + (2u * PDMPC_HP_MAX * PDMPC_HP_MAX) * 8u + 16u * 16u)
#define PDMPC_LKX_NEAR_ID(W, P) (PDMPC_LKX_NEAR_KEY(W) + PDMPC_LK_ALIGN16((uint32_t)(P) * PDMPC_LKX_THREADS(W) * 8u))
#define PDMPC_LKX_READY(W, P) (PDMPC_LKX_NEAR_ID(W, P) + PDMPC_LK_ALIGN16((uint32_t)(P) * PDMPC_LKX_THREADS(W) * 4u))
#define PDMPC_LKX_HIST(W, RC, P) (PDMPC_LKX_READY(W, P) + (uint32_t)(RC) * 8u)
#define PDMPC_LKX_MISC(W, RC, P) (PDMPC_LKX_HIST(W, RC, P) + 3072u * 4u)
#define PDMPC_LKX_PSHAPE(W, RC, P) (PDMPC_LKX_MISC(W, RC, P) + 2048u)
#define PDMPC_LKX_REACH(W, RC, P) (PDMPC_LKX_PSHAPE(W, RC, P) + PDMPC_LK_ALIGN16(PDMPC_HP_MAX * PDMPC_VMAX * 16u + PDMPC_HP_MAX * 4u + PDMPC_HP_MAX * 8u + PDMPC_HP_MAX * 4u))
/* the reach lists' fixed part (include/pdmpc_reach.h): double[HP_MAX][4] the widened rectangle of every step in the root's frame, uint32[3][HP_MAX]
   segments in reach per soup (vehicle obstacles, HDV sets, lanelet boundary) and step, uint32[4]: [0] the vehicle-obstacle lists are older
   than the soup, int32[8] the check items' words, double[8] the root: x, y, cos and sin of its yaw, and the rectangle around all steps' (the boundary's one list, reach_shared) */
#define PDMPC_LK_REACH_CNT (PDMPC_HP_MAX * 4u * 8u)
#define PDMPC_LK_REACH_STALE (PDMPC_LK_REACH_CNT + 3u * PDMPC_HP_MAX * 4u)
#define PDMPC_LK_REACH_SC (PDMPC_LK_REACH_STALE + 16u) /* int32[8]: what a check item would otherwise read from scalar registers: byte offsets of the soup and of the automaton's areas, Hp, ll_base, ll_len, the distance between the boundary's lists of two steps (ll_len, or 0: one list) */
#define PDMPC_LK_REACH_ROOT (PDMPC_LK_REACH_SC + 32u)
#define PDMPC_LKX_FIXED_END(W, RC, P) (PDMPC_LKX_REACH(W, RC, P) + PDMPC_LK_REACH_ROOT + 64u)
#ifndef PDMPC_BK_PER
#define PDMPC_BK_PER 4
#endif
/* entries of the LDS open list per thread (a selection pass holds them in registers) */
#define PDMPC_LK_REF PDMPC_LKX_REF
#define PDMPC_LK_SHAPE PDMPC_LKX_SHAPE
#define PDMPC_LK_PATH PDMPC_LKX_PATH(PDMPC_LK_WAVES)
#define PDMPC_LK_CAND PDMPC_LKX_CAND(PDMPC_LK_WAVES)
#define PDMPC_LK_EXPAND PDMPC_LKX_EXPAND(PDMPC_LK_WAVES)
#define PDMPC_LK_NEAR_KEY PDMPC_LKX_NEAR_KEY(PDMPC_LK_WAVES)
#define PDMPC_LK_NEAR_ID PDMPC_LKX_NEAR_ID(PDMPC_LK_WAVES, PDMPC_BK_PER)
#define PDMPC_LK_READY PDMPC_LKX_READY(PDMPC_LK_WAVES, PDMPC_BK_PER)
#define PDMPC_LK_HIST PDMPC_LKX_HIST(PDMPC_LK_WAVES, PDMPC_LK_READY_CAP, PDMPC_BK_PER)
#define PDMPC_LK_MISC PDMPC_LKX_MISC(PDMPC_LK_WAVES, PDMPC_LK_READY_CAP, PDMPC_BK_PER)
#define PDMPC_LK_PSHAPE PDMPC_LKX_PSHAPE(PDMPC_LK_WAVES, PDMPC_LK_READY_CAP, PDMPC_BK_PER)
#define PDMPC_LK_REACH PDMPC_LKX_REACH(PDMPC_LK_WAVES, PDMPC_LK_READY_CAP, PDMPC_BK_PER)
#define PDMPC_LK_FIXED_END PDMPC_LKX_FIXED_END(PDMPC_LK_WAVES, PDMPC_LK_READY_CAP, PDMPC_BK_PER)

struct NodeArena {  // HBM arrays, per-vehicle stride = max_nodes entries
    NodeRec* nodes;
    double* key;       // open-list key f = g + h of node i (GraphSearch.m:100-102)
    unsigned long long* link;  // parent | packed << 32 per node, eight nodes to a 64-byte line (what walks and phase B read of the tree)
    uint8_t* vstate;   // validity bytes of the nodes beyond the LDS-resident NV (and the read-back copy of those)
    double* far_key;   // open entries outside LDS: keys and nodes of `far`; the heap of a replay beyond its LDS part
    uint32_t* far_id;
    double* mid_key;   // ... and of `mid` (what a heavy search refills near from; far feeds it)
    uint32_t* mid_id;  //     (a replay leaves its pop sequence here)
    double* pb_key;    // phase B: a node's branch maximum
    uint32_t* pb_d;    // phase B: where a node's branch leaves the goal's path; a replay: the node's id in the reference's tree
    double* walk;      // per node, 16 bytes: what its branch to the goal candidate's path looks like (bk_classify_wave)
    uint32_t* child0;  // 1-based arena index of a node's first child (its children are consecutive, ascending trim), 0 while it has none: what the replay of a tied search descends by
    uint32_t* vlist;   // per vehicle Hp + 1 lists of max_nodes entries: the collision-free nodes of steps 1 .. Hp, the parked nodes (what a verification visits)
};

// the fixed part of the graph search's layout for (W wavefronts, ready list of RC entries): what the kernel built with those two
// numbers addresses with immediates; returns the first free byte
static inline uint32_t pdmpc_lk_fixed(uint32_t W, uint32_t RC, uint32_t P, LdsLayout* L) {
    L->ref = PDMPC_LKX_REF;
    L->shape = PDMPC_LKX_SHAPE;
    L->path = PDMPC_LKX_PATH(W);
    L->cand = PDMPC_LKX_CAND(W);
    L->expand = PDMPC_LKX_EXPAND(W);
    L->bk_near_key = PDMPC_LKX_NEAR_KEY(W);
    L->bk_near_id = PDMPC_LKX_NEAR_ID(W, P);
    L->bk_ready = PDMPC_LKX_READY(W, P);
    L->bk_hist = PDMPC_LKX_HIST(W, RC, P);
    L->bk_misc = PDMPC_LKX_MISC(W, RC, P);
    L->bk_pshape = PDMPC_LKX_PSHAPE(W, RC, P);
    L->bk_reach = PDMPC_LKX_REACH(W, RC, P);
    return PDMPC_LKX_FIXED_END(W, RC, P);
}

#define PDMPC_HELP_CAP 2048 /* entries of a round that can be shared (= the ready list's capacity) */
/* a search's board (64-bit words): what its seated helper workgroups read and write (bulk_search.hpp) */
#define PDMPC_HB_SEATS_MAX 64
#define PDMPC_HB_N 1      /* entries of the round that is being shared */
#define PDMPC_HB_MASK 2   /* predecessors whose areas the owner has in its soup */
#define PDMPC_HB_SEATS 3  /* launch id << 32 | seats taken (a helper takes one with a fetch-and-add; the owner resets the word when it starts) */
#define PDMPC_HB_WANT 4   /* == launch id: the search shares its rounds, helpers may take seats; 0 once it has ended */
#define PDMPC_HB_WEIGHT 5 /* nodes the search has processed so far: helpers go where the work per seat is largest */
#define PDMPC_HB_ASSIGN 8 /* [64] per seat: round << 40 | first entry << 20 | entries: the range that seat checks */
#define PDMPC_HB_DONE 72  /* [64] per seat: the last round whose range that seat has finished */
#define PDMPC_HB_WORDS 136
/* The board's words, declared once: owner (bulk_search.hpp) and helper (bk_helper.hpp) pack and read them through these alone.
 * ASSIGN = round << 40 | first entry << 20 | entries: 24 + 20 + 20 bits.  first + entries <= PDMPC_HELP_CAP < 2^20.  The round is the owner's
 * 32-bit help_seq cut to 24 bits; the helper echoes those 24 bits into its DONE word and the owner compares that word with all 32 bits of
 * help_seq, so the 2^24-th shared round of ONE search would find no seat done and end on the watchdog (a search shares at most one round
 * per round, and spin_limit ends it long before).  SEATS = launch id << 32 | seats taken: another launch's word counts as no seat.
 * VERDICT (help_verdict, one 32-bit word per entry) from a check item's flag bits (1 collides, 2 crosses expected areas only): 1
 * collision-free, 2 collides, 3 expected areas only; 0 is "no verdict" and never written. */
#define PDMPC_VALUE_FN constexpr __attribute__((always_inline)) inline /* host and device; always inlined, so that a use compiles to what the literal expression did */
#define PDMPC_HB_ASSIGN_WORD(round, first, count) (((unsigned long long)(round) << 40) | ((unsigned long long)(first) << 20) | (unsigned long long)(count)) /* (a macro at its use in the kernel, like the two below) */
PDMPC_VALUE_FN unsigned long long pdmpc_hb_assign(uint32_t round, uint32_t first, uint32_t count) { return PDMPC_HB_ASSIGN_WORD(round, first, count); }
PDMPC_VALUE_FN uint32_t pdmpc_hb_assign_round(unsigned long long w) { return (uint32_t)(w >> 40); }
PDMPC_VALUE_FN uint32_t pdmpc_hb_assign_first(unsigned long long w) { return (uint32_t)((w >> 20) & 0xfffffull); }
PDMPC_VALUE_FN uint32_t pdmpc_hb_assign_count(unsigned long long w) { return (uint32_t)(w & 0xfffffull); }
PDMPC_VALUE_FN unsigned long long pdmpc_hb_seats(uint32_t launch_id, uint32_t taken) { return ((unsigned long long)launch_id << 32) | (unsigned long long)taken; }
PDMPC_VALUE_FN uint32_t pdmpc_hb_seats_launch(unsigned long long w) { return (uint32_t)(w >> 32); }
PDMPC_VALUE_FN unsigned long long pdmpc_hb_seats_count(unsigned long long w) { return w & 0xffffffffull; }
/* (these are macros at their uses in the kernels and functions for everybody else: behind an inlined call the same expression gave
 * the search kernels other device code at some of its uses) */
#define PDMPC_HB_SEATS_TAKEN(w, launch_id) ((uint32_t)((w) >> 32) == (launch_id) ? (uint32_t)((w) & 0xffffffffull) : 0u) /* the seats taken if the word is this launch's, else 0 */
PDMPC_VALUE_FN uint32_t pdmpc_hb_seats_taken(unsigned long long w, uint32_t launch_id) { return PDMPC_HB_SEATS_TAKEN(w, launch_id); }
PDMPC_VALUE_FN uint32_t pdmpc_hb_verdict(uint32_t flags) { return (flags & 1u) ? 2u : ((flags & 2u) ? 3u : 1u); }
PDMPC_VALUE_FN bool pdmpc_hb_verdict_missing(uint32_t v) { return v < 1u || v > 3u; }
PDMPC_VALUE_FN uint32_t pdmpc_hb_verdict_flags(uint32_t v) { return v == 2u ? 1u : (v == 3u ? 2u : 0u); }
/* bit p = the p-th predecessor: all n_pred of them (a search with more than 64 waits for them all and keeps no such set) */
#define PDMPC_ALL_PREDECESSORS(n_pred) ((n_pred) >= 64 ? ~0ull : ((1ull << (n_pred)) - 1ull))
PDMPC_VALUE_FN unsigned long long pdmpc_all_predecessors(int n_pred) { return PDMPC_ALL_PREDECESSORS(n_pred); }
PDMPC_VALUE_FN bool pdmpc_hb_assign_round_trips(uint32_t round, uint32_t first, uint32_t count) {
    return pdmpc_hb_assign_round(pdmpc_hb_assign(round, first, count)) == round && pdmpc_hb_assign_first(pdmpc_hb_assign(round, first, count)) == first &&
           pdmpc_hb_assign_count(pdmpc_hb_assign(round, first, count)) == count;
}
static_assert(PDMPC_HELP_CAP < (1 << 20), "a first entry and an entry count each fit their 20 bits of the assignment word");
static_assert(pdmpc_hb_assign_round_trips(0u, 0u, 0u) && pdmpc_hb_assign_round_trips(1u, 1u, 1u) && pdmpc_hb_assign_round_trips(1u, PDMPC_HELP_CAP, PDMPC_HELP_CAP) &&
                  pdmpc_hb_assign_round_trips((1u << 24) - 1u, (1u << 20) - 1u, (1u << 20) - 1u) && pdmpc_hb_assign_round_trips((1u << 24) - 1u, 0u, 0u) &&
                  pdmpc_hb_assign_round_trips(0u, (1u << 20) - 1u, 0u) && pdmpc_hb_assign_round_trips(0u, 0u, (1u << 20) - 1u),
              "the fields of the assignment word do not overlap");
static_assert(pdmpc_hb_assign_round(pdmpc_hb_assign(1u << 24, 0u, 0u)) == 0u, "the round is cut to 24 bits");
static_assert(pdmpc_hb_seats_taken(pdmpc_hb_seats(7u, 0u), 7u) == 0u && pdmpc_hb_seats_taken(pdmpc_hb_seats(7u, 0u) + 3ull, 7u) == 3u && pdmpc_hb_seats_taken(pdmpc_hb_seats(7u, 5u), 8u) == 0u &&
                  pdmpc_hb_seats_taken(pdmpc_hb_seats(0xffffffffu, PDMPC_HB_SEATS_MAX), 0xffffffffu) == PDMPC_HB_SEATS_MAX,
              "a seat is counted for its own launch only");
static_assert(pdmpc_hb_verdict(0u) == 1u && pdmpc_hb_verdict(1u) == 2u && pdmpc_hb_verdict(2u) == 3u && pdmpc_hb_verdict(3u) == 2u, "a crossing of a real area decides");
static_assert(pdmpc_hb_verdict_flags(1u) == 0u && pdmpc_hb_verdict_flags(2u) == 1u && pdmpc_hb_verdict_flags(3u) == 2u && pdmpc_hb_verdict_missing(0u) && pdmpc_hb_verdict_missing(4u) &&
                  !pdmpc_hb_verdict_missing(1u) && !pdmpc_hb_verdict_missing(3u),
              "the owner reads a verdict back as the flag bits P2 expects");
static_assert(pdmpc_all_predecessors(0) == 0ull && pdmpc_all_predecessors(1) == 1ull && pdmpc_all_predecessors(63) == 0x7fffffffffffffffull && pdmpc_all_predecessors(64) == ~0ull &&
                  pdmpc_all_predecessors(65) == ~0ull,
              "one bit per predecessor, all 64 from 64 on");

struct KernelArgs {
    // MPA
    const uint64_t* succ_mask;
    const int16_t* man_index;
    const DevManPose* man_pose;
    const double* man_area;  // double2 pairs
    int32_t n_trims, n_words, n_man, Hp;
    int32_t checker;
    int32_t areas_in_lds;
    double dt;
    // batch
    const DevVehicle* veh;
    const double* points;  // double2 pairs
    const int32_t* pred;
    pdmpc_vehicle_out* out;
    uint32_t* done_flag;
    uint32_t epoch;
    int32_t first;  // slot of blockIdx.x == 0
    // arenas
    NodeArena arena;
    uint32_t max_nodes;
    int32_t* tree_size;  // per slot: nodes in the arena after the search | PDMPC_TREE_FRONTIER (| PDMPC_TREE_REPLAYED) (debug read-back)
#define PDMPC_TREE_FRONTIER 0x40000000  /* d_tree_size marker: the arena holds the frontier kernel's raw tree (creation order differs from the reference's) */
#define PDMPC_TREE_REPLAYED 0x20000000  /* ... and the search ended on the replay through the binary heap (equal keys): its pop sequence, in arena indices, is in the mid list's array */
#define PDMPC_TREE_SIZE(sz) ((sz) & ~(PDMPC_TREE_FRONTIER | PDMPC_TREE_REPLAYED))
    // LDS
    LdsLayout lds;
    int32_t NL, NV, soup_cap, cand_cap;
    int32_t n_waves;                   // wavefronts per workgroup of this launch (workgroup size / 64)
    unsigned long long* work_count;    // [0] edge checks evaluated, [1] segment pairs they stand for, [2] nodes processed, [3] rounds, [4] shared rounds, [5] nodes checked by helpers, [6] plans that are not planning results (cumulative, all vehicles)
    int32_t* tie_count;                // [0] searches that ended on the binary heap (equal keys), [2] arrival events (cumulative)
    uint32_t* progress;    // host-mapped (pinned) words, 64 per slot: live counters, for debugging a launch that does not end (or null)
    int32_t debug_tail;    // 1: the search leaves its round / node / tick counters in the unused last rows of pdmpc_vehicle_out.path_nodes
    // helper workgroups (blockIdx >= n_searches): CUs the launch leaves idle check tiles of other workgroups' large rounds
    int32_t n_searches;              // workgroups of this launch that run a search (the first ones)
    int32_t n_helpers;               // helper workgroups behind them (0: none)
    unsigned long long* help_board;  // [slot][PDMPC_HB_WORDS]: see above
    uint32_t* help_verdict;          // [slot][PDMPC_HELP_CAP] 1 collision-free, 2 colliding, 3 crosses expected areas only (written by helpers)
    uint32_t* help_finished;         // searches that have published their result (runs on from launch to launch) ...
    uint32_t help_fin_base;          // ... and its value when this launch went out
    uint32_t launch_id;              // number of this launch on its handle (never 0): tells this launch's board words from an earlier launch's
    int32_t bk_ready_cap;   // entries of the ready list (a round's nodes)
    int32_t bk_round0;      // nodes a round of a young search takes
    int32_t bk_round;       // ... and the most any round takes
    int32_t bk_ramp;        // a round of a search that is no longer young grows by 1 / bk_ramp of the nodes processed so far
    int32_t bk_helpers_first;  // helper workgroups dispatched in front of the searches (the others follow them)
    int32_t bk_seat_nodes;     // a search is entitled to its share of the launch's helpers per this many nodes processed (bulk_helper_body)
    int32_t bk_tentative;   // 1: predecessors that are still planning have their expected areas (the ones they publish when exhausted) in their soup slots
    int32_t bk_tile;        // the most entries of a shared round one seat takes (what a helper stages in LDS; at most 768)
    int32_t bk_mid_min;     // a far list longer than this is not scanned by every refill of near: a band of its smallest keys is moved to mid first
    int32_t bk_mid_fill;    // ... about this many entries at a time
    int32_t bk_share_min;   // a round with at least this many entries is shared with the helper workgroups
    int32_t bk_force_tie;    // testing only: every search is treated as if it had met equal keys, i.e. ends on the replay of its tree through the reference's binary heap
    int32_t bk_fast_arrival; // 1: a finished search checks an arriving predecessor's areas against its plan's path first and publishes its own areas as soon as the last one has passed (the other collision-free nodes are verified afterwards)
    double* bk_post;        // [slot][bk_ready_cap][3] double2: what a check item reads of the tree, posted per entry of a shared round
    int32_t speculate;  // 1: start searching before all predecessors have finished (results are identical)
    uint32_t spin_limit;
    int32_t reverse_dispatch;  // testing only: workgroup b plans slot first + n_searches - 1 - b, i.e. successors are
                               // dispatched before their predecessors -- the adversarial order the watchdog + resident slices must survive
};

// Every search kernel is built twice from one body (bulk_search.hpp).  The PRODUCT instantiation (pdmpc_bulk_kernel, _wide, _sat,
// _compact) has the debug and test switches below compiled in at these values -- the defaults of Tuning --;
// the maneuver areas are where the product's launches of that kernel have them: in LDS for the one-mask-word InterX kernel and
// the separating-axis kernel, in L2 for the compact kernel (its layout leaves them there) and for the wide kernel (the only automaton
// of more than 64 trims, the realistic one, has 527 maneuvers: their areas never fit; a wide automaton small enough to keep its areas
// in LDS would always run pdmpc_bulk_kernel_wide_any).  KernelArgs::progress is read by no search kernel and selects nothing.  A uniform value that is a constant costs the
// round loop no scalar register.  The GENERIC instantiation (the same names + _any) reads all of them from
// KernelArgs.  launch_plan.hpp: bulk_generic plans the product instantiation exactly when matches() holds.
enum { PDMPC_BULK = 0, PDMPC_BULK_WIDE = 1, PDMPC_BULK_SAT = 2, PDMPC_BULK_COMPACT = 3 };  // the four search kernels
struct ProductSwitches {
    static constexpr int32_t debug_tail = 0, bk_force_tie = 0, reverse_dispatch = 0, bk_tentative = 1, bk_fast_arrival = 1, speculate = 1;
    static constexpr int32_t areas_in_lds(int kernel) { return kernel == PDMPC_BULK || kernel == PDMPC_BULK_SAT ? 1 : 0; }
    static bool matches(const KernelArgs& a, int kernel) {
        return a.debug_tail == debug_tail && a.bk_force_tie == bk_force_tie && a.reverse_dispatch == reverse_dispatch && a.bk_tentative == bk_tentative &&
               a.bk_fast_arrival == bk_fast_arrival && a.speculate == speculate && a.areas_in_lds == areas_in_lds(kernel);
    }
};

// The joint search of centralized control (joint_kernel.hip): one workgroup per problem, problem p = packed slots
// [problem_off[p], problem_off[p + 1]).  Joint node i of a problem is the N records nodes[(first slot + v) * max_nodes + i], v < N:
// vehicle v's pose and trim, k, parent, and the node's joint g and h in every one of them.  The open list keeps its first heap_lds
// entries in LDS and the rest in far_key / far_id of the problem's first slot.
struct JointLds {  // byte offsets into the dynamic LDS allocation (launch_plan.hpp: layout_joint)
    uint32_t mask, man_index, pose, area;  // MPA tables (area: only if areas_in_lds)
    uint32_t ref;                          // double [PDMPC_JOINT_MAX][3][PDMPC_HP_MAX]: ref_x, ref_y, v_ref per vehicle
    uint32_t shape;                        // double2 [PDMPC_JOINT_MAX][2][PDMPC_VMAX]: area, boundary-check area of the node's edge
    uint32_t ints;                         // int32: soup offsets [JOINT_MAX][HP_MAX + 1], boundary base / length / columns [3][JOINT_MAX], path [HP_MAX + 1]
    uint32_t succ;                         // int32 [PDMPC_JOINT_MAX][n_trims]: successor trims of the node being expanded
    uint32_t soup;                         // double2 [soup_cap]: the problem's obstacle soups and boundaries, vehicle after vehicle, every distinct one once
    uint32_t heap_key, heap_id;            // the LDS part of the open list: double [heap_lds], uint32 [heap_lds]
    uint32_t total;
};
#define PDMPC_JOINT_INTS (PDMPC_JOINT_MAX * (PDMPC_HP_MAX + 1) + 3 * PDMPC_JOINT_MAX + PDMPC_HP_MAX + 1)

// ONE LDS copy per distinct soup of a joint problem.  Vehicle v of a problem (veh: its first packed slot) takes over the LDS soup of
// the first earlier vehicle u < v whose per-step pool offsets lit_off[0 .. Hp] equal its own -- the packer gives vehicles that hand
// over the same obstacle arrays the same offsets (pack.cpp) --, and its boundary of the first earlier vehicle with the same ll_off and
// ll_len.  -1: v brings its own.  The rule of the kernel's prologue (what is staged) AND of layout_joint's soup_cap (what is
// budgeted), which is why it is written here once.
#ifdef __HIP__
#define PDMPC_HOST_DEVICE __attribute__((host)) __attribute__((device))
#else
#define PDMPC_HOST_DEVICE
#endif
PDMPC_HOST_DEVICE static inline int pdmpc_joint_soup_owner(const DevVehicle* veh, int v, int Hp) {
    for (int u = 0; u < v; ++u) {
        bool same = true;
        for (int k = 0; k <= Hp && same; ++k) same = veh[u].lit_off[k] == veh[v].lit_off[k];
        if (same) return u;
    }
    return -1;
}
PDMPC_HOST_DEVICE static inline int pdmpc_joint_boundary_owner(const DevVehicle* veh, int v) {
    for (int u = 0; u < v; ++u)
        if (veh[u].ll_off == veh[v].ll_off && veh[u].ll_len == veh[v].ll_len) return u;
    return -1;
}
// the soup columns a joint problem of N vehicles stages (the sum the prologue's `off` ends at)
PDMPC_HOST_DEVICE static inline int pdmpc_joint_soup_columns(const DevVehicle* veh, int N, int Hp) {
    int need = 0;
    for (int v = 0; v < N; ++v) {
        if (pdmpc_joint_soup_owner(veh, v, Hp) < 0) need += veh[v].lit_off[Hp] - veh[v].lit_off[0];
        if (pdmpc_joint_boundary_owner(veh, v) < 0) need += veh[v].ll_len;
    }
    return need;
}

struct JointArgs {
    const uint64_t* succ_mask;
    const int16_t* man_index;
    const DevManPose* man_pose;
    const double* man_area;  // double2 pairs
    int32_t n_trims, n_words, n_man, Hp;
    int32_t areas_in_lds;
    double dt;
    const DevVehicle* veh;
    const double* points;      // double2 pairs
    const int32_t* problem_off;  // [n_problems + 1]
    pdmpc_vehicle_out* out;      // per slot
    NodeRec* nodes;              // per slot: max_nodes records
    double* far_key;             // per slot: max_nodes entries (a problem uses its first slot's)
    uint32_t* far_id;
    uint32_t max_nodes;
    uint32_t heap_lds;
    int32_t* tree_size;          // per slot: nodes in the problem's tree after the search
    unsigned long long* work_count;  // [0] edge checks (one per popped node that has a parent), [2] nodes popped
    JointLds lds;
};

// The unique prioritizations of a coupling graph (priority_kernel.hip; Prioritizer.unique_priorities, Prioritizer.m:97-140): edge e
// (0-based, find(triu(adjacency, 1)) order: by column, then by row) runs edge_row -> edge_col unless orientation m flips it, which it
// does exactly when bit E - 1 - e of m is set (dec2bin(m, E): edge 1 is the most significant bit).  So the flip set of lane m IS m.
#define PDMPC_PRIO_MAX_N 64
#define PDMPC_PRIO_MAX_E 32
#define PDMPC_PRIO_THREADS 256  // a workgroup: four wavefronts
#define PDMPC_PRIO_ROUNDS 16    // a tile: this many rounds of PDMPC_PRIO_THREADS consecutive masks
#define PDMPC_PRIO_TILE (PDMPC_PRIO_THREADS * PDMPC_PRIO_ROUNDS)
struct PriorityArgs {                          // passed by value: the kernels read it from the kernel arguments (uniform, scalar loads)
    uint32_t in_base[PDMPC_PRIO_MAX_N];        // per vertex: the edges (as bits of m) that point INTO it when not flipped
    uint32_t out_base[PDMPC_PRIO_MAX_N];       // ... that point OUT of it when not flipped (flipped, they point into it)
    int32_t active[PDMPC_PRIO_MAX_N];          // the vertices that have edges, ascending
    int32_t n, E, n_active;
    uint32_t all_edges;                        // the E low bits
    uint64_t n_masks;                          // 2^E
};
// The grouped call (pdmpc_unique_priorities_grouped): one PriorityArgs per graph and the prefix tables, in the handle's memory.  A launch
// holds fewer than 2^32 threads, so the tiles of all graphs of a call are fewer than 2^24.
#define PDMPC_PRIO_MAX_TILES (((int64_t)1 << 24) - 1)
struct PriorityGroups {
    int32_t n_groups;
    const PriorityArgs* graph;    // [n_groups]
    const int64_t* tile_first;    // [n_groups + 1] prefix sums of the graphs' tile counts ceil(2^E_g / PDMPC_PRIO_TILE)
    int64_t* mask_first;          // [n_groups + 1] where graph g's masks start in the concatenated list (the offsets pass writes it)
    const int64_t* row_first;     // [n_groups] where graph g's rows start in priorities: sum over g' < g of K_g' n_g'
};

// The reachable-set coupler (reachable_kernel.hip; ReachableSetCoupler.m:5-56): every vehicle's step-Hp hull moved to its pose,
// then the pairs i < j.  All arrays are the handle's, sized at pdmpc_upload_reachable_sets.
#define PDMPC_REACH_MAX_COLS 256  // vertices of one local hull (pdmpc_upload_reachable_sets returns PDMPC_ERR_CAPACITY above)
#define PDMPC_REACH_WAVE 64       // a workgroup of pass 2 is one wavefront
struct ReachArgs {
    int32_t n, max_cols;
    const double* local_x;        // the local step-Hp hulls of the trims, clockwise, open: trim t = columns local_off[t] .. local_off[t + 1] - 1
    const double* local_y;
    const int32_t* local_off;     // [n_trims + 1]
    const double* in;             // [4 n]: x, y, cos(yaw), sin(yaw) of every vehicle (host libm)
    const int32_t* trim;          // [n] 0-based, checked on the host
    double* hull_x;               // [n * max_cols] the moved hulls
    double* hull_y;
    int32_t* hull_n;              // [n]
    double* box;                  // [4 n] x0, x1, y0, y1
    uint8_t* adjacency;           // [n * n]
    double* area;                 // [n * n] overlap area of every pair that passed the box test, 0 elsewhere
    const int32_t* group;         // the grouped call only (PairGroup per vehicle): adjacency / area then hold one block per group
    int32_t max_group;            // ... and its largest group
};

// Grouped couplers (pdmpc_*_coupling_grouped): the vehicles handed over are consecutive groups, pairs are formed inside a group only, and
// group g's n_g x n_g results stand row-major at element offset sum_{h<g} n_h^2 of adjacency / area.  Per vehicle, staged by the host:
struct PairGroup {
    int32_t first, end, block;    // the vehicle's group is vehicles first .. end - 1; its block's element offset
};

// Lanelet bounding and the coupler on the bounded sets (bounded_kernel.hip; include/pdmpc_geometry.h).  Set o = v * S + q holds vehicle v's
// step (all_steps ? q + 1 : Hp) set in slot o of set_x / set_y (stride PDMPC_BOUND_SLOT), closed; every array is the handle's.
#define PDMPC_BOUND_SLOT 1024       // = PDMPC_BOUNDED_MAX_COLS
#define PDMPC_BOUND_LANELET_MAX 512 // = PDMPC_LANELET_POLY_MAX_COLS
#define PDMPC_BOUND_OVERFLOW 0x80   // set_flags: the set did not fit its slot
#define PDMPC_BOUND_PAIR_BLOCKS 2048 // workgroups of the pair pass (grid-stride over the survivors of the box test)
struct BoundArgs {
    int32_t n, S, Hp, all_steps;
    const double* local_x;     // every trim's local hulls of every step, polygon trim * Hp + k, x then y
    const double* local_y;
    const int32_t* local_off;  // [n_trims * Hp + 1]
    const double* in;          // [4 n]: x, y, cos(yaw), sin(yaw)
    const int32_t* trim;       // [n] 0-based, checked on the host
    const int32_t* lan_off;    // [n + 1] the normalized lanelet polygons (0 vertices: not bounded)
    const double* lan_x;
    const double* lan_y;
    double* set_x;             // [n S PDMPC_BOUND_SLOT]
    double* set_y;
    int32_t* set_n;            // [n S] vertices (closing one included)
    uint8_t* set_flags;        // [n S] PDMPC_BOUND_* | PDMPC_BOUND_OVERFLOW
    double* box;               // [4 n] x0, x1, y0, y1 of the step-Hp sets
    uint8_t* adjacency;        // [n n]
    double* area;              // [n n]
    int32_t* pairs;            // [n (n - 1) / 2] i * n + j of the pairs that pass the box test
    int32_t* n_pairs;          // [1] their count (cleared before the box pass)
    const int32_t* group;      // the grouped call only (PairGroup per vehicle)
    int32_t max_group;         // ... and its largest group
};

// Future collision assessment (fca_kernel.hip; FcaPrioritizer.m:11-92): the footprints of every (vehicle, step), then
// one lane per work item — (pair, step), (vehicle < n - 1, step, static obstacle), (vehicle < n - 1, step, dynamic row), in this order
// of the flat item index — with integer atomics into the counts.  All arrays are the handle's (api.cpp: pdmpc_fca_collisions).
#define PDMPC_FCA_BLOCK 256         // lanes per workgroup of both passes
#define PDMPC_FCA_MAX_BLOCKS 4096   // workgroups of the item pass at most (grid-stride beyond)
struct FcaArgs {
    int32_t n, Hp, n_pairs, n_static, n_rows;
    double length, width, offset;
    int64_t n_pair_items, n_static_items, n_items;  // n_pairs Hp, (n - 1) Hp n_static, and the total with (n - 1) Hp n_rows
    const double* in;           // [4 n Hp]: x, y, cos(yaw), sin(yaw) of every reference point (point k of vehicle v at v Hp + k)
    const int32_t* pairs;       // [2 n_pairs] a < b, checked on the host
    const int32_t* static_off;  // [n_static + 1]
    const double* static_x;
    const double* static_y;
    const int32_t* dyn_off;     // [n_rows Hp + 1]: row r at step k is polygon r Hp + k
    const double* dyn_x;
    const double* dyn_y;
    double* fp;                 // [8 n Hp] footprint of (v, k) at 8 (v Hp + k): the x of its 4 corners, then their y
    int32_t* counts;            // [n]
};

// The grouped form (pdmpc_fca_collisions_grouped): the n vehicles of `a` are n_groups consecutive groups, each with its
// own sizes, static obstacles and dynamic rows.  a.pairs are rebased to the concatenated vehicles; a.static_off / a.dyn_off and the
// vertices behind them hold the groups' polygons one group after the other; a.n_static_items / a.n_items are the sums over the groups
// (a.n_static, a.n_rows, a.length, a.width, a.offset are not read).  Per group, staged by the host:
struct FcaGroup {
    int32_t first;                        // its first vehicle
    int32_t n_static, n_rows;             // S_g static polygons, R_g rows of Hp polygons
    int32_t static_polygon, dyn_polygon;  // its first polygon in a.static_off / a.dyn_off
    double length, width, offset;
};
struct FcaGroups {
    int32_t n_groups;
    const FcaGroup* group;         // [n_groups]
    const int32_t* vehicle_group;  // [n] every vehicle's group
    const int64_t* static_first;   // [n_groups + 1] prefix sums of (n_g - 1) Hp S_g: where group g's static items start in the static range
    const int64_t* dyn_first;      // [n_groups + 1] ... of (n_g - 1) Hp R_g, in the dynamic range (groups of no vehicle count 0 items)
};
struct FcaGroupedArgs {
    FcaArgs a;
    FcaGroups g;
};

// HDV traffic (hdv_kernel.hip; include/pdmpc_hdv.h): the closest lanelets and chains of every HDV, the reachable lane
// of every (HDV, chain, step) and the CAV/HDV adjacency, in four launches of one call.  A (HDV h, chain c, step k) works in slot
// (h PDMPC_HDV_MAX_CHAINS + c) Hp + k; the pack pass moves the slots of the chains that exist into the caller's layout: rows =
// (HDV, chain) in order, polygon row Hp + k, vertices one polygon behind the other, nothing written at or beyond `capacity`.
#define PDMPC_HDV_WAVE 64             // a workgroup of every pass is one wavefront
#define PDMPC_HDV_OVER_LISTS 1        // status: an HDV has more than PDMPC_HDV_MAX_CHAINS closest lanelets or chains
#define PDMPC_HDV_OVER_SLOT 2         // status: a reachable lane did not fit its slot
struct HdvArgs {
    pdmpc_hdv_map map;          // the uploaded map (device arrays)
    int32_t n_hdv, n_cav, Hp, capacity;
    const double* local_x;      // the HDV automaton's local hulls, polygon trim * Hp + k, x then y
    const double* local_y;
    const int32_t* local_off;   // [n_trims Hp + 1]
    const double* in;           // [6 n_hdv]: x, y, cos(yaw), sin(yaw), tile_dx, tile_dy, one array after the other
    const int32_t* trim;        // [n_hdv] 0-based
    const double* cav;          // [4 n_cav]: x, y, tile_dx, tile_dy
    const int32_t* cav_lanelet; // [n_cav] 1-based
    int32_t* n_closest;         // [n_hdv] length of the list (the first PDMPC_HDV_MAX_CHAINS ids are kept)
    int32_t* closest;           // [n_hdv PDMPC_HDV_MAX_CHAINS]
    int32_t* n_chains;          // [n_hdv]
    int32_t* chain_id;          // [n_hdv PDMPC_HDV_MAX_CHAINS]
    int32_t* chain_succ;
    double* slot_x;             // [slots PDMPC_BOUND_SLOT]
    double* slot_y;
    int32_t* slot_n;            // [slots] vertices (closing one included; 0: empty)
    uint8_t* slot_flags;        // [slots] PDMPC_BOUND_* | PDMPC_BOUND_OVERFLOW
    int32_t* status;            // [2]: rows, PDMPC_HDV_OVER_*
    int32_t* row_hdv;           // [n_hdv PDMPC_HDV_MAX_CHAINS]
    int32_t* set_off;           // [slots + 1]
    uint8_t* set_flags;         // [slots]
    double* set_x;              // [capacity]
    double* set_y;
    uint8_t* adjacency;         // [n_cav n_hdv]
};
// ... of several independent groups in one call (pdmpc_hdv_traffic_grouped; five launches).  The work arrays are HdvArgs' over the HDVs
// and CAVs of all groups, group after group (a: n_hdv / n_cav the totals, map and local_* unused); an item finds its group through
// group_of (an HDV's) or pair_first (a (CAV, HDV) pair's, searched) and its map in the handle's table of one record per map slot,
// written at the upload.  The outputs keep the blocks of pdmpc_hdv_grouped_layout_host: group g's rows, offsets and HDV indices are
// its own (from 0), its vertices start at set_base[g].
#define PDMPC_HDV_SCAN_BLOCK 256      // lanes of the scan pass's one workgroup = slots of one of its tiles
struct HdvMapRecord {
    pdmpc_hdv_map map;
    const double *local_x, *local_y;
    const int32_t* local_off;
};
struct HdvGroup {
    int32_t slot, h0, n_hdv, c0, n_cav;  // map slot; first HDV / CAV and their numbers
};
struct HdvGroupedArgs {
    HdvArgs a;
    const HdvMapRecord* maps;   // [PDMPC_HDV_MAP_SLOTS]
    const HdvGroup* groups;     // [n_groups]
    const int32_t* group_of;    // [n_hdv]
    const int32_t* pair_first;  // [n_groups + 1] first (CAV, HDV) pair of every group; the last entry: all pairs
    int32_t n_groups, n_pairs;  // n_pairs: the host's copy of pair_first[n_groups]
    int32_t* slot_before;       // [slots] vertices of the group's slots in front (slots that exist)
    int32_t* row_base;          // [n_hdv] rows of the group's HDVs in front
    int32_t* n_rows;            // [n_groups] -1: an HDV of the group ran over its lists (the group writes nothing else)
    int32_t* set_base;          // [n_groups + 1]
};
// The drive pass in front of them (pdmpc_hdv_drive_kernel; include/pdmpc_hdv.h: the driver model): one wavefront per HDV of the call moves
// it one step along its route.  It reads the old states and the CAVs, and writes the new state, speed and gap and -- where the passes
// behind it read them -- the new pose into `in`.  The HDVs of a group that does not drive (drives[g] == 0) keep the poses staged in `in`.
#define PDMPC_HDV_DRIVE_PARAMS 5      // per group: look_ahead, gap_min, headway, lateral, dt
struct HdvDriveArgs {
    const HdvMapRecord* maps;   // [PDMPC_HDV_MAP_SLOTS]
    const HdvGroup* groups;     // [n_groups]
    const int32_t* group_of;    // [n_hdv]
    const uint8_t* drives;      // [n_groups]
    int32_t n_hdv, n_cav;       // of all groups
    const int32_t* route_off;   // [n_hdv + 1]
    const int32_t* route_id;    // 1-based lanelet ids, route after route
    const uint8_t* closed;      // [n_hdv]
    const int32_t* state_seg;   // [2 n_hdv]: r of every HDV, then j
    const double* state_u;      // [n_hdv]
    const double* v_des;        // [n_hdv]
    const double* params;       // [PDMPC_HDV_DRIVE_PARAMS n_groups]
    const double* cav;          // HdvArgs::cav
    double* in;                 // HdvArgs::in: tile_dx / tile_dy are read, x, y, cos(yaw), sin(yaw) written
    int32_t* new_seg;           // [2 n_hdv]
    double *new_u, *speed, *gap;  // [n_hdv] each
    double* pose;               // [4 n_hdv]: the new x, y, cos(yaw), sin(yaw) once more, where the call reads them back
};
struct HdvDriveTrafficArgs {
    HdvDriveArgs d;
    HdvGroupedArgs g;
};

// The choice among the plans of a batch (choice_kernel.hip; pdmpc_choice in include/pdmpc.h) on the result records
// where the search left them.  The lists are the caller's with the slots mapped to record slots and checked on the host (api.cpp:
// stage_choice); cells of no graph are the cells in front of first_graph_cell and from end_graph_cell on.
#define PDMPC_CHOICE_GATHER_BLOCK 256  // lanes of the workgroup that copies one picked record
enum { PDMPC_CHOICE_OVERFLOW = 0, PDMPC_CHOICE_TIMED_OUT = 1, PDMPC_CHOICE_OTHER = 2, PDMPC_CHOICE_COUNTERS = 4 };
struct ChoiceArgs {
    const pdmpc_vehicle_out* rec;  // the result records (the handle's d_out)
    int32_t n, Hp;                 // records of the batch, the row of path_nodes whose g is the plan's cost
    int32_t n_cells, n_graphs, n_picks;
    int32_t first_graph_cell, end_graph_cell;
    const int32_t* cell_offset;    // [n_cells + 1]
    const int32_t* cell_slot;
    const int32_t* graph_offset;   // [n_graphs + 1]
    const int32_t* pick_graph;     // [n_picks]
    const int32_t* pick_offset;    // [n_picks + 1]
    const int32_t* pick_slot;
    int32_t* tally;                // [PDMPC_CHOICE_COUNTERS] records per non-planning status, counted by the first pass; zero between calls
    int32_t* counters;             // [PDMPC_CHOICE_COUNTERS] ... as the call reads them back (the second pass moves them here and clears the tally)
    int32_t* chosen;               // [n_graphs]
    double* cell_cost;             // [n_cells]
    pdmpc_vehicle_out* picks;      // [n_picks]
};

#ifdef __cplusplus
extern "C" {
#endif
// choice_kernel.hip: the sums, status counters and first minima in one launch, the gather of the picked records in a second
int pdmpc_launch_choice(const ChoiceArgs* args, void* stream);
// fca_kernel.hip: the footprint pass (which also clears the counts) and the item pass on the handle's stream
int pdmpc_launch_fca(const FcaArgs* args, void* stream);
int pdmpc_launch_fca_grouped(const FcaGroupedArgs* args, void* stream);
// fca.cpp: the argument checks pdmpc_fca_collisions and its host twin share (PDMPC_OK, or an error code with *why set), and the
// stable descending sort of the counts (priorities = 1-based index vector)
int pdmpc_fca_check_args(int32_t n, int32_t Hp, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, int32_t n_pairs,
                         const int32_t* pairs, const pdmpc_polygon_set* obstacles, const pdmpc_polygon_set* dynamic_rows, const int32_t* collisions,
                         const int32_t* priorities, const char** why);
void pdmpc_fca_sort_index(int32_t n, const int32_t* collisions, int32_t* priorities);
// ... and of the grouped calls: n_groups, Hp, the arrays and every group with vehicles (pdmpc_fca_check_args on its slices); *n_total =
// the vehicles of all groups, `why` (why_size bytes) names the group that was refused
int pdmpc_fca_check_groups(int32_t n_groups, const pdmpc_fca_group* groups, int32_t Hp, const double* x, const double* y, const double* cos_yaw,
                           const double* sin_yaw, const int32_t* collisions, const int32_t* priorities, int32_t* n_total, char* why, int32_t why_size);
// hdv_kernel.hip: closest lanelets and chains, reachable lanes, packing and adjacency on the handle's stream (n_hdv > 0)
int pdmpc_launch_hdv_traffic(const HdvArgs* args, void* stream);
// ... of the groups of a grouped call: closest, lane, scan, copy and adjacency pass (a.n_hdv > 0)
int pdmpc_launch_hdv_traffic_grouped(const HdvGroupedArgs* args, void* stream);
// ... the drive pass alone (n_hdv > 0), and in front of the five passes of the grouped call: six launches
int pdmpc_launch_hdv_drive(const HdvDriveArgs* args, void* stream);
int pdmpc_launch_hdv_drive_traffic_grouped(const HdvDriveTrafficArgs* args, void* stream);
// reachable_kernel.hip: the two passes of the reachable-set coupler on the handle's stream
int pdmpc_launch_reachable_coupling(const ReachArgs* args, void* stream);
int pdmpc_launch_reachable_coupling_grouped(const ReachArgs* args, void* stream);
// bounded_kernel.hip: the bounding pass (one wavefront per set) and the two passes of the coupler on the step-Hp sets
int pdmpc_launch_bound_sets(const BoundArgs* args, void* stream);
int pdmpc_launch_bounded_coupling(const BoundArgs* args, void* stream);
int pdmpc_launch_bounded_coupling_grouped(const BoundArgs* args, void* stream);
// bulk_kernel*.hip: the graph search as bulk-synchronous passes (count searches + args->n_helpers helper workgroups in ONE launch) for the
// InterX checker with one successor-mask word / with any number of them, and for the separating-axis checker; lds_high_water = the
// handle's record of the dynamic LDS size set so far on that kernel.  Each launches the product instantiation, its _any twin the generic
// one (ProductSwitches); every instantiation has a high-water mark of its own.
int pdmpc_launch_bulk(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
int pdmpc_launch_bulk_any(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
int pdmpc_launch_bulk_wide(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
int pdmpc_launch_bulk_wide_any(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
int pdmpc_launch_bulk_sat(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
int pdmpc_launch_bulk_sat_any(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
// bulk_kernel_compact.hip: the InterX / one-mask-word kernel built for 8 wavefronts and at most 80 KB of LDS: two workgroups per CU
int pdmpc_launch_bulk_compact(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
int pdmpc_launch_bulk_compact_any(const KernelArgs* args, int count, void* stream, uint32_t* lds_high_water);
// util_kernels.hip: (cost-to-come of the final node, status) of n result records into lean[2 * n]
int pdmpc_launch_gather_lean(const pdmpc_vehicle_out* out, int n, int Hp, double* lean, void* stream);
// debug_kernels.hip: the first n doubles of mt19937ar(seeds[i]) for every i, by the sampled kernel's device generator (out: [count][n])
int pdmpc_launch_debug_mt19937(const uint32_t* seeds, int count, int n, double* out, void* stream);
// debug_kernels.hip: the open-list command script on one wavefront, and the collision primitives on given polygons (one wavefront per case)
int pdmpc_launch_heap_script(const int32_t* op, const int32_t* id, const double* key, int n, int32_t* out, unsigned long long* stats, double* gkey, uint32_t* gid, int HL,
                             void* stream);
// joint_kernel.hip: centralized control, one workgroup of one wavefront per joint problem
int pdmpc_launch_joint(const JointArgs* args, int n_problems, void* stream);
// priority_kernel.hip: the acyclic orientations of a coupling graph in ascending mask order, compacted in two passes over tiles of
// PDMPC_PRIO_TILE masks (count per tile, exclusive int64 scan, write), and the priorities of every written orientation
int pdmpc_launch_priority_count(const PriorityArgs* args, int64_t n_tiles, uint32_t* tile_count, void* stream);
int pdmpc_launch_priority_scan(const uint32_t* tile_count, int64_t n_tiles, int64_t* tile_off, void* stream);
int pdmpc_launch_priority_write(const PriorityArgs* args, int64_t n_tiles, const int64_t* tile_off, int64_t capacity, uint32_t* masks, void* stream);
int pdmpc_launch_priority_order(const PriorityArgs* args, const uint32_t* masks, int64_t count, int32_t* priorities, void* stream);
// ... and of several graphs in one call: the same passes over the tiles of all graphs (n_tiles <= PDMPC_PRIO_MAX_TILES), and behind the
// scan the pass that gathers the graphs' mask offsets into g->mask_first
int pdmpc_launch_priority_count_grouped(const PriorityGroups* g, int64_t n_tiles, uint32_t* tile_count, void* stream);
int pdmpc_launch_priority_group_offsets(const PriorityGroups* g, const int64_t* tile_off, void* stream);
int pdmpc_launch_priority_write_grouped(const PriorityGroups* g, int64_t n_tiles, const int64_t* tile_off, int64_t capacity, uint32_t* masks, void* stream);
int pdmpc_launch_priority_order_grouped(const PriorityGroups* g, const uint32_t* masks, int64_t count, int32_t* priorities, void* stream);
int pdmpc_launch_edge_check(int mode, int n_cases, const int32_t* a_off, const double* a_x, const double* a_y, const int32_t* b_off, const double* b_x,
                            const double* b_y, int32_t* hit, void* stream);
// debug_kernels.hip: interx_check on three soups per case (s_off[3 * n_cases + 1]), shape B in (b_x, b_y) at shape A's offsets; pdmpc_sincos on n arguments
int pdmpc_launch_interx_soups(int n_cases, const int32_t* a_off, const double* a_x, const double* a_y, const double* b_x, const double* b_y, const int32_t* s_off,
                              const double* s_x, const double* s_y, int32_t* hit, void* stream);
int pdmpc_launch_debug_sincos(const double* x, int n, double* s, double* c, void* stream);
#ifdef __cplusplus
}
#endif

#endif
