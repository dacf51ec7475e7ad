// lds_layout.hpp — where the graph search keeps what in LDS, declared once (device code, included by search_common.hpp): the words the
// wavefronts of a workgroup share (a search's block, a helper workgroup's block), and the regions of the fixed layout
// (pdmpc_device.h: PDMPC_LK_*) that hold several small tables: the 2 KB at PDMPC_LK_MISC, the 12 KB at PDMPC_LK_HIST, and what follows
// the areas in the region at PDMPC_LK_PSHAPE.  A new shared word or small table is declared HERE; the
// static_asserts below refuse two names on one word and a region that does not have the size pdmpc_device.h gives it.
#pragma once
#include <cstddef>

// ---------------------------------------------------------------------------------------------------
// The shared words of a search: LdsPathRegion::shared, PDMPC_SH_WORDS 32-bit words, every one zeroed by the prologue.
// X(name, index, bits): in index order, one name per word; a 64-bit word (sh_ld_d / sh_st_d / sh_min_d / sh_max_d) takes an even index
// and the word behind it.  The comment says who writes the word.
#define SH_WORD_TABLE(X)                                                                                                                  \
    X(SH_STATE, 0, 32)       /* ST_RUN searching, ST_ARRIVED predecessors have finished (SH_ARR says who): bk_poll_predecessors, the arrival block */ \
    /* 1, 2: free */                                                                                                                      \
    X(SH_NNODES, 3, 32)      /* 1 once the root exists (the root's initialisation; nobody reads it: the tree's size is FR_NNODES) */      \
    /* 4: free */                                                                                                                         \
    X(SH_PEND_LO, 5, 32)     /* predecessors whose areas are not in the soup yet (bit p = p-th predecessor): prologue, arrival block, bk_wait_done */ \
    X(SH_PEND_HI, 6, 32)                                                                                                                  \
    X(SH_ARR_LO, 7, 32)      /* predecessors that just finished (to be copied into the soup): prologue, bk_poll_predecessors */          \
    X(SH_ARR_HI, 8, 32)                                                                                                                   \
    /* 9: free */                                                                                                                         \
    X(BK_MID_N, 10, 32)      /* entries of mid: to_far, the refill */                                                                     \
    X(BK_MID_PAD, 11, 32)    /* cleared with BK_MID_N by the root's initialisation, otherwise unused */                                   \
    X(BK_MID_MIN, 12, 64)    /* exact minimum key of mid: flush_far, the refill */                                                        \
    X(BK_L_MID, 14, 64)      /* open entries that leave near, and children beyond near's limit, go to mid up to this key and to far above it (-1: no mid list): the refill */ \
    X(BK_FD_LO, 16, 32)      /* predecessors whose areas are in the soup and have passed the path of the finished plan, but whose re-check of the */ \
    X(BK_FD_HI, 17, 32)      /*   other collision-free nodes is still to come (they stay in SH_PEND until the arrival block has seen them): bk_wait_done, arrival block */ \
    X(BK_WAITRES, 18, 32)    /* result of bk_wait_done: 0 nothing yet, 1 an arrival crosses the path, 2 the last predecessor has passed: published */ \
    X(BK_PUBLISHED, 19, 32)  /* the done flag is out (bk_wait_done): the areas of the record in HBM are final and may be read; only counts and ids may still be written */ \
    X(BK_TIEMODE, 20, 32)    /* the search has met equal keys where the pop order decides (or PDMPC_BK_FORCE_TIE): it ends on bk_replay; the round boundary */ \
    X(BK_RP_NEED, 21, 32)    /* bk_replay: a node (1-based) the reference's heap pops that no round has evaluated (0: none) */            \
    X(BK_RP_GOAL, 22, 32)    /* ... the goal it ended on (1-based arena index, 0: exhausted) */                                           \
    X(BK_RP_NPOP, 23, 32)    /* ... nodes popped */                                                                                       \
    X(BK_RP_NREF, 24, 32)    /* ... nodes of the reference's tree */                                                                      \
    /* 25: free */                                                                                                                        \
    X(BK_TENT_MIN, 26, 64)   /* smallest key among the parked nodes: P2, the arrival block */                                             \
    X(FR_ROUND_B1, 28, 64)   /* smallest path maximum among the round's goal candidates: fr_resolve_goals */                             \
    X(FR_PB_ALL_A, 30, 32)   /* phase B: "every node of the chunk is resolved", two words taken in turn (fr_phase_b) */                   \
    X(FR_PB_ALL_B, 31, 32)                                                                                                                \
    X(FR_NNODES, 32, 32)     /* tree size (atomic reservation of node indices): P2 */                                                     \
    X(BK_DEPTH, 33, 32)      /* deepest collision-free node so far (its step k): P2 */                                                    \
    X(BK_IDLE, 34, 32)       /* polls a waiting search has made (the watchdog's count): bk_wait, bk_wait_done */                          \
    /* 35: free */                                                                                                                        \
    X(FR_NEAR_N, 36, 32)     /* entries of near: to_near, the selection */                                                                \
    X(FR_FAR_N, 37, 32)      /* entries of far: to_far, the refill */                                                                     \
    X(FR_FLAGS, 38, 32)      /* FRF_*: anybody, with atomicOr */                                                                          \
    X(FR_GOAL_N, 39, 32)     /* goal candidates of the running round (entries of goal_list): P2, fr_resolve_goals */                      \
    X(FR_BEST_ID, 40, 32)    /* best goal candidate so far (1-based node, 0 = none): fr_resolve_goals, the arrival block */               \
    X(FR_SEL_BIN, 41, 32)    /* result of fr_select2: bin ... (between refills: the size of the next round, the selection) */             \
    X(FR_SEL_CUM, 42, 32)    /* ... and the number of entries up to and including it */                                                   \
    X(BK_NTENT, 43, 32)      /* parked nodes: P2, the arrival block */                                                                    \
    X(BK_ARRIVALS, 44, 32)   /* arrival events handled by this search: the arrival block */                                               \
    X(FR_ROUNDS, 45, 32)     /* rounds so far: the round boundary */                                                                      \
    X(FR_BEST_B1, 46, 64)    /* largest key on the best candidate's path: fr_resolve_goals */                                             \
    X(FR_NEAR_MIN, 48, 64)   /* exact minimum key of near: flush_near, the selection */                                                   \
    X(FR_NEAR_MAX, 50, 64)   /* upper bound of near's keys */                                                                             \
    X(FR_FAR_MIN, 52, 64)    /* exact minimum key of far: flush_far, the refill */                                                        \
    X(FR_FAR_MAX, 54, 64)    /* upper bound of far's keys */                                                                              \
    X(FR_HELP_CLOSED, 56, 32) /* shared round: entries of the shared part the helpers claimed before the owner closed it: P1 */           \
    X(FR_DEAD, 57, 32)       /* open entries dropped because an ancestor was invalidated: the selection */                                \
    X(FR_L_FAR, 58, 64)      /* children with key > this go to far: the selection, the refill */                                          \
    X(FR_PROCESSED, 60, 32)  /* nodes processed so far: the round boundary */                                                             \
    X(FR_PATH_FOR, 61, 32)   /* the goal candidate whose path is in the relevance tables (0: none): the round boundary */                 \
    X(FR_DROPPED, 62, 32)    /* open entries dropped because they come after the best candidate (restored if that one is invalidated): the selection */ \
    X(FR_EVER_INVAL, 63, 32) /* set once a late arrival has invalidated a node of this search: the arrival block */                       \
    X(FR_SCRATCH, 64, 64 * 32) /* one scratch word per lane: targets of the lanes that only take part pro forma (sh_add_uniform, to_far) */
// the root's initialisation (bulk_search) zeroes the words from this one to the end of the block once more; the words below it keep
// what the prologue left (SH_PEND) or are set one by one
#define SH_ROOT_CLEAR 26
#define ST_RUN 0u
#define ST_ARRIVED 1u

// The shared words of a helper workgroup (bulk_helper_body: the same block of its own LDS), written by its first wavefront.
#define HS_WORD_TABLE(X)                                                                                       \
    X(HS_CMD, 0, 32)     /* 0 nothing found, 1 work, 2 every search has finished, 3 the seat's search is over */ \
    X(HS_SLOT, 1, 32)    /* the search this helper has taken a seat at */                                       \
    X(HS_FIRST, 2, 32)   /* the seat it got; seated: first entry of the assigned range */                       \
    X(HS_COUNT, 3, 32)   /* entries of the range */                                                             \
    X(HS_MASK_LO, 4, 32) /* predecessors whose areas the owner has in its soup */                               \
    X(HS_MASK_HI, 5, 32)                                                                                        \
    X(HS_TICKET, 6, 32)  /* the shared round's number */                                                        \
    /* 7 .. PDMPC_SH_WORDS - 1: free */

#define LDS_WORD_ENUM(name, index, bits) name = (index),
#define LDS_WORD_ENTRY(name, index, bits) {(index), (bits)},
enum : int { SH_WORD_TABLE(LDS_WORD_ENUM) };
enum : int { HS_WORD_TABLE(LDS_WORD_ENUM) };
struct LdsWord {
    int index, bits;
};
constexpr LdsWord kShWords[] = {SH_WORD_TABLE(LDS_WORD_ENTRY)};
constexpr LdsWord kHsWords[] = {HS_WORD_TABLE(LDS_WORD_ENTRY)};
#undef LDS_WORD_ENUM
#undef LDS_WORD_ENTRY
// every entry a whole number of words inside the block, behind the entry in front of it; a 64-bit entry at an even index
template <int N>
constexpr bool lds_words_disjoint(const LdsWord (&t)[N], int block_words) {
    int next = 0;
    for (int i = 0; i < N; ++i) {
        const int words = t[i].bits / 32;
        if (words < 1 || words * 32 != t[i].bits) return false;
        if (t[i].index < next || t[i].index + words > block_words) return false;
        if (t[i].bits == 64 && (t[i].index & 1) != 0) return false;
        next = t[i].index + words;
    }
    return true;
}
static_assert(lds_words_disjoint(kShWords, PDMPC_SH_WORDS), "two shared words of the search overlap, a 64-bit word is misaligned, or one lies outside the block");
static_assert(lds_words_disjoint(kHsWords, PDMPC_SH_WORDS), "two shared words of a helper workgroup overlap or lie outside the block");
static_assert(FR_SCRATCH + PDMPC_WAVE == PDMPC_SH_WORDS, "one scratch word per lane ends the block");

// ---------------------------------------------------------------------------------------------------
// The 2 KB at PDMPC_LK_MISC: small tables of the owner of a search (bulk_search, bulk_body); a helper workgroup uses chm alone.
struct BkMisc {
    uint32_t gp_path[32];           // [Hp + 1] path of the best goal candidate
    double gp_mp[32];               // [HP_MAX + 1] largest key of that path below depth d
    unsigned long long wsum64[32];  // scan partials (wg_scan_excl: two arrays of PDMPC_MAX_WAVES, taken in turn)
    uint32_t wsum[32];              // fr_partition's per-wave counts (likewise)
    uint32_t chm[8];                // chunks per node for S = 1, 2, 4, 8, 16, ... (bk_chunk_table)
    unsigned long long tk[12];      // (debug_tail) ticks: mark, start, work, arrival, select (without the refills), wait, p1, p2, p3, phase B, refill, time of the early publication
    uint32_t ref_ids[PDMPC_HP_MAX + 2];  // the ids the nodes of the plan's path carry in the reference's tree (phase B, bk_replay -> bk_write_record)
    unsigned long long tk2[7];      // (debug_tail) the arrival handling in detail: poll + copy, re-check items, parked nodes' return, bookkeeping + candidates, record + flag of a finished search, finding the nodes to re-check; mark
    uint32_t bins[256];             // [BK_NB] the selection's histogram
};
static_assert(sizeof(BkMisc) == 2048, "PDMPC_LKX_PSHAPE puts the next region 2048 bytes behind PDMPC_LKX_MISC");
static_assert(offsetof(BkMisc, bins) == 1024, "the selection's histogram is the second KB of the region");
static_assert(offsetof(BkMisc, tk) % 8 == 0 && offsetof(BkMisc, tk2) % 8 == 0 && offsetof(BkMisc, tk2) == offsetof(BkMisc, ref_ids) + sizeof(BkMisc::ref_ids), "no padding between the tables");

// The 12 KB at PDMPC_LK_HIST.  During a round: the goal candidates, a tile's expansion groups, their children's offsets.  Between rounds the
// refill's histogram of FR_NBINS bins lies over goal_list and vlist, and phase B's tables (fr_phase_b) start at goal_list.
struct BkHist {
    uint32_t goal_list[1024];  // goal candidates of the running round
    uint32_t vlist[1024];      // expansion groups of a tile
    uint32_t voffs[1024];      // ... and where their children go
};
static_assert(sizeof(BkHist) == 3072 * 4, "PDMPC_LKX_MISC puts the next region 3072 words behind PDMPC_LKX_HIST");

namespace {

typedef LDS_AS unsigned long long lds_u64s;

__device__ __forceinline__ LDS_AS BkMisc* bk_misc(LDS_AS unsigned char* lsm) { return (LDS_AS BkMisc*)(lsm + PDMPC_LK_MISC); }
__device__ __forceinline__ LDS_AS BkHist* bk_hist(LDS_AS unsigned char* lsm) { return (LDS_AS BkHist*)(lsm + PDMPC_LK_HIST); }

}  // namespace

// The region at PDMPC_LK_PSHAPE: the areas along the path of the record written last, and behind them — the stride follows the launch's
// Hp, not HP_MAX — three tables of HP_MAX entries (the region's size: PDMPC_LKX_REACH).  Macros like BK_RBOX, not functions: the same
// arithmetic behind an inlined call gave the search kernels another register allocation.
#define BK_PSHAPE(lsm) ((lds_d2*)((lsm) + PDMPC_LK_PSHAPE))                                /* [Hp][VMAX] the areas (bk_write_record; what an arrival is checked against first, bk_wait_done) */
#define BK_PCOLS(pshape, Hp) ((lds_u32*)((pshape) + (Hp) * PDMPC_VMAX))                    /* [HP_MAX] their column counts */
#define BK_PCHG(pshape, Hp) ((lds_u64s*)(BK_PCOLS(pshape, Hp) + PDMPC_HP_MAX))             /* [HP_MAX] per step the predecessors whose areas differ from the expected ones (bk_incorporate) */
#define BK_PVCNT(pshape, Hp) ((lds_u32*)(BK_PCHG(pshape, Hp) + PDMPC_HP_MAX))              /* [HP_MAX] collision-free nodes per step: the lengths of the verification's lists (BK_VLIST) */
