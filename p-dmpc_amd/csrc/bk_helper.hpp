// bk_helper.hpp — the helper workgroups of the graph search (included by bulk_search.hpp; what they share with a search's owner: bk_shared.hpp).
#pragma once
#include "bk_shared.hpp"

namespace {

// Helper workgroups (the workgroups of a launch behind its searches, bulk_body).  A helper takes a SEAT at a search that shares its
// rounds (the board's WANT word; the search with the fewest seats; one fetch-and-add, once), mirrors that search's obstacle soup in
// its own LDS (literal obstacles, lanelet boundary, the areas of the predecessors the owner has incorporated, the expected areas of
// the others) and from then on polls ONE word that nobody else polls: its seat's assignment.  An assignment is a range of the
// round's posted records; the helper runs the owner's own check items on it, leaves one verdict word per entry and the round's number
// in its seat's done word.  It keeps the seat until the search ends, then looks for another search.  A helper never waits for
// anything but memory, so an owner that waits for its seats always gets them; helpers leave when every search of the launch has ended.
template <int CHECKER, class SW>
__device__ __forceinline__ void bulk_helper_body(const KernelArgs& A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LDS_AS unsigned char* lsm = (LDS_AS unsigned char*)smem;
    const int tid = threadIdx.x, lane = tid & (PDMPC_WAVE - 1), wave = uni_i(tid >> 6), bd = (int)blockDim.x;
    const int Hp = A.Hp, n_s = A.n_searches;
    const uint32_t CAP = (uint32_t)A.bk_tile;  // records of a range (what fits the staging area)
    // the owners' carve (search_prologue): only the regions a check item reads are filled
    LDS_AS LdsPathRegion* l_pr = (LDS_AS LdsPathRegion*)(lsm + PDMPC_LK_PATH);
    lds_i32* l_soff = l_pr->soff;
    lds_i32* l_hoff = l_pr->hoff;
    volatile lds_u32* hs = l_pr->shared;  // (HS_*: lds_layout.hpp)
    lds_i32* l_lit = l_pr->lit;
    lds_d2* l_soup = (lds_d2*)(lsm + A.lds.soup);
    lds_d2* t_rec = (lds_d2*)(lsm + PDMPC_LK_NEAR_KEY);              // [bk_tile][3] the range's posted records
    volatile lds_u32* t_flag = (volatile lds_u32*)(lsm + PDMPC_LK_READY);  // [bk_tile] collision flags
    lds_u32* chm = bk_misc(lsm)->chm;
    BkCheck CK;
    CK.l_area = (const lds_d2*)(lsm + A.lds.area);
    CK.g_area = (const d2*)A.man_area;
    CK.l_soup = l_soup;
    CK.l_soff = l_soff;
    CK.l_hoff = l_hoff;
    CK.l_lit = l_lit;
    CK.areas_in_lds = SW::areas_in_lds(A);
    CK.ll_base = 0;
    CK.ll_len = 0;
    CK.Hp = Hp;
    const lds_u32* rcnt = BK_RCNT(lsm);
    if (SW::areas_in_lds(A)) stage16(lsm + A.lds.area, A.man_area, A.n_man * 3 * PDMPC_VMAX, tid);
    if (tid < PDMPC_SH_WORDS) hs[tid] = 0;
    __syncthreads();
    int my_slot = -1, my_seat = -1;  // (uniform)
    uint32_t last_seq = 0;
    unsigned long long cur_mask = 0;
    const int pref = (int)blockIdx.x % n_s;  // where this helper starts to look
    SpecCtx P;
    P.sh = hs;
    P.l_soup = l_soup;
    P.l_soff = l_soff;
    P.l_lit = l_lit;
    P.out = A.out;
    P.pred = A.pred;
    P.counters = A.tie_count;
    P.n_pred = 0;
    P.Hp = Hp;
    uint32_t idle = 0;
    // (PDMPC_TUNING=debug_tail=1: where a helper's time goes, 100 MHz ticks summed over its ranges: idle, from the assignment to the
    // soup in place, the range's records, its check items, verdicts + report; work_count[8..12], [13] = ranges)
    const bool hticking = SW::debug_tail(A) != 0 && tid == 0;
    unsigned long long hk_mark = hticking ? __builtin_amdgcn_s_memrealtime() : 0ull, hk[5] = {0, 0, 0, 0, 0}, hk_tiles = 0;
    const unsigned long long hk_start = hk_mark;
#define HK_TICK(i)                                                        \
    if (hticking) {                                                       \
        const unsigned long long n__ = __builtin_amdgcn_s_memrealtime(); \
        hk[i] += n__ - hk_mark;                                           \
        hk_mark = n__;                                                    \
    }
    for (;;) {
        // ================= no seat: look for a search that shares its rounds =================
        if (my_slot < 0) {
            if (wave == 0) {
                // one lane per search: candidates say so in their WANT word; the one with the most work per seat is joined (work = nodes
                // processed so far: a step takes as long as its heaviest search, and that is where the helpers belong)
                float best_score = -1.0f;
                int best_rel = -1;
                for (int base = 0; base < n_s; base += PDMPC_WAVE) {  // (uniform trip count)
                    const int k = base + lane;
                    const int s_rel = k < n_s ? (pref + k) % n_s : 0;
                    const unsigned long long* b = A.help_board + (size_t)(A.first + s_rel) * PDMPC_HB_WORDS;
                    const unsigned long long want = __hip_atomic_load(b + PDMPC_HB_WANT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long sw = __hip_atomic_load(b + PDMPC_HB_SEATS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long wt = __hip_atomic_load(b + PDMPC_HB_WEIGHT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t cnt = PDMPC_HB_SEATS_TAKEN(sw, A.launch_id);
                    // (a seat is kept until the search ends, so a search only gets the seats its work so far entitles it to: its share of the
                    // launch's helpers per 256 nodes processed — plenty of helpers per search (C2): every seat at once; a fifth of a helper
                    // per search (C4): a medium search holds one or two, the 10^5-node search of the step collects all 64 as it grows)
                    uint32_t allowed = 1u + (uint32_t)((wt * (unsigned long long)A.n_helpers) / ((unsigned long long)n_s * (unsigned long long)A.bk_seat_nodes));
                    if (idle >= 8u) allowed = (uint32_t)PDMPC_HB_SEATS_MAX;  // (this helper has found nothing it was entitled to for a while: better seated than idle)
                    allowed = allowed < (uint32_t)PDMPC_HB_SEATS_MAX ? allowed : (uint32_t)PDMPC_HB_SEATS_MAX;
                    const bool cand = k < n_s && want == (unsigned long long)A.launch_id && cnt < allowed;
                    const float score = cand ? (float)(wt + 1ull) / (float)(cnt + 1u) : -1.0f;
                    float c = score;
#pragma unroll
                    for (int o = PDMPC_WAVE / 2; o > 0; o >>= 1) {
                        const float v = __shfl_xor(c, o);
                        c = v > c ? v : c;
                    }
                    const unsigned long long m = __ballot(cand && score == c);
                    if (m && c > best_score) {  // (uniform)
                        best_score = c;
                        best_rel = (pref + base + (int)__builtin_ctzll(m)) % n_s;
                    }
                }
                uint32_t got = 0xffffffffu;
                if (best_rel >= 0) {  // (uniform) take a seat: one fetch-and-add; a stale word (another launch's) gives nothing
                    unsigned long long old = 0;
                    if (lane == 0)
                        old = __hip_atomic_fetch_add(A.help_board + (size_t)(A.first + best_rel) * PDMPC_HB_WORDS + PDMPC_HB_SEATS, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t lo32 = uni_u((uint32_t)pdmpc_hb_seats_count(old)), hi32 = uni_u(pdmpc_hb_seats_launch(old));
                    if (hi32 == A.launch_id && lo32 < (uint32_t)PDMPC_HB_SEATS_MAX) got = lo32;
                }
                uint32_t cmd = 0;
                if (got != 0xffffffffu) {
                    cmd = 1;
                } else {
                    const uint32_t fin = __hip_atomic_load(A.help_finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (fin - A.help_fin_base >= (uint32_t)n_s) cmd = 2;
                }
                if (lane == 0) {
                    hs[HS_SLOT] = (uint32_t)(A.first + (best_rel >= 0 ? best_rel : 0));
                    hs[HS_FIRST] = got;
                    hs[HS_CMD] = cmd;
                }
            }
            __syncthreads();
            const uint32_t cmd = hs[HS_CMD];
            if (cmd == 2u) break;
            if (cmd == 0u) {  // nobody shares: look again in a while (a search announces itself once; nothing is lost by being a few microseconds late)
                __builtin_amdgcn_s_sleep(127);
                __builtin_amdgcn_s_sleep(127);
                if (++idle > (A.spin_limit >> 4)) break;  // (uniform) the searches never came: leave; they do without helpers
                __syncthreads();
                continue;
            }
            my_slot = (int)hs[HS_SLOT];
            my_seat = (int)hs[HS_FIRST];
            last_seq = 0;
            idle = 0;
            // ---- the search's obstacle soup, as its owner has it (bk_shared.hpp); its predecessors' slots start empty
            const DevVehicle* __restrict__ V = A.veh + my_slot;
            const int pred_cols = V->n_pred * PDMPC_VMAX;
            int off = 0;
            BK_STAGE_SOUPS(A, V, l_soup, l_soff, l_hoff, l_lit, Hp, pred_cols, tid, off)
            CK.ll_base = off;
            CK.ll_len = V->ll_len;
            __syncthreads();
            BK_CLEAR_PRED_SLOTS(l_soup, l_soff, l_lit, Hp, pred_cols, tid, bd)
            __syncthreads();
            P.pred = A.pred + V->pred_off;
            P.n_pred = V->n_pred;
            if (SW::tentative(A)) bk_tentative_areas(A, P, PDMPC_ALL_PREDECESSORS(V->n_pred), tid, bd);  // (as the owner: expected areas until the real ones are in)
            cur_mask = 0;
            if (CHECKER == PDMPC_CHECK_INTERX) {  // (this helper's own lists of its own copy of the soup)
                bk_reach_boxes(A, V, lsm, tid);
                if (tid == 0) bk_reach_scalars(CK, lsm, A.lds.reach_shared != 0u);
            }
            __syncthreads();
            if (CHECKER == PDMPC_CHECK_INTERX) {
                bk_reach_build<7>(CK, lsm, lane, wave, bd >> 6);
                __syncthreads();
            }
            bk_chunk_table<CHECKER>(CK, rcnt, chm, tid);  // the chunk table of this soup (bulk_search)
            __syncthreads();
            if (hticking) hk_mark = __builtin_amdgcn_s_memrealtime();
            continue;
        }
        // ================= seated: this seat's assignment word =================
        unsigned long long* board = A.help_board + (size_t)my_slot * PDMPC_HB_WORDS;
        if (wave == 0) {
            const unsigned long long w = __hip_atomic_load(board + PDMPC_HB_ASSIGN + my_seat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t seq = pdmpc_hb_assign_round(w);
            uint32_t cmd = 0;
            if (seq != last_seq && seq != 0u) {
                cmd = 1;
                const unsigned long long mask = __hip_atomic_load(board + PDMPC_HB_MASK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane == 0) {
                    hs[HS_FIRST] = pdmpc_hb_assign_first(w);
                    hs[HS_COUNT] = pdmpc_hb_assign_count(w);
                    hs[HS_TICKET] = seq;
                    hs[HS_MASK_LO] = (uint32_t)mask;
                    hs[HS_MASK_HI] = (uint32_t)(mask >> 32);
                }
            } else if ((idle & 15u) == 15u) {  // (now and then) has the search ended?
                const unsigned long long want = __hip_atomic_load(board + PDMPC_HB_WANT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (want != (unsigned long long)A.launch_id) cmd = 3;
            }
            if (lane == 0) hs[HS_CMD] = cmd;
        }
        __syncthreads();
        const uint32_t cmd = hs[HS_CMD];
        if (cmd == 3u) {  // the seat's search is over: look for another one
            my_slot = -1;
            my_seat = -1;
            idle = 0;
            __syncthreads();
            continue;
        }
        if (cmd == 0u) {
            if (idle < 256u)
                __builtin_amdgcn_s_sleep(1);
            else
                __builtin_amdgcn_s_sleep(16);
            if (++idle > A.spin_limit) break;  // (uniform) must never happen: the search ends and says so
            __syncthreads();
            continue;
        }
        idle = 0;
        HK_TICK(0)
        const uint32_t first = hs[HS_FIRST], Rt = hs[HS_COUNT] < CAP ? hs[HS_COUNT] : CAP, seq = hs[HS_TICKET];
        const unsigned long long mask = ((unsigned long long)hs[HS_MASK_HI] << 32) | hs[HS_MASK_LO];
        last_seq = seq;
        if (mask != cur_mask) {  // (within a launch a search's set of incorporated predecessors only grows)
            bk_incorporate(P.out, P.pred, P.l_soup, P.l_soff, P.l_lit, Hp, mask & ~cur_mask, tid, bd, nullptr, nullptr);  // (loads that are coherent by themselves)
            cur_mask = mask;
            if (CHECKER == PDMPC_CHECK_INTERX) {  // (uniform) the lists of the steps' vehicle obstacles follow the soup
                __syncthreads();
                bk_reach_build<1>(CK, lsm, lane, wave, bd >> 6);
                __syncthreads();
                bk_chunk_table<CHECKER>(CK, rcnt, chm, tid);
            }
        }
        HK_TICK(1)
        // ---- the range: its records into LDS, its check items, its verdicts
        {
            const d2* post = (const d2*)A.bk_post + ((size_t)my_slot * (size_t)A.bk_ready_cap + first) * 3u;
            for (uint32_t i = (uint32_t)tid; i < Rt * 3u; i += (uint32_t)bd) t_rec[i] = bk_post_load(post + i);
            for (uint32_t i = (uint32_t)tid; i < Rt; i += (uint32_t)bd) t_flag[i] = 0u;
        }
        __syncthreads();
        HK_TICK(2)
        if (Rt) {
            const BkPostSrc psrc{t_rec};
            const int ls = bk_chunk_shift(chm, Rt, (uint32_t)bd);
            const unsigned long long pend = SW::tentative(A) ? PDMPC_ALL_PREDECESSORS(P.n_pred) & ~mask : 0ull;
            bk_check_items<CHECKER>(CK, psrc, t_flag, 0u, Rt, ls, chm[ls], pend, tid, bd);
        }
        __syncthreads();
        HK_TICK(3)
        {
            uint32_t* verdict = A.help_verdict + (size_t)my_slot * PDMPC_HELP_CAP + first;
            for (uint32_t i = (uint32_t)tid; i < Rt; i += (uint32_t)bd) {  // 1 collision-free, 2 collides, 3 crosses expected areas only
                const uint32_t fl = t_flag[i];
                __hip_atomic_store(verdict + i, pdmpc_hb_verdict(fl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's verdicts have been acknowledged (the barrier alone does not wait for them) ...
        __syncthreads();                                     // ... every wave's have: the seat's done word can say so
        if (tid == 0) {
            __hip_atomic_store(board + PDMPC_HB_DONE + my_seat, (unsigned long long)seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            hs[HS_CMD] = 0;
        }
        __syncthreads();
        HK_TICK(4)
        hk_tiles += 1;
    }
    if (hticking) {
        atomicAdd(A.work_count + 7, __builtin_amdgcn_s_memrealtime() - hk_start);  // (this helper's lifetime)
        for (int i = 0; i < 5; ++i) atomicAdd(A.work_count + 8 + i, hk[i]);
        atomicAdd(A.work_count + 13, hk_tiles);
    }
#undef HK_TICK
}

}  // namespace
