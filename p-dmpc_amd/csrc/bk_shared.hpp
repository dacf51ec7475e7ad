// bk_shared.hpp — the contract between the owner of a search (bulk_search.hpp) and the helper workgroups seated at it (bk_helper.hpp):
// everything BOTH run, stated once.  A helper's verdicts are the owner's only if its mirror of the obstacle soup has the owner's layout
// column for column (l_soff, l_hoff, l_lit, ll_base, the NaN slots of the predecessors, the reach lists, the chunk table) and its check
// items are the owner's: so the soup is staged (BK_STAGE_SOUPS, BK_CLEAR_PRED_SLOTS), its lists are built (bk_reach_boxes,
// bk_reach_scalars, bk_reach_build, bk_chunk_table), arrived areas are copied in (bk_incorporate) and an entry is checked
// (bk_check_items) by the text below on either side.  The words of the board they talk through: pdmpc_device.h (pdmpc_hb_*).
// (included by search_common.hpp behind the types it rests on: SpecCtx, the LDS layout, the wavefront primitives)
#pragma once
#include "../../include/pdmpc_reach.h"

namespace {

typedef volatile LDS_AS unsigned long long lds_vu64;
typedef LDS_AS uint16_t lds_u16;

// piece q (16 bytes) of node i0's record: LDS copy if it has one
__device__ __forceinline__ d2 node_piece(const Search& S, uint32_t i0, int q) {
    if (i0 < S.NL) return S.ln[4 * (size_t)i0 + q];
    return ((const d2*)(S.gn + i0))[q];
}
__device__ __forceinline__ void piece_link(d2 p3, uint32_t& parent, uint32_t& packed) {
    const uint64_t u = (uint64_t)__double_as_longlong(p3.y);
    parent = (uint32_t)(u & 0xffffffffull);
    packed = (uint32_t)(u >> 32);
}

// What a check item reads.  The same for the owner of a search and for a workgroup that helps it.
struct BkCheck {
    const lds_d2* l_area;
    const d2* g_area;
    const lds_d2* l_soup;
    const lds_i32* l_soff;
    const lds_i32* l_hoff;
    const lds_i32* l_lit;  // literal soup length per step (the predecessors' slots of VMAX columns each follow)
    int areas_in_lds, ll_base, ll_len, Hp;
};

// The obstacle soup of search V into LDS, in the layout every check item and every list assumes: per step [literal polygons + NaN]
// [predecessors' areas, VMAX columns each] (vectorize_all_obstacles.m:36-62), then the steps' HDV sets, the lanelet boundary last.  Thread 0
// writes where each soup begins (l_soff, l_hoff: [Hp + 1]) and the literal lengths (l_lit).  `off` is the caller's `int off = 0;` and
// ends as the boundary's first column.  Every thread of the workgroup runs it; the caller's barrier follows.  BK_CLEAR_PRED_SLOTS, behind
// that barrier: the predecessors' slots start as NaN, i.e. no obstacle.
// (Macros, not functions: as stage_soups() / clear_pred_slots() with this very text the two moved the register allocation of the whole
// kernel and its round loop's scalar reloads past the bar of tests/test_build_specialized.py)
#define BK_STAGE_SOUPS(A, V, l_soup, l_soff, l_hoff, l_lit, Hp, pred_cols, tid, off)                \
    for (int k = 0; k < Hp; ++k) {                                                                  \
        const int a = V->lit_off[k], b = V->lit_off[k + 1];                                         \
        if (tid == 0) {                                                                             \
            l_soff[k] = off;                                                                        \
            l_lit[k] = b - a;                                                                       \
        }                                                                                           \
        stage16(l_soup + off, (const d2*)A.points + a, b - a, tid);                                 \
        off += (b - a) + pred_cols;                                                                 \
    }                                                                                               \
    if (tid == 0) l_soff[Hp] = off;                                                                 \
    for (int k = 0; k < Hp; ++k) {                                                                  \
        const int a = V->hdv_off[k], b = V->hdv_off[k + 1];                                         \
        if (tid == 0) l_hoff[k] = off;                                                              \
        stage16(l_soup + off, (const d2*)A.points + a, b - a, tid);                                 \
        off += (b - a);                                                                             \
    }                                                                                               \
    if (tid == 0) l_hoff[Hp] = off;                                                                 \
    stage16(l_soup + off, (const d2*)A.points + V->ll_off, V->ll_len, tid);
#define BK_CLEAR_PRED_SLOTS(l_soup, l_soff, l_lit, Hp, pred_cols, tid, nthreads)                                                     \
    {                                                                                                                                \
        const d2 nanpt = d2{__longlong_as_double(0x7ff8000000000000LL), __longlong_as_double(0x7ff8000000000000LL)};                 \
        for (int idx = tid; idx < Hp * pred_cols; idx += nthreads) {                                                                 \
            const int k = idx / pred_cols;                                                                                           \
            l_soup[l_soff[k] + l_lit[k] + (idx - k * pred_cols)] = nanpt;                                                            \
        }                                                                                                                            \
    }

// The reach lists (include/pdmpc_reach.h): per step and soup the segments an edge check of that step can meet
// at all, ascending, with their counts.  Rectangles, root, counts and lists live at compile-time offsets (PDMPC_LK_REACH; the lists of run-time
// length behind the fixed regions, in front of the automaton's tables: no register holds their address): the list of a step's vehicle
// obstacles / HDV sets at the index of that soup's first column, the boundary's list of step k at ll_base + (k - 1) * ll_len.
#define BK_RLIST(lsm) ((lds_u16*)((lsm) + PDMPC_LK_FIXED_END))
// (the base of the dynamic LDS allocation as the constant it is: what a check item reads of these regions costs no register)
__device__ __forceinline__ LDS_AS unsigned char* bk_lds_base() {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    return (LDS_AS unsigned char*)smem;
}
#define BK_RBOX(lsm) ((lds_f64*)((lsm) + PDMPC_LK_REACH))
#define BK_RCNT(lsm) ((lds_u32*)((lsm) + PDMPC_LK_REACH + PDMPC_LK_REACH_CNT))
#define BK_RSTALE(lsm) ((volatile lds_u32*)((lsm) + PDMPC_LK_REACH + PDMPC_LK_REACH_STALE))
#define BK_RSC(lsm) ((lds_i32*)((lsm) + PDMPC_LK_REACH + PDMPC_LK_REACH_SC))
#define BK_RROOT(lsm) ((lds_f64*)((lsm) + PDMPC_LK_REACH + PDMPC_LK_REACH_ROOT))
// What an InterX check item reads of its search besides the lists, as LDS words at constant addresses (the workgroup's scalar registers
// are spent, DESIGN.md section 3.9: a value read here is one LDS load per item, not a reload per use).  Thread 0 writes them.
__device__ __forceinline__ void bk_reach_scalars(const BkCheck& C, LDS_AS unsigned char* lsm, bool shared_boundary_list) {
    lds_i32* sc = BK_RSC(lsm);
    sc[0] = (int32_t)((LDS_AS unsigned char*)C.l_soup - lsm);
    sc[1] = (int32_t)((LDS_AS unsigned char*)C.l_area - lsm);
    sc[2] = C.Hp;
    sc[3] = C.ll_base;
    sc[4] = C.ll_len;
    sc[5] = shared_boundary_list ? 0 : C.ll_len;  // (one list of the boundary for every step, built against the rectangle around all steps' rectangles: a superset of each step's own)
}
struct BkItemCtx {  // the same values for a check item, each read where it is used: from the LDS words (InterX) or from the caller's registers
    const BkCheck& C;
    int interx;
    __device__ __forceinline__ int word(int i) const { return BK_RSC(bk_lds_base())[i]; }
    __device__ __forceinline__ const lds_d2* l_soup() const { return interx ? (const lds_d2*)(bk_lds_base() + word(0)) : C.l_soup; }
    __device__ __forceinline__ const lds_d2* l_area() const { return interx ? (const lds_d2*)(bk_lds_base() + word(1)) : C.l_area; }
    __device__ __forceinline__ int Hp() const { return interx ? word(2) : C.Hp; }
    __device__ __forceinline__ int ll_base() const { return interx ? word(3) : C.ll_base; }
    __device__ __forceinline__ int ll_stride() const { return interx ? word(5) : C.ll_len; }
};
template <int CHECKER>
__device__ __forceinline__ BkItemCtx bk_item_ctx(const BkCheck& C) {
    return BkItemCtx{C, CHECKER == PDMPC_CHECK_INTERX ? 1 : 0};
}
// the widened rectangles of the steps in the root's frame (tid < Hp; the automaton's reach sits behind its areas in HBM — Dmax, Amax, then
// [trim][step] rectangles —: read here only) and, once per search, the root: position, cos and sin of its yaw (thread Hp)
__device__ __forceinline__ void bk_reach_boxes(const KernelArgs& A, const DevVehicle* V, LDS_AS unsigned char* lsm, int tid) {
    if (tid < A.Hp) {
        // (32-bit index arithmetic: the 64-bit form of this address cost the generic kernels two spilled registers)
        const int at = A.n_man * (3 * PDMPC_VMAX * 2) + 2 + ((V->trim0 - 1) * A.Hp + tid) * 4;
        const double r[4] = {A.man_area[at], A.man_area[at + 1], A.man_area[at + 2], A.man_area[at + 3]};
        double box[4];
        pdmpc_reach_rect_box(r, V->x0, V->y0, box);
        lds_f64* rb = BK_RBOX(lsm) + 4 * tid;
        rb[0] = box[0];
        rb[1] = box[1];
        rb[2] = box[2];
        rb[3] = box[3];
    } else if (tid == A.Hp) {
        double cs, sn;
        pdmpc_sincos(V->yaw0, &sn, &cs);
        lds_f64* rr = BK_RROOT(lsm);
        rr[0] = V->x0;
        rr[1] = V->y0;
        rr[2] = cs;
        rr[3] = sn;
        if (A.lds.reach_shared != 0u) {  // (the layout of last resort: ONE list of the boundary for every step — a later step's rectangle need not hold an earlier one's)
            const double* rect = A.man_area + (A.n_man * (3 * PDMPC_VMAX * 2) + 2 + (V->trim0 - 1) * A.Hp * 4);
            double lo_x = 0.0, hi_x = 0.0, lo_y = 0.0, hi_y = 0.0;
            for (int k = 0; k < A.Hp; ++k) {
                const double r[4] = {rect[4 * k], rect[4 * k + 1], rect[4 * k + 2], rect[4 * k + 3]};
                double box[4];
                pdmpc_reach_rect_box(r, V->x0, V->y0, box);
                lo_x = k == 0 || !(box[0] >= lo_x) ? box[0] : lo_x;  // (a NaN stays: the rule then culls nothing)
                hi_x = k == 0 || !(box[1] <= hi_x) ? box[1] : hi_x;
                lo_y = k == 0 || !(box[2] >= lo_y) ? box[2] : lo_y;
                hi_y = k == 0 || !(box[3] <= hi_y) ? box[3] : hi_y;
            }
            rr[4] = lo_x;
            rr[5] = hi_x;
            rr[6] = lo_y;
            rr[7] = hi_y;
        }
    }
}
// One wavefront per (step, soup) — soups: bit 0 vehicle obstacles, 1 HDV sets, 2 lanelet boundary —: the segments 64 at a time, a ballot
// and the lanes' ranks in it compact the indices of those in reach.  Every wavefront of the workgroup calls; no barrier inside.
template <int SOUPS>
__device__ __forceinline__ void bk_reach_build(const BkCheck& C, LDS_AS unsigned char* lsm, int lane, int wave, int n_waves) {
    const lds_f64* rbox = BK_RBOX(lsm);
    lds_u32* rcnt = BK_RCNT(lsm);
    for (int u = wave; u < (SOUPS == 1 ? 1 : 3) * C.Hp; u += n_waves) {  // (uniform per wavefront)
        const int k = SOUPS == 1 ? u : u / 3, s = SOUPS == 1 ? 0 : u - 3 * k;  // (k: 0-based step)
        int base, n, at, kb = k;  // (kb: the step whose rectangle decides)
        bool one_list = false;  // (the boundary in the layout of last resort)
        if (s == 0) {
            base = C.l_soff[k];
            n = C.l_soff[k + 1] - base - 1;
            at = base;
        } else if (s == 1) {
            base = C.l_hoff[k];
            n = C.l_hoff[k + 1] - base - 1;
            at = base;
        } else {
            const int stride = BK_RSC(lsm)[5];  // (0: every step writes the same list and the same count)
            base = C.ll_base;
            n = C.ll_len - 1;
            at = base + k * stride;
            kb = stride ? k : C.Hp - 1;
            one_list = stride == 0;
        }
        const lds_f64* rb = one_list ? BK_RROOT(lsm) + 4 : rbox + 4 * kb;  // (one list for every step: the rectangle around the rectangles of all of them)
        const lds_f64* root = BK_RROOT(lsm);
        const lds_d2* q = C.l_soup + base;
        lds_u16* lst = BK_RLIST(lsm) + at;
        uint32_t cnt = 0;
        for (int j0 = 0; j0 < n; j0 += PDMPC_WAVE) {
            const int j = j0 + lane;
            bool in = false;
            if (j < n) {
                const d2 q0 = q[j], q1 = q[j + 1];  // (root and rectangle from LDS per trip: eight values held across the loop cost the generic kernels scratch memory)
                in = pdmpc_reach_in_oriented(q0.x, q0.y, q1.x, q1.y, root[0], root[1], root[2], root[3], rb[0], rb[1], rb[2], rb[3]) != 0;
            }
            const unsigned long long m = __ballot(in);
            if (in) lst[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)j;
            cnt += (uint32_t)__builtin_popcountll(m);
        }
        if (lane == 0) rcnt[s * PDMPC_HP_MAX + k] = cnt;
    }
}

// Tentative areas.  A predecessor that is still planning has its EXPECTED areas in its soup slots: what it publishes should its search
// be exhausted, i.e. its previous plan shifted by one step (PrioritizedController.m:568-616, 678-718) — where it most likely ends up
// driving.  An edge that crosses only such areas is neither collision-free nor colliding: its node is parked (VS_TENT) and comes back
// into the open set when a predecessor arrives.  The result is a function of the final areas alone (every node that comes before
// the goal ends up evaluated against them); what changes is that the plan found ahead of the arrivals usually survives them.
#define VS_TENT 6u
// (the shared words of the parked nodes, the mid list, the fast arrival path and the replay: lds_layout.hpp)

// copies the expected areas of the predecessors in `who` into their soup slots
__device__ __forceinline__ void bk_tentative_areas(const KernelArgs& A, const SpecCtx& P, unsigned long long who, int tid, int nthreads) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int per = P.Hp * PDMPC_VMAX, n_pred = P.n_pred < 64 ? P.n_pred : 64;
    for (int idx = tid; idx < n_pred * per; idx += nthreads) {  // (every pending predecessor's loads side by side)
        const int p = idx / per, rest = idx - p * per;
        if (!((who >> p) & 1ull)) continue;
        const DevVehicle* PV = A.veh + P.pred[p];
        if (PV->fb_off[0] < 0) continue;  // no expectation: its slots stay empty
        const int k = rest / PDMPC_VMAX, v = rest - k * PDMPC_VMAX;
        const int a = PV->fb_off[k], b = PV->fb_off[k + 1];
        const int cols = (b - a < PDMPC_VMAX) ? (b - a) : PDMPC_VMAX;
        d2 pt;
        pt.x = v < cols ? A.points[2 * (size_t)(a + (v < cols ? v : 0))] : qnan;
        pt.y = v < cols ? A.points[2 * (size_t)(a + (v < cols ? v : 0)) + 1] : qnan;
        P.l_soup[P.l_soff[k] + P.l_lit[k] + p * PDMPC_VMAX + v] = pt;
    }
}

// Where a check item finds its node: the owner of a search reads the tree (LDS copies where they exist), a workgroup that helps it
// reads the 48-byte records the owner has posted for the round (staged in the helper's LDS).
struct BkTreeSrc {
    const Search* S;
    const lds_u32* ready;
    __device__ __forceinline__ void link(uint32_t r, uint32_t& parent, uint32_t& packed) const { piece_link(node_piece(*S, ready[r] - 1u, 3), parent, packed); }
    __device__ __forceinline__ void pose(uint32_t, uint32_t parent, double& px, double& py, double& cs, double& sn) const {
        const d2 pxy = node_piece(*S, parent - 1u, 0), pcs = node_piece(*S, parent - 1u, 2);
        px = pxy.x;
        py = pxy.y;
        cs = pcs.x;
        sn = pcs.y;
    }
};
struct BkPostSrc {
    const lds_d2* rec;  // [tile][3]: (x, y) and (cos, sin) of the parent, (parent | packed << 32 as bits, -)
    __device__ __forceinline__ void link(uint32_t r, uint32_t& parent, uint32_t& packed) const { piece_link(d2{0.0, rec[3 * r + 2].x}, parent, packed); }
    __device__ __forceinline__ void pose(uint32_t r, uint32_t, double& px, double& py, double& cs, double& sn) const {
        const d2 pxy = rec[3 * r], pcs = rec[3 * r + 1];
        px = pxy.x;
        py = pxy.y;
        cs = pcs.x;
        sn = pcs.y;
    }
};

// P1, the check items of the entries r0 .. r0 + R - 1: item = c * R + r (chunk-major), chunk c = S = 1 << ls consecutive segments of
// one of the node's three soups (vehicle obstacles of its step and HDV sets against the area, lanelet boundary against the
// boundary-check area: are_constraints_satisfied_interx.m:17-37).  chmax = chunks of the step with the most segments.  Lanes work alone.
// What a node's check items cover, per soup: segments (InterX: the vehicle obstacles of its step, the HDV sets, the lanelet boundary) or,
// for the separating-axis checker, COLUMNS of the vehicle obstacles' soup — the lane whose chunk holds a polygon's first column tests
// that polygon whole (are_constraints_satisfied_sat.m:15-35; its HDV loop is dead code, :55-66) — and segments of the boundary (:46-53).
template <int CHECKER>
__device__ __forceinline__ void bk_item_counts(int M_k, int Hk, int ll_len, int& n0, int& n1, int& n2) {
    n0 = CHECKER == PDMPC_CHECK_INTERX ? (M_k > 1 ? M_k - 1 : 0) : M_k;
    n1 = CHECKER == PDMPC_CHECK_INTERX ? (Hk > 1 ? Hk - 1 : 0) : 0;
    n2 = ll_len > 1 ? ll_len - 1 : 0;
}
// what the check items of a node of step k (1-based) cover per soup: InterX the segments in reach (the lists' counts), the
// separating-axis checker all columns / boundary segments
template <int CHECKER>
__device__ __forceinline__ void bk_reach_counts(const BkCheck& C, const lds_u32* rcnt, int k, int& n0, int& n1, int& n2) {
    if (CHECKER == PDMPC_CHECK_INTERX) {
        n0 = (int)rcnt[k - 1];
        n1 = (int)rcnt[PDMPC_HP_MAX + k - 1];
        n2 = (int)rcnt[2 * PDMPC_HP_MAX + k - 1];
    } else {
        bk_item_counts<CHECKER>(C.l_soff[k] - C.l_soff[k - 1], C.l_hoff[k] - C.l_hoff[k - 1], C.ll_len, n0, n1, n2);
    }
}
// chm[ls] for S = 1 << ls: the chunks of the step with the most (threads 0 .. 7 of `t`)
template <int CHECKER>
__device__ __forceinline__ void bk_chunk_table(const BkCheck& C, const lds_u32* rcnt, lds_u32* chm, int t) {
    if (t < 0 || t >= 8) return;
    const int ls = t, Sg = 1 << ls;
    uint32_t mx = 0;
    for (int k = 1; k <= C.Hp; ++k) {
        int n0, n1, n2;
        bk_reach_counts<CHECKER>(C, rcnt, k, n0, n1, n2);
        const uint32_t ch = (uint32_t)(((n0 + Sg - 1) >> ls) + ((n1 + Sg - 1) >> ls) + ((n2 + Sg - 1) >> ls));
        mx = ch > mx ? ch : mx;
    }
    chm[ls] = mx;
}
template <int CHECKER, class Src>
__device__ __forceinline__ void bk_check_items(const BkCheck& C, const Src& src, volatile lds_u32* r_flag, uint32_t r0, uint32_t R, int ls, uint32_t chmax, unsigned long long pend, int tid, int nthreads) {
    const lds_u32* rcnt = BK_RCNT(bk_lds_base());
    const lds_u16* rlist = BK_RLIST(bk_lds_base());
    const uint32_t items = R * chmax;
    const int Sg = 1 << ls;
    for (uint32_t item = (uint32_t)tid; item < items; item += (uint32_t)nthreads) {
        const uint32_t c = item / R, r = r0 + (item - c * R);
        if (r_flag[r] & 1u) continue;  // collides already: the reference's early out
        uint32_t parent, packed;
        src.link(r, parent, packed);
        if (!parent) continue;  // the root has no edge (GraphSearch.m:137-139)
        const BkItemCtx I = bk_item_ctx<CHECKER>(C);
        const int k = NODE_K(packed), m = NODE_MAN(packed), ncols = NODE_COLS(packed);
        const int so = C.l_soff[k - 1], ho = C.l_hoff[k - 1];
        const int M_k = C.l_soff[k] - so;
        int n0, n1, n2;
        bk_reach_counts<CHECKER>(C, rcnt, k, n0, n1, n2);
        const uint32_t c0 = (uint32_t)((n0 + Sg - 1) >> ls), c1 = (uint32_t)((n1 + Sg - 1) >> ls), c2 = (uint32_t)((n2 + Sg - 1) >> ls);
        int base, t0, left, which = 0, lat = 0;  // (lat: where the boundary's list of this step begins, relative to the boundary)
        if (c < c0) {
            base = so;
            t0 = (int)(c << ls);
            left = n0 - t0;
        } else if (c < c0 + c1) {
            base = ho;
            t0 = (int)((c - c0) << ls);
            left = n1 - t0;
        } else if (c < c0 + c1 + c2) {
            base = I.ll_base();
            t0 = (int)((c - c0 - c1) << ls);
            left = n2 - t0;
            lat = (k - 1) * I.ll_stride();
            which = k == I.Hp() ? 2 : 1;  // large offset at k == Hp, else without offset (GraphSearch.m:161-174)
        } else {
            continue;
        }
        const int tn = left < Sg ? left : Sg;
        double cc, ss, pX, pY;
        src.pose(r, parent, pX, pY, cc, ss);
        const size_t abase = ((size_t)m * 3 + (size_t)which) * PDMPC_VMAX;
        d2 pt[PDMPC_VMAX];
        if (C.areas_in_lds) {  // (one branch around the eight loads, not a choice per load: the places are reloaded once)
#pragma unroll
            for (int i = 0; i < PDMPC_VMAX; ++i) pt[i] = I.l_area()[abase + i];
        } else {
#pragma unroll
            for (int i = 0; i < PDMPC_VMAX; ++i) pt[i] = C.g_area[abase + i];
        }
#pragma unroll
        for (int i = 0; i < PDMPC_VMAX; ++i) {  // (columns beyond ncols are padding: transformed, never used)
            const d2 a = pt[i];
            pt[i].x = cc * a.x - ss * a.y + pX;  // GraphSearch.m:158 / :162 / :168
            pt[i].y = ss * a.x + cc * a.y + pY;  // :159 / :163 / :169
        }
        if (CHECKER == PDMPC_CHECK_SAT) {
            const lds_d2* q = I.l_soup() + base + t0;
            uint32_t fnd = 0;  // 1: overlaps a real area, 2: an expected one (the slot of a predecessor that is still planning, `pend`)
            if (which == 0) {  // the polygons that begin in this chunk of the step's soup ([polygon, NaN] ..., then the predecessors' slots)
                const int lit = C.l_lit[k - 1];
                for (int t = 0; t < tn && !(fnd & 1u); ++t) {
                    const int j = t0 + t;
                    // (a predecessor's slot begins a polygon of its own: its first column follows the last column of a full slot in front of it)
                    const bool start = !is_nan(q[t].x) && (j == 0 || is_nan(C.l_soup[base + j - 1].x) || (j >= lit && ((j - lit) & (PDMPC_VMAX - 1)) == 0));
                    if (start) {
                        int e = j + 1;
                        const int lim = j >= lit ? j + PDMPC_VMAX - ((j - lit) & (PDMPC_VMAX - 1)) : M_k;  // (a slot ends with its VMAX columns)
                        while (e < lim && !is_nan(C.l_soup[base + e].x)) ++e;
                        if (sat_pair_lane(pt, ncols, C.l_soup + base + j, e - j)) {  // intersect_sat.m:1-42
                            const bool tent = j >= lit && ((pend >> ((j - lit) >> 3)) & 1ull) != 0ull;
                            fnd |= tent ? 2u : 1u;
                        }
                    }
                }
            } else {  // intersect_lanelet_boundary.m:16-54 on [left, NaN, right, NaN]
                double min_x, max_x, min_y, max_y;
                sat_area_bbox(pt, ncols, min_x, max_x, min_y, max_y);
                for (int t = 0; t < tn && !fnd; ++t) fnd = sat_boundary_segment_lane(pt, ncols, min_x, max_x, min_y, max_y, q[t], q[t + 1]) ? 1u : 0u;
            }
            if (fnd) __hip_atomic_fetch_or((lds_u32*)&r_flag[r], fnd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            continue;
        }
        // (InterX walks the chunk's entries of the soup's reach list: the segments that can decide anything)
        const lds_u16* lst = rlist + base + lat + t0;
        const lds_d2* sp = I.l_soup() + base;
        // (segments of the slots of predecessors that are still planning — `pend` — hold expected areas: a crossing there is tentative)
        const int rel0 = (which == 0 && base == so) ? -C.l_lit[k - 1] : -(1 << 20);
        uint32_t found = 0;  // 1: crosses a real area, 2: crosses an expected one
        for (int t = 0; t < tn && !(found & 1u); ++t) {
            // (the area's points are made opaque per segment: the compiler would otherwise hoist the seven edges' dx1, dy1, S1 of the
            // C1 test out of this loop — 42 registers for a test that one segment in ten reaches)
            asm volatile("" : "+v"(pt[0].x), "+v"(pt[0].y), "+v"(pt[1].x), "+v"(pt[1].y), "+v"(pt[2].x), "+v"(pt[2].y), "+v"(pt[3].x), "+v"(pt[3].y), "+v"(pt[4].x), "+v"(pt[4].y),
                         "+v"(pt[5].x), "+v"(pt[5].y), "+v"(pt[6].x), "+v"(pt[6].y), "+v"(pt[7].x), "+v"(pt[7].y));
            const int j = (int)lst[t];
            const d2 q0 = sp[j], q1 = sp[j + 1];
            if (interx_segment_n<PDMPC_VMAX>(pt, ncols - 1, q0, q1)) {
                const int rel = rel0 + j;
                const bool tent = rel >= 0 && ((pend >> (rel >> 3)) & 1ull) != 0ull;  // (rel >> 3 < 64: a search with more predecessors waits for them all)
                found |= tent ? 2u : 1u;
            }
        }
        if (found) __hip_atomic_fetch_or((lds_u32*)&r_flag[r], found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// the chunk size (as a shift) with which the check items of R entries fit the workgroup once, at most 16 segments per item
__device__ __forceinline__ int bk_chunk_shift(const lds_u32* chm, uint32_t R, uint32_t nthreads) {
    int ls = 0;
    while (ls < 4 && R * chm[ls] > nthreads) ++ls;
    return ls;
}

// position of the rk-th set bit of mask (rk < popcount)
__device__ __forceinline__ int nth_bit(uint64_t mask, int rk) {
    for (int b = 0; b < rk; ++b) mask &= mask - 1ull;
    return (int)__builtin_ctzll(mask);
}

// The areas of a result record and their column counts — all a successor reads of it (PrioritizedController.m:476-491) — go to memory
// with agent-scope stores and are read with agent-scope loads: coherent across the XCDs' L2s by themselves, without the release /
// acquire fences of rounds 2-4 (a write-back / invalidation of the whole L2).
// The records a shared round posts for its helpers and everything else owner and helpers exchange likewise go through agent-scope
// stores and loads, not plain stores behind a release fence and reads behind an acquire fence as in rounds 2-4 (every fence writes
// back / invalidates the whole L2 of its XCD: with a helper on every idle CU that is every L2 of the chip, once per round).
__device__ __forceinline__ void bk_post_store(d2* p, d2 v) {
    __hip_atomic_store((double*)p, (double)v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((double*)p + 1, (double)v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ d2 bk_post_load(const d2* p) {
    d2 v;
    v.x = __hip_atomic_load((const double*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v.y = __hip_atomic_load((const double*)p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v;
}
__device__ __forceinline__ void bk_area_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void bk_area_store_u32(int32_t* p, int v) { __hip_atomic_store(p, (int32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double bk_area_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int bk_area_load_i32(const int32_t* p) { return (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// incorporate_areas with loads that are coherent by themselves (bk_area_load): the solved areas of the predecessors in `arr` into
// their soup slots (PrioritizedController.m:476-491); nthreads threads call (a workgroup, or one wave).
// (chg, when given: [Hp] 64-bit masks — bit p of chg[k] is set when the area predecessor p publishes for step k + 1 differs from what
// its slot held, i.e. from the area it was expected to take.  A collision-free edge of that step has been checked against exactly
// those numbers: only the pairs (step, predecessor) marked here are due for the re-check, bk_recheck_items.
// rbox, when given (InterX): the rectangles of the steps with the root behind them, include/pdmpc_reach.h — an area none of whose segments is in reach of its step
// cannot take an edge of that step away, whatever the slot held: its bit is not set.  The two ballots and the __shfl_down sit in a
// loop whose last trip is partial, i.e. with some lanes of the wavefront switched off.  That is safe because an area's eight columns
// never straddle the boundary between active and inactive lanes: idx = tid + trip * nthreads with nthreads a multiple of 64 (the
// workgroup, or the one wavefront of bk_wait_done) and the item count n_arr * Hp * VMAX a multiple of 8, so the columns v = 0 .. 7 of
// one area are eight consecutive lanes of one wavefront, aligned to 8, and all of them are in the loop or none is: a ballot's byte g
// holds exactly that area's columns, and lane v < 7 shuffles from a lane of its own group.)
__device__ __forceinline__ void bk_incorporate(const pdmpc_vehicle_out* out, const int32_t* pred, lds_d2* l_soup, const lds_i32* l_soff, const lds_i32* l_lit, int Hp, unsigned long long arr, int tid,
                                               int nthreads, lds_u64s* chg, const lds_f64* rbox) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const int per = Hp * PDMPC_VMAX, n_arr = __builtin_popcountll(arr);
    for (int idx = tid; idx < n_arr * per; idx += nthreads) {  // (every arrived predecessor's loads side by side)
        const int a = idx / per, rest = idx - a * per;
        const int p = nth_bit(arr, a);
        const pdmpc_vehicle_out* PO = out + pred[p];
        const int k = rest / PDMPC_VMAX, v = rest - k * PDMPC_VMAX;
        const int cols = bk_area_load_i32(&PO->shape_cols[k]);
        const double sx = bk_area_load(&PO->shapes[k][0][v]), sy = bk_area_load(&PO->shapes[k][1][v]);
        d2 pt;
        pt.x = v < cols ? sx : qnan;
        pt.y = v < cols ? sy : qnan;
        lds_d2* slot = l_soup + l_soff[k] + l_lit[k] + p * PDMPC_VMAX + v;
        if (chg) {
            const d2 was = *slot;
            const bool differs = __double_as_longlong(was.x) != __double_as_longlong(pt.x) || __double_as_longlong(was.y) != __double_as_longlong(pt.y);
            if (rbox) {
                const double nx = __shfl_down(pt.x, 1), ny = __shfl_down(pt.y, 1);  // (column v + 1: the same area for v < VMAX - 1)
                const lds_f64* root = rbox + (PDMPC_LK_REACH_ROOT >> 3);
                const bool in = v + 1 < PDMPC_VMAX && pdmpc_reach_in_oriented(pt.x, pt.y, nx, ny, root[0], root[1], root[2], root[3], rbox[4 * k], rbox[4 * k + 1], rbox[4 * k + 2], rbox[4 * k + 3]) != 0;
                const int g = (tid & (PDMPC_WAVE - 1)) & ~(PDMPC_VMAX - 1);
                const unsigned long long md = __ballot(differs), mi = __ballot(in);
                if (v == 0 && ((md >> g) & 0xffull) != 0ull && ((mi >> g) & 0xffull) != 0ull)
                    __hip_atomic_fetch_or(chg + k, 1ull << p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else if (differs) {
                __hip_atomic_fetch_or(chg + k, 1ull << p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        *slot = pt;
    }
}

}  // namespace
