// hdv_kernel.hip — human-driven vehicles on the device (HighLevelController.update_hdv_traffic_info, HighLevelController.m:394-447, with
// the semantics of DESIGN.md §3.24), f64 throughout.  One call is four launches on one stream:
//
//   closest    one wavefront per HDV: lanes over the lanelets (pdmpc_hdv_lanelet_distance, the distances in LDS), then lane 0 runs the
//              order-dependent scan (pdmpc_hdv_closest_scan) and lists the chains (pdmpc_hdv_list_chains)
//   lane       one wavefront per (HDV, chain, step): K (the trim's step hull moved to the HDV's pose) and the raw chain polygon in LDS,
//              lane 0 normalizes it, lanes clip its edges against K (pdmpc_clip_edge_t), lane 0 builds the kept region in the slot
//              (pdmpc_bound_region: the rule of bounded_kernel.hip, not a copy of it); an empty K ∩ L is a polygon of 0 vertices
//   pack       one wavefront per slot: where its polygon starts in the caller's layout is the sum of the vertex counts of the slots in
//              front of it (integers, summed across the lanes), then the lanes copy the vertices, none at or beyond the capacity
//   adjacency  one lane per (CAV, HDV) pair (pdmpc_hdv_is_behind)
// The host twin (hdv.cpp) runs the same header functions, so lists, rows, vertices, flags and adjacency are bit-identical.  Every
// output entry is written by exactly one lane.
//
// The grouped call (pdmpc_hdv_traffic_grouped: several independent sets of HDVs and CAVs, each on one of the handle's resident maps) is
// five launches whatever the number of groups.  Its closest, lane and adjacency passes run the same per-item bodies (hdv_closest_item,
// hdv_lane_item, hdv_adjacency_item) on the item's own map, read from the handle's table of map records; packing is
//   scan       ONE workgroup of PDMPC_HDV_SCAN_BLOCK lanes walks the slots in order, a tile of PDMPC_HDV_SCAN_BLOCK at a time: an
//              inclusive prefix sum of the vertex counts per wavefront (__shfl_up), the wavefronts' totals through LDS, a carry from
//              tile to tile; a slot's place is that sum less the sum at its group's first slot.  Also the rows in front of every HDV,
//              the rows and the vertex base of every group, and the status words
//   copy       one wavefront per slot that exists: its offset, flags and row, and its vertices, none at or beyond the capacity
// so a slot's count is read twice, not once per slot behind it.
//
// The drive pass (pdmpc_hdv_drive_kernel, further down: the driver model of include/pdmpc_hdv.h) moves the HDVs of a grouped call one step
// along their routes; alone it is pdmpc_hdv_drive_grouped, in front of the five passes pdmpc_hdv_drive_traffic_grouped: six launches.
#include <hip/hip_runtime.h>

#include "../../include/pdmpc_geometry.h"
#include "pdmpc_device.h"

namespace {
// the chains of HDV h that exist and fit: 0 for an HDV whose lists ran over (the call fails; nothing of it is computed)
__device__ inline int hdv_chains(const HdvArgs& A, int h) {
    const int nc = A.n_chains[h];
    return A.n_closest[h] > PDMPC_HDV_MAX_CHAINS || nc > PDMPC_HDV_MAX_CHAINS ? 0 : nc;
}
// the sum of v over the wavefront's 64 lanes, in every lane
__device__ inline int wave_sum(int v) {
    for (int o = PDMPC_HDV_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- the per-item bodies, shared by the kernels of the ungrouped and of the grouped call: the work arrays are A's (over all HDVs and
// CAVs of the call), the map and the hulls are the item's own

// HDV h (a wavefront; d: PDMPC_HDV_MAX_LANELETS distances in LDS): its closest lanelets and its chains
__device__ inline void hdv_closest_item(const HdvArgs& A, const pdmpc_hdv_map* M, int h, int lane, double* d) {
    const int n = A.n_hdv, nl = M->n_lanelets;
    const double px = A.in[h] - A.in[4 * n + h], py = A.in[n + h] - A.in[5 * n + h];
    for (int i = lane; i < nl; i += PDMPC_HDV_WAVE) d[i] = pdmpc_hdv_lanelet_distance(M, i, px, py);
    __syncthreads();
    if (lane != 0) return;
    int32_t* list = A.closest + (size_t)h * PDMPC_HDV_MAX_CHAINS;
    const int n_list = pdmpc_hdv_closest_scan(d, nl, list, PDMPC_HDV_MAX_CHAINS);
    A.n_closest[h] = n_list;
    const int kept = n_list < PDMPC_HDV_MAX_CHAINS ? n_list : PDMPC_HDV_MAX_CHAINS;
    A.n_chains[h] = pdmpc_hdv_list_chains(M, list, kept, A.chain_id + (size_t)h * PDMPC_HDV_MAX_CHAINS, A.chain_succ + (size_t)h * PDMPC_HDV_MAX_CHAINS,
                                          PDMPC_HDV_MAX_CHAINS);
}

// the LDS of the lane pass's workgroup (48 KB: three workgroups per CU)
struct HdvLaneLds {
    double kx[PDMPC_REACH_MAX_COLS], ky[PDMPC_REACH_MAX_COLS];
    double rawx[PDMPC_BOUND_LANELET_MAX], rawy[PDMPC_BOUND_LANELET_MAX];
    double lx[PDMPC_BOUND_LANELET_MAX], ly[PDMPC_BOUND_LANELET_MAX], tmn[PDMPC_BOUND_LANELET_MAX], tmx[PDMPC_BOUND_LANELET_MAX];
    int ci[6 * PDMPC_BOUND_LANELET_MAX];
    double cd[2 * PDMPC_BOUND_LANELET_MAX];
    int nl_shared;
};
// slot (h PDMPC_HDV_MAX_CHAINS + c) Hp + k (a wavefront): the reachable lane of HDV h's chain c at step k into the slot
__device__ inline void hdv_lane_item(const HdvArgs& A, const pdmpc_hdv_map* M, const double* local_x, const double* local_y, const int32_t* local_off, int slot, int lane,
                                     HdvLaneLds& S) {
    const int n = A.n_hdv, Hp = A.Hp;
    const int hc = slot / Hp, k = slot - hc * Hp;
    const int h = hc / PDMPC_HDV_MAX_CHAINS, c = hc - h * PDMPC_HDV_MAX_CHAINS;
    if (c >= hdv_chains(A, h)) return;  // (the whole wavefront: no barrier is left behind)
    const int id = A.chain_id[hc], succ = A.chain_succ[hc];
    const int nr = pdmpc_hdv_chain_vertices(M, id, succ);  // (<= PDMPC_BOUND_LANELET_MAX: checked at the upload)
    const double dx = A.in[4 * n + h], dy = A.in[5 * n + h];
    for (int r = lane; r < nr; r += PDMPC_HDV_WAVE) pdmpc_hdv_chain_vertex(M, id, succ, dx, dy, r, &S.rawx[r], &S.rawy[r]);
    const int p = A.trim[h] * Hp + k;
    const int a = local_off[p], m = local_off[p + 1] - a;  // (<= PDMPC_REACH_MAX_COLS: checked at the upload)
    const double x0 = A.in[h], y0 = A.in[n + h], cs = A.in[2 * n + h], sn = A.in[3 * n + h];
    for (int r = lane; r < m; r += PDMPC_HDV_WAVE) pdmpc_move_point(cs, sn, x0, y0, local_x[a + r], local_y[a + r], &S.kx[r], &S.ky[r]);
    __syncthreads();
    if (lane == 0) S.nl_shared = pdmpc_lanelet_polygon_normalize(S.rawx, S.rawy, nr, S.lx, S.ly);
    __syncthreads();
    const int nl = S.nl_shared;
    if (nl >= 3 && m >= 3)
        for (int e = lane; e < nl; e += PDMPC_HDV_WAVE) {
            const int e1 = e + 1 == nl ? 0 : e + 1;
            pdmpc_clip_edge_t(S.lx[e], S.ly[e], S.lx[e1], S.ly[e1], S.kx, S.ky, m, &S.tmn[e], &S.tmx[e]);
        }
    __syncthreads();
    if (lane != 0) return;
    pdmpc_bound_chains C;
    C.start = S.ci;
    C.end = S.ci + PDMPC_BOUND_LANELET_MAX;
    C.kin = S.ci + 2 * PDMPC_BOUND_LANELET_MAX;
    C.kout = S.ci + 3 * PDMPC_BOUND_LANELET_MAX;
    C.next = S.ci + 4 * PDMPC_BOUND_LANELET_MAX;
    C.region = S.ci + 5 * PDMPC_BOUND_LANELET_MAX;
    C.sin = S.cd;
    C.sout = S.cd + PDMPC_BOUND_LANELET_MAX;
    int cnt = 0;
    unsigned fl = 0u;
    const int over = pdmpc_bound_region(S.kx, S.ky, m, S.lx, S.ly, nl, S.tmn, S.tmx, &C, A.slot_x + (size_t)slot * PDMPC_BOUND_SLOT, A.slot_y + (size_t)slot * PDMPC_BOUND_SLOT, PDMPC_BOUND_SLOT, &cnt, &fl);
    const int empty = (fl & PDMPC_BOUND_RESTORED) != 0u;  // K ∩ L is empty: 0 vertices (HighLevelController.m:416-419), not K
    A.slot_n[slot] = empty ? 0 : cnt;
    A.slot_flags[slot] = (uint8_t)(fl | (over && !empty ? PDMPC_BOUND_OVERFLOW : 0u));
}

// CAV v and HDV h (a lane) -> 1 unless they drive on different copies of the map or the HDV is behind the CAV
__device__ inline int hdv_adjacency_item(const HdvArgs& A, const pdmpc_hdv_map* M, int v, int h) {
    const int n = A.n_hdv, nc = A.n_cav;
    if (!(A.cav[2 * nc + v] == A.in[4 * n + h] && A.cav[3 * nc + v] == A.in[5 * n + h])) return 0;
    const int n_list = A.n_closest[h] < PDMPC_HDV_MAX_CHAINS ? A.n_closest[h] : PDMPC_HDV_MAX_CHAINS;
    return !pdmpc_hdv_is_behind(M, A.cav_lanelet[v], A.cav[v], A.cav[nc + v], A.closest + (size_t)h * PDMPC_HDV_MAX_CHAINS, n_list, A.in[h], A.in[n + h], A.in[2 * n + h],
                                A.in[3 * n + h]);
}

// the polygon of slot (cnt vertices as the lane pass counted them) to first .. of the call's vertices, none at or beyond the capacity
__device__ inline void hdv_copy_slot(const HdvArgs& A, int slot, int cnt, int first, int lane) {
    const int fits = cnt < PDMPC_BOUND_SLOT ? cnt : PDMPC_BOUND_SLOT;  // (an overflowed slot holds no more; the call fails)
    const double* sx = A.slot_x + (size_t)slot * PDMPC_BOUND_SLOT;
    const double* sy = A.slot_y + (size_t)slot * PDMPC_BOUND_SLOT;
    for (int r = lane; r < fits; r += PDMPC_HDV_WAVE)
        if (first + r < A.capacity) {
            A.set_x[first + r] = sx[r];
            A.set_y[first + r] = sy[r];
        }
}
}  // namespace

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_closest_kernel(const HdvArgs A) {
    __shared__ double d[PDMPC_HDV_MAX_LANELETS];
    hdv_closest_item(A, &A.map, (int)blockIdx.x, (int)threadIdx.x, d);
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_lane_kernel(const HdvArgs A) {
    __shared__ HdvLaneLds S;
    hdv_lane_item(A, &A.map, A.local_x, A.local_y, A.local_off, (int)blockIdx.x, (int)threadIdx.x, S);
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_pack_kernel(const HdvArgs A) {
    const int slot = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int n = A.n_hdv, Hp = A.Hp, per_hdv = PDMPC_HDV_MAX_CHAINS * Hp;
    const int hc = slot / Hp, k = slot - hc * Hp;
    const int h = hc / PDMPC_HDV_MAX_CHAINS, c = hc - h * PDMPC_HDV_MAX_CHAINS;
    const bool mine = c < hdv_chains(A, h);
    if (!mine && slot != 0) return;
    // the rows and vertices in front of this slot; workgroup 0 also adds up all of them and the status of the call.  Every workgroup sums
    // for itself, so the pass reads S (S - 1) / 2 counts for S slots: S <= PDMPC_HDV_MAX_VEHICLES * PDMPC_HDV_MAX_CHAINS * Hp, 256 at
    // 2 HDVs and Hp 8 (32 640 reads), 16 384 at the limits (1.3e8 reads of 64 KB that stay in L2).  The grouped call scans instead
    // (pdmpc_hdv_scan_kernel).
    const int end = slot == 0 ? n * per_hdv : slot;
    int rows = 0, before = 0, all_rows = 0, all = 0, status = 0;
    for (int g = lane; g < n; g += PDMPC_HDV_WAVE) {
        const int nc = hdv_chains(A, g);
        if (g < h) rows += nc;
        all_rows += nc;
        if (A.n_closest[g] > PDMPC_HDV_MAX_CHAINS || A.n_chains[g] > PDMPC_HDV_MAX_CHAINS) status |= PDMPC_HDV_OVER_LISTS;
    }
    for (int j = lane; j < end; j += PDMPC_HDV_WAVE) {
        const int jhc = j / Hp, jh = jhc / PDMPC_HDV_MAX_CHAINS, jc = jhc - jh * PDMPC_HDV_MAX_CHAINS;
        if (jc >= hdv_chains(A, jh)) continue;
        const int cnt = A.slot_n[j];
        if (j < slot) before += cnt;
        all += cnt;
        if (A.slot_flags[j] & PDMPC_BOUND_OVERFLOW) status |= PDMPC_HDV_OVER_SLOT;
    }
    rows = wave_sum(rows);
    before = wave_sum(before);
    if (slot == 0) {
        all_rows = wave_sum(all_rows);
        all = wave_sum(all);
        const int lists = wave_sum(status & PDMPC_HDV_OVER_LISTS ? 1 : 0), slots = wave_sum(status & PDMPC_HDV_OVER_SLOT ? 1 : 0);
        if (lane == 0) {
            A.status[0] = all_rows;
            A.status[1] = (lists ? PDMPC_HDV_OVER_LISTS : 0) | (slots ? PDMPC_HDV_OVER_SLOT : 0);
            A.set_off[all_rows * Hp] = all;
        }
    }
    if (!mine) return;
    const int row = rows + c, set = row * Hp + k;
    const int cnt = A.slot_n[slot];
    if (lane == 0) {
        A.set_off[set] = before;
        A.set_flags[set] = (uint8_t)(A.slot_flags[slot] & (PDMPC_BOUND_RESTORED | PDMPC_BOUND_MULTIPLE));
        if (k == 0) A.row_hdv[row] = h;
    }
    hdv_copy_slot(A, slot, cnt, before, lane);
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_adjacency_kernel(const HdvArgs A) {
    const int n = A.n_hdv, nc = A.n_cav;
    const int item = (int)blockIdx.x * PDMPC_HDV_WAVE + (int)threadIdx.x;
    if (item >= nc * n) return;
    const int v = item / n, h = item - v * n;
    A.adjacency[item] = (uint8_t)hdv_adjacency_item(A, &A.map, v, h);
}

// ---- the grouped call

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_closest_grouped_kernel(const HdvGroupedArgs G) {
    __shared__ double d[PDMPC_HDV_MAX_LANELETS];
    const int h = (int)blockIdx.x;
    const HdvMapRecord* R = G.maps + G.groups[G.group_of[h]].slot;
    hdv_closest_item(G.a, &R->map, h, (int)threadIdx.x, d);
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_lane_grouped_kernel(const HdvGroupedArgs G) {
    __shared__ HdvLaneLds S;
    const int slot = (int)blockIdx.x;
    const int hc = slot / G.a.Hp, h = hc / PDMPC_HDV_MAX_CHAINS;
    // (a slot of a chain that does not exist leaves before its map is looked up)
    if (hc - h * PDMPC_HDV_MAX_CHAINS >= hdv_chains(G.a, h)) return;
    const HdvMapRecord* R = G.maps + G.groups[G.group_of[h]].slot;
    hdv_lane_item(G.a, &R->map, R->local_x, R->local_y, R->local_off, slot, (int)threadIdx.x, S);
}

// One workgroup.  (1) a lane per group walks the group's HDVs: the rows in front of each (row_base), the group's rows, -1 if an HDV of
// it ran over its lists -- such a group is dead: its slots count as not there.  (2) the tiles of slots in order: the number of vertices
// in front of every slot among ALL slots that exist (wavefront prefix sums, the wavefronts' totals in LDS, the carry of the tiles
// before); the lane at a group's first slot notes it as the group's set_base, and less that note it is the slot's place within its
// group (slot_before).  (3) one lane walks the groups back to front: set_base of the groups without HDVs (where the next group
// starts), the last entry of every group's offsets, the status words.  What one lane writes to global memory and another reads
// (n_rows, set_base) is a barrier apart.  All sums are integers: any association gives the same bits.
extern "C" __global__ __launch_bounds__(PDMPC_HDV_SCAN_BLOCK) void pdmpc_hdv_scan_kernel(const HdvGroupedArgs G) {
    constexpr int WAVES = PDMPC_HDV_SCAN_BLOCK / PDMPC_HDV_WAVE;
    __shared__ int wave_total[WAVES];
    __shared__ int over[2];  // lists, slots
    const HdvArgs& A = G.a;
    const int t = (int)threadIdx.x, lane = t % PDMPC_HDV_WAVE, wave = t / PDMPC_HDV_WAVE;
    const int Hp = A.Hp, per_hdv = PDMPC_HDV_MAX_CHAINS * Hp, S = A.n_hdv * per_hdv;
    if (t < 2) over[t] = 0;
    __syncthreads();
    // (1)
    for (int g = t; g < G.n_groups; g += PDMPC_HDV_SCAN_BLOCK) {
        const HdvGroup grp = G.groups[g];
        int rows = 0, dead = 0;
        for (int h = grp.h0; h < grp.h0 + grp.n_hdv; ++h) {
            G.row_base[h] = rows;
            rows += hdv_chains(A, h);
            if (A.n_closest[h] > PDMPC_HDV_MAX_CHAINS || A.n_chains[h] > PDMPC_HDV_MAX_CHAINS) dead = 1;
        }
        G.n_rows[g] = dead ? -1 : rows;
        if (dead) over[0] = 1;  // (every writer writes 1)
    }
    __syncthreads();
    // (2)
    int carry = 0;
    for (int base = 0; base < S; base += PDMPC_HDV_SCAN_BLOCK) {
        const int j = base + t;
        int cnt = 0, g = 0;
        bool there = false, first = false;
        if (j < S) {
            const int jhc = j / Hp, jh = jhc / PDMPC_HDV_MAX_CHAINS, jc = jhc - jh * PDMPC_HDV_MAX_CHAINS;
            g = G.group_of[jh];
            first = j == G.groups[g].h0 * per_hdv;
            there = G.n_rows[g] >= 0 && jc < hdv_chains(A, jh);
            if (there) {
                cnt = A.slot_n[j];
                if (A.slot_flags[j] & PDMPC_BOUND_OVERFLOW) over[1] = 1;
            }
        }
        int incl = cnt;
        for (int o = 1; o < PDMPC_HDV_WAVE; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == PDMPC_HDV_WAVE - 1) wave_total[wave] = incl;
        __syncthreads();
        int before = carry + incl - cnt, tile = 0;
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) before += wave_total[w];
            tile += wave_total[w];
        }
        if (first) G.set_base[g] = before;
        __syncthreads();  // (the groups' notes are there; wave_total may be written again)
        if (there) G.slot_before[j] = before - G.set_base[g];
        carry += tile;
    }
    __syncthreads();
    // (3)
    if (t != 0) return;
    int next = carry;
    G.set_base[G.n_groups] = carry;
    for (int g = G.n_groups - 1; g >= 0; --g) {
        const HdvGroup grp = G.groups[g];
        if (grp.n_hdv == 0) G.set_base[g] = next;
        const int start = G.set_base[g];
        const int rows = G.n_rows[g] > 0 ? G.n_rows[g] : 0;
        A.set_off[(size_t)grp.h0 * per_hdv + g + (size_t)rows * Hp] = next - start;
        next = start;
    }
    A.status[0] = carry;
    A.status[1] = (over[0] ? PDMPC_HDV_OVER_LISTS : 0) | (over[1] ? PDMPC_HDV_OVER_SLOT : 0);
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_copy_kernel(const HdvGroupedArgs G) {
    const HdvArgs& A = G.a;
    const int slot = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int Hp = A.Hp, per_hdv = PDMPC_HDV_MAX_CHAINS * Hp;
    const int hc = slot / Hp, k = slot - hc * Hp;
    const int h = hc / PDMPC_HDV_MAX_CHAINS, c = hc - h * PDMPC_HDV_MAX_CHAINS;
    const int g = G.group_of[h];
    if (G.n_rows[g] < 0 || c >= hdv_chains(A, h)) return;
    const int h0 = G.groups[g].h0;
    const int row = G.row_base[h] + c, set = row * Hp + k;
    const int cnt = A.slot_n[slot], before = G.slot_before[slot];
    if (lane == 0) {
        A.set_off[(size_t)h0 * per_hdv + g + set] = before;
        A.set_flags[(size_t)h0 * per_hdv + set] = (uint8_t)(A.slot_flags[slot] & (PDMPC_BOUND_RESTORED | PDMPC_BOUND_MULTIPLE));
        if (k == 0) A.row_hdv[(size_t)h0 * PDMPC_HDV_MAX_CHAINS + row] = h - h0;
    }
    hdv_copy_slot(A, slot, cnt, G.set_base[g] + before, lane);
}

extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_adjacency_grouped_kernel(const HdvGroupedArgs G) {
    const int item = (int)blockIdx.x * PDMPC_HDV_WAVE + (int)threadIdx.x;
    if (item >= G.pair_first[G.n_groups]) return;
    int lo = 0, hi = G.n_groups;  // the last group whose first pair is not behind the item (groups without pairs share a first pair: the last of them owns it)
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (G.pair_first[mid] <= item)
            lo = mid;
        else
            hi = mid;
    }
    const HdvGroup grp = G.groups[lo];
    const int local = item - G.pair_first[lo];
    const int v = local / grp.n_hdv, h = local - v * grp.n_hdv;
    G.a.adjacency[item] = (uint8_t)hdv_adjacency_item(G.a, &G.maps[grp.slot].map, grp.c0 + v, grp.h0 + h);
}

// ---- the drive pass (include/pdmpc_hdv.h: the driver model).  One wavefront per HDV h of the call.  The lanes compute where the HDVs of
// h's group stand BEFORE the step (from the old states: nothing this launch writes is read by it); lane 0 lists the window in LDS; the
// lanes stride over the (other vehicle, window segment) items -- the group's CAVs first, then its other HDVs -- and the smallest
// distance ahead is taken across the wavefront (a minimum of doubles without NaN: any order gives the same bits); lane 0 moves the HDV
// and writes its state, speed, gap and pose.  hdv_drive_host.hpp: hdv_drive_member is the same step on the host.
extern "C" __global__ __launch_bounds__(PDMPC_HDV_WAVE) void pdmpc_hdv_drive_kernel(const HdvDriveArgs D) {
    __shared__ pdmpc_hdv_window W;
    __shared__ double ox[PDMPC_HDV_MAX_VEHICLES], oy[PDMPC_HDV_MAX_VEHICLES];
    __shared__ int nw_shared;
    const int h = (int)blockIdx.x, lane = (int)threadIdx.x, n = D.n_hdv, nc = D.n_cav;
    const int g = D.group_of[h];
    if (!D.drives[g]) return;  // (the whole wavefront)
    const HdvGroup grp = D.groups[g];
    const pdmpc_hdv_map* M = &D.maps[grp.slot].map;
    const double* P = D.params + (size_t)g * PDMPC_HDV_DRIVE_PARAMS;
    const double tdx = D.in[4 * n + h], tdy = D.in[5 * n + h];
    for (int q = lane; q < grp.n_hdv; q += PDMPC_HDV_WAVE) {  // (n_hdv <= PDMPC_HDV_MAX_VEHICLES: checked by the call)
        const int o = grp.h0 + q;
        const pdmpc_hdv_route R{D.route_id + D.route_off[o], D.route_off[o + 1] - D.route_off[o], D.closed[o] ? 1 : 0};
        const pdmpc_hdv_drive_state S{D.state_seg[o], D.state_seg[n + o], D.state_u[o]};
        double c, s;
        pdmpc_hdv_state_pose(M, &R, &S, D.in[4 * n + o], D.in[5 * n + o], &ox[q], &oy[q], &c, &s);
    }
    const pdmpc_hdv_route R{D.route_id + D.route_off[h], D.route_off[h + 1] - D.route_off[h], D.closed[h] ? 1 : 0};
    pdmpc_hdv_drive_state S{D.state_seg[h], D.state_seg[n + h], D.state_u[h]};
    if (lane == 0) nw_shared = pdmpc_hdv_build_window(M, &R, &S, P[0], &W);
    __syncthreads();
    const int nw = nw_shared, items = (grp.n_cav + grp.n_hdv) * nw;  // (<= (2^20 + 64) 64 < 2^31)
    double best = (double)INFINITY;
    for (int it = lane; it < items; it += PDMPC_HDV_WAVE) {
        const int o = it / nw, w = it - o * nw;
        double px, py, odx, ody;
        if (o < grp.n_cav) {
            const int v = grp.c0 + o;
            px = D.cav[v];
            py = D.cav[nc + v];
            odx = D.cav[2 * nc + v];
            ody = D.cav[3 * nc + v];
        } else {
            const int q = o - grp.n_cav;
            if (grp.h0 + q == h) continue;
            px = ox[q];
            py = oy[q];
            odx = D.in[4 * n + grp.h0 + q];
            ody = D.in[5 * n + grp.h0 + q];
        }
        if (!(odx == tdx && ody == tdy)) continue;
        const double ahead = pdmpc_hdv_gap_item(&W, w, S.u, px - tdx, py - tdy, P[3]);
        if (ahead < best) best = ahead;
    }
    for (int o = PDMPC_HDV_WAVE / 2; o > 0; o >>= 1) {
        const double other = __shfl_xor(best, o);
        if (other < best) best = other;
    }
    if (lane != 0) return;
    D.gap[h] = best;
    D.speed[h] = pdmpc_hdv_move(M, &R, &S, best, D.v_des[h], P, P[4]);
    D.new_seg[h] = S.r;
    D.new_seg[n + h] = S.j;
    D.new_u[h] = S.u;
    double x, y, c, s;
    pdmpc_hdv_state_pose(M, &R, &S, tdx, tdy, &x, &y, &c, &s);
    const double pose[4] = {x, y, c, s};
    for (int q = 0; q < 4; ++q) D.in[q * n + h] = D.pose[q * n + h] = pose[q];
}

extern "C" int pdmpc_launch_hdv_drive(const HdvDriveArgs* args, void* stream) {
    if (args->n_hdv <= 0) return 0;
    hipLaunchKernelGGL(pdmpc_hdv_drive_kernel, dim3((uint32_t)args->n_hdv), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_hdv_traffic(const HdvArgs* args, void* stream) {
    const int n = args->n_hdv;
    if (n <= 0) return 0;
    const uint32_t slots = (uint32_t)n * PDMPC_HDV_MAX_CHAINS * (uint32_t)args->Hp;
    hipLaunchKernelGGL(pdmpc_hdv_closest_kernel, dim3((uint32_t)n), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    hipLaunchKernelGGL(pdmpc_hdv_lane_kernel, dim3(slots), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    hipLaunchKernelGGL(pdmpc_hdv_pack_kernel, dim3(slots), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    if (args->n_cav > 0) {
        const uint32_t blocks = (uint32_t)(((long long)args->n_cav * n + PDMPC_HDV_WAVE - 1) / PDMPC_HDV_WAVE);
        hipLaunchKernelGGL(pdmpc_hdv_adjacency_kernel, dim3(blocks), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    }
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_hdv_traffic_grouped(const HdvGroupedArgs* args, void* stream) {
    const int n = args->a.n_hdv;
    if (n <= 0) return 0;
    const uint32_t slots = (uint32_t)n * PDMPC_HDV_MAX_CHAINS * (uint32_t)args->a.Hp;
    hipLaunchKernelGGL(pdmpc_hdv_closest_grouped_kernel, dim3((uint32_t)n), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    hipLaunchKernelGGL(pdmpc_hdv_lane_grouped_kernel, dim3(slots), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    hipLaunchKernelGGL(pdmpc_hdv_scan_kernel, dim3(1), dim3(PDMPC_HDV_SCAN_BLOCK), 0, (hipStream_t)stream, *args);
    hipLaunchKernelGGL(pdmpc_hdv_copy_kernel, dim3(slots), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    if (args->n_pairs > 0) {
        const uint32_t blocks = (uint32_t)(((long long)args->n_pairs + PDMPC_HDV_WAVE - 1) / PDMPC_HDV_WAVE);
        hipLaunchKernelGGL(pdmpc_hdv_adjacency_grouped_kernel, dim3(blocks), dim3(PDMPC_HDV_WAVE), 0, (hipStream_t)stream, *args);
    }
    return (int)hipGetLastError();
}

extern "C" int pdmpc_launch_hdv_drive_traffic_grouped(const HdvDriveTrafficArgs* args, void* stream) {
    if (const int rc = pdmpc_launch_hdv_drive(&args->d, stream)) return rc;
    return pdmpc_launch_hdv_traffic_grouped(&args->g, stream);
}
