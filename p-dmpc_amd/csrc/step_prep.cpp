// step_prep.cpp — the step-preparation calls of the C ABI: device work that runs once per time step before the searches are packed
// (unique prioritizations, reachable-set coupling, lanelet bounding and the coupling on the bounded sets, future collision assessment,
// HDV traffic and the HDV drivers' step in front of it).
//
// Every call but pdmpc_unique_priorities(_grouped) follows one recipe: carve ONE pinned staging block and ONE device workspace with the same
// offsets (Carver, carver.hpp), stage the inputs, copy them in once, launch between an event pair (timed_launch), copy the result back, synchronise.
#include <atomic>

#include "handle.hpp"
#include "hdv_call_host.hpp"

#include "../../include/pdmpc_geometry.h"

namespace {

// one kernel launch between t's events, created on first use (t.fold() after the caller's synchronise)
template <class Args>
int timed_launch(pdmpc_handle* h, TimedLaunch& t, int (*launch)(const Args*, void*), const Args& a, const char* what) {
    for (hipEvent_t& e : t.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(t.ev[0], h->stream));
    const int lrc = launch(&a, (void*)h->stream);
    if (lrc) return fail(PDMPC_ERR_HIP, std::string(what) + " kernel launch failed: " + hipGetErrorString((hipError_t)lrc));
    HIPCHK(hipEventRecord(t.ev[1], h->stream));
    return PDMPC_OK;
}

// what a coupler writes: adjacency [n x n] (8-aligned), then areas [n x n]; a grouped call fills the first sum n_g^2 entries of both
struct PairOut {
    size_t adj, area;
};
PairOut carve_pair_out(Carver& c, int n) {
    PairOut o;
    o.adj = c.take<uint8_t>((size_t)n * n, 8);
    o.area = c.take<double>((size_t)n * n);
    return o;
}
// ... read back through `pinned` (nn entries; the areas only when asked for) after t's launch; synchronises the stream
int fetch_pair_out(pdmpc_handle* h, TimedLaunch& t, const unsigned char* dev, unsigned char* pinned, const PairOut& o, size_t nn, uint8_t* adjacency, double* area) {
    const size_t bytes = area ? o.area - o.adj + nn * sizeof(double) : nn;
    HIPCHK(hipMemcpyAsync(pinned, dev + o.adj, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    t.fold();
    std::memcpy(adjacency, pinned, nn);
    if (area) std::memcpy(area, pinned + (o.area - o.adj), nn * sizeof(double));
    return PDMPC_OK;
}

// The groups of a grouped coupler call as the kernels read them: one PairGroup per vehicle.  Returns the number of result entries
// (sum n_g^2) and the largest group, or an error for offsets that do not start at 0 or decrease.
int check_groups(const char* who, int32_t n_groups, const int32_t* group_offset, int* n_out) {
    if (n_groups < 0 || !group_offset || group_offset[0] != 0) return fail(PDMPC_ERR_INVALID, std::string(who) + ": bad groups");
    for (int g = 0; g < n_groups; ++g)
        if (group_offset[g + 1] < group_offset[g]) return fail(PDMPC_ERR_INVALID, std::string(who) + ": group offsets decrease");
    *n_out = group_offset[n_groups];
    return PDMPC_OK;
}
size_t stage_groups(PairGroup* pg, int32_t n_groups, const int32_t* group_offset, int* max_group) {
    size_t block = 0;
    *max_group = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int a = group_offset[g], b = group_offset[g + 1];
        for (int v = a; v < b; ++v) pg[v] = PairGroup{a, b, (int32_t)block};
        block += (size_t)(b - a) * (b - a);
        *max_group = std::max(*max_group, b - a);
    }
    return block;
}

// ---- Prioritizer.unique_priorities (Prioritizer.m:97-140) on the device: priority_kernel.hip.  The acyclic orientations are counted
// first; the true count K is reported whatever max_out is, and only a K that fits is written (never a truncated list).
// E of find(triu(adjacency, 1))
int count_edges(int n, const uint8_t* adjacency) {
    int E = 0;
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < c; ++r)
            if (adjacency[(size_t)r * n + c]) ++E;
    return E;
}
// a graph within the limits (n <= PDMPC_PRIO_MAX_N, E <= PDMPC_PRIO_MAX_E) as the kernels read it -> its tiles
int64_t stage_graph(PriorityArgs& A, int n, int E, const uint8_t* adjacency) {
    std::memset(&A, 0, sizeof A);
    A.n = n;
    for (int c = 0, e = 0; c < n; ++c)  // find(triu(adjacency, 1)): by column, then by row
        for (int r = 0; r < c; ++r)
            if (adjacency[(size_t)r * n + c]) {
                const uint32_t bit = 1u << (E - 1 - e);  // dec2bin(m, E): edge 1 is the most significant bit
                A.in_base[c] |= bit;
                A.out_base[r] |= bit;
                ++e;
            }
    for (int v = 0; v < n; ++v)
        if (A.in_base[v] | A.out_base[v]) A.active[A.n_active++] = v;
    A.E = E;
    A.all_edges = E == 32 ? 0xffffffffu : (1u << E) - 1u;
    A.n_masks = 1ull << E;
    return (int64_t)((A.n_masks + PDMPC_PRIO_TILE - 1) / PDMPC_PRIO_TILE);
}

// PrioState::table and its pinned staging for M graphs
struct PrioLayout {
    size_t graph, tile_first, in_bytes, row_first, total;
};
PrioLayout prio_layout(int M) {
    Carver c;
    PrioLayout L;
    L.graph = c.take<PriorityArgs>((size_t)M);
    L.tile_first = c.take<int64_t>((size_t)M + 1);
    L.in_bytes = c.at;  // (what the count pass needs: the first copy)
    L.row_first = c.take<int64_t>((size_t)M + 1);
    L.total = c.at;
    return L;
}

// pdmpc_unique_priorities (grouped == false: M = 1, the graph in the kernel arguments) and its grouped sibling (the graphs and their
// tile prefix staged in ONE copy): count, scan, ONE read-back of the count(s), the capacity rule, write, order, the lists copied out.
// group_n / adjacency were checked by the entry points; edges[g] < 0 marks a graph outside the limits: it has no tiles and n_out -1.
int enumerate_priorities(pdmpc_handle* h, const char* who, bool grouped, int32_t M, const int32_t* group_n, const uint8_t* const* adjacency, const int32_t* edges,
                         const int64_t* max_out, int64_t* n_out, uint32_t* masks, int32_t* priorities) {
    const std::string w(who);
    ON_DEVICE(h->cfg.device);
    PrioState& P = h->prio;
    PriorityArgs one;
    PriorityGroups G{};
    const PrioLayout L = prio_layout(M);
    int64_t* tile_first = nullptr;
    int64_t n_tiles = 0;
    bool outside = false;
    if (grouped) {
        if (P.h_table.ensure(L.total) || P.table.ensure(L.total) || P.group_off.ensure((size_t)M + 1) || P.h_group_off.ensure((size_t)M + 1))
            return fail(PDMPC_ERR_HIP, "hipMalloc failed for the graph table of " + w);
        PriorityArgs* graph = (PriorityArgs*)(P.h_table.p + L.graph);
        tile_first = (int64_t*)(P.h_table.p + L.tile_first);
        for (int g = 0; g < M; ++g) {
            tile_first[g] = n_tiles;
            n_out[g] = -1;
            if (edges[g] < 0) {
                std::memset(&graph[g], 0, sizeof graph[g]);
                outside = true;
            } else
                n_tiles += stage_graph(graph[g], group_n[g], edges[g], adjacency[g]);
        }
        tile_first[M] = n_tiles;
        if (n_tiles > PDMPC_PRIO_MAX_TILES) return fail(PDMPC_ERR_CAPACITY, w + ": the graphs have 2^24 or more tiles of PDMPC_PRIO_TILE orientations");
        G.n_groups = M;
        G.graph = (const PriorityArgs*)(P.table.p + L.graph);
        G.tile_first = (const int64_t*)(P.table.p + L.tile_first);
        G.mask_first = P.group_off.p;
        G.row_first = (const int64_t*)(P.table.p + L.row_first);
    } else
        n_tiles = stage_graph(one, group_n[0], edges[0], adjacency[0]);
    int64_t total = 0;
    if (n_tiles > 0) {
        if (P.count.ensure((size_t)n_tiles) || P.off.ensure((size_t)n_tiles + 1)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the tile counts of " + w);
        int lrc;
        if (grouped) {
            HIPCHK(hipMemcpyAsync(P.table.p, P.h_table.p, L.in_bytes, hipMemcpyHostToDevice, h->stream));
            lrc = pdmpc_launch_priority_count_grouped(&G, n_tiles, P.count.p, (void*)h->stream);
        } else
            lrc = pdmpc_launch_priority_count(&one, n_tiles, P.count.p, (void*)h->stream);
        if (!lrc) lrc = pdmpc_launch_priority_scan(P.count.p, n_tiles, P.off.p, (void*)h->stream);
        if (!lrc && grouped) lrc = pdmpc_launch_priority_group_offsets(&G, P.off.p, (void*)h->stream);
        if (lrc) return fail(PDMPC_ERR_HIP, std::string("priority kernel launch failed: ") + hipGetErrorString((hipError_t)lrc));
        if (grouped)
            HIPCHK(hipMemcpyAsync(P.h_group_off.p, P.group_off.p, ((size_t)M + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        else
            HIPCHK(hipMemcpyAsync(&total, P.off.p + n_tiles, sizeof total, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(sync_stream(h));
    }
    int over = -1;  // the first graph with more unique prioritizations than its max_out
    if (grouped) {
        const int64_t* first = P.h_group_off.p;
        for (int g = 0; g < M; ++g) {
            if (edges[g] < 0) continue;
            n_out[g] = first[g + 1] - first[g];
            if (n_out[g] > max_out[g] && over < 0) over = g;
        }
        total = n_tiles > 0 ? first[M] : 0;
    } else {
        n_out[0] = total;
        if (total > max_out[0]) over = 0;
    }
    if (over >= 0) {
        char buf[200];
        if (grouped)
            snprintf(buf, sizeof buf, "%s: graph %d has %lld unique prioritizations, its max_out is %lld", who, over, (long long)n_out[over], (long long)max_out[over]);
        else
            snprintf(buf, sizeof buf, "%s: %lld unique prioritizations, max_out is %lld", who, (long long)total, (long long)max_out[0]);
        return fail(PDMPC_ERR_CAPACITY, buf);
    }
    if (outside) return fail(PDMPC_ERR_CAPACITY, w + ": a graph has more than 64 vehicles or more than 32 coupling edges");
    int64_t rows = 0;  // entries of priorities
    if (grouped) {
        int64_t* row_first = (int64_t*)(P.h_table.p + L.row_first);
        for (int g = 0; g < M; ++g) {
            row_first[g] = rows;
            rows += n_out[g] * group_n[g];
        }
        row_first[M] = rows;
    } else
        rows = total * group_n[0];
    if (P.mask.ensure((size_t)total) || P.order.ensure((size_t)rows)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the output of " + w);
    int lrc;
    if (grouped) {
        HIPCHK(hipMemcpyAsync(P.table.p + L.row_first, P.h_table.p + L.row_first, L.total - L.row_first, hipMemcpyHostToDevice, h->stream));
        lrc = pdmpc_launch_priority_write_grouped(&G, n_tiles, P.off.p, total, P.mask.p, (void*)h->stream);
        if (!lrc) lrc = pdmpc_launch_priority_order_grouped(&G, P.mask.p, total, P.order.p, (void*)h->stream);
    } else {
        lrc = pdmpc_launch_priority_write(&one, n_tiles, P.off.p, total, P.mask.p, (void*)h->stream);
        if (!lrc) lrc = pdmpc_launch_priority_order(&one, P.mask.p, total, P.order.p, (void*)h->stream);
    }
    if (lrc) return fail(PDMPC_ERR_HIP, std::string("priority kernel launch failed: ") + hipGetErrorString((hipError_t)lrc));
    HIPCHK(hipMemcpyAsync(masks, P.mask.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(priorities, P.order.p, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    return PDMPC_OK;
}
}  // namespace

extern "C" {

int pdmpc_unique_priorities(pdmpc_handle* h, int32_t n, const uint8_t* adjacency, int64_t max_out, int64_t* n_out, uint32_t* masks, int32_t* priorities) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (n_out) *n_out = -1;
    if (n < 1 || !adjacency || !n_out || max_out < 0 || (max_out > 0 && (!masks || !priorities)))
        return fail(PDMPC_ERR_INVALID, "pdmpc_unique_priorities: bad argument");
    if (n > PDMPC_PRIO_MAX_N) return fail(PDMPC_ERR_CAPACITY, "pdmpc_unique_priorities: more than 64 vehicles");
    const int32_t E = count_edges(n, adjacency);
    if (E > PDMPC_PRIO_MAX_E) return fail(PDMPC_ERR_CAPACITY, "pdmpc_unique_priorities: more than 32 coupling edges");
    return enumerate_priorities(h, "pdmpc_unique_priorities", false, 1, &n, &adjacency, &E, &max_out, n_out, masks, priorities);
}

// ... of several graphs in one call: one staging copy, one launch per pass and one read-back of the counts, whatever the number of graphs
int pdmpc_unique_priorities_grouped(pdmpc_handle* h, int32_t n_groups, const int32_t* group_n, const uint8_t** adjacency, int64_t* max_out, int64_t* n_out, uint32_t* masks,
                                    int32_t* priorities) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (n_groups < 1 || !group_n || !adjacency || !max_out || !n_out) return fail(PDMPC_ERR_INVALID, "pdmpc_unique_priorities_grouped: bad argument");
    for (int g = 0; g < n_groups; ++g) {
        n_out[g] = -1;
        if (group_n[g] < 1 || !adjacency[g] || max_out[g] < 0 || (max_out[g] > 0 && (!masks || !priorities)))
            return fail(PDMPC_ERR_INVALID, "pdmpc_unique_priorities_grouped: bad argument for graph " + std::to_string(g));
    }
    std::vector<int32_t>& edges = h->prio.edges;
    edges.resize((size_t)n_groups);
    for (int g = 0; g < n_groups; ++g) {
        edges[(size_t)g] = group_n[g] > PDMPC_PRIO_MAX_N ? -1 : count_edges(group_n[g], adjacency[g]);
        if (edges[(size_t)g] > PDMPC_PRIO_MAX_E) edges[(size_t)g] = -1;
    }
    return enumerate_priorities(h, "pdmpc_unique_priorities_grouped", true, n_groups, group_n, adjacency, edges.data(), max_out, n_out, masks, priorities);
}

// ---- the reachable-set coupler on the device (reachable_kernel.hip)
namespace {
// ReachState::ws and its pinned staging for n vehicles (carved the same way at upload, for max_vehicles, and per call): the inputs are
// the block's first in_bytes, the coupler's output its last
struct ReachLayout {
    size_t in, trim, group, in_bytes, hull_x, hull_y, box, hull_n, total;
    PairOut out;
};
ReachLayout reach_layout(int n, int cols) {
    Carver c;
    ReachLayout L;
    L.in = c.take<double>((size_t)4 * n);
    L.trim = c.take<int32_t>((size_t)n);
    L.group = c.take<int32_t>((size_t)3 * n);  // (PairGroup per vehicle: the grouped call's)
    L.in_bytes = c.end8();
    L.hull_x = c.take<double>((size_t)n * cols);
    L.hull_y = c.take<double>((size_t)n * cols);
    L.box = c.take<double>((size_t)4 * n);
    L.hull_n = c.take<int32_t>((size_t)n);
    L.out = carve_pair_out(c, n);
    L.total = c.at;
    return L;
}
}  // namespace

int pdmpc_upload_reachable_sets(pdmpc_handle* h, int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* sets) {
    if (!h || !sets || !sets->offset || n_trims < 1 || Hp < 1) return fail(PDMPC_ERR_INVALID, "pdmpc_upload_reachable_sets: bad argument");
    if (Hp != h->cfg.Hp) return fail(PDMPC_ERR_INVALID, "pdmpc_upload_reachable_sets: Hp differs from the handle's config.Hp");
    if (sets->n_polygons != n_trims * Hp) return fail(PDMPC_ERR_INVALID, "pdmpc_upload_reachable_sets: expected n_trims * Hp polygons");
    int cols = 1;
    for (int p = 0; p < sets->n_polygons; ++p) {
        const int m = sets->offset[p + 1] - sets->offset[p];
        if (m < 1) return fail(PDMPC_ERR_INVALID, "pdmpc_upload_reachable_sets: empty polygon");
        if (m > PDMPC_REACHABLE_MAX_COLS) return fail(PDMPC_ERR_CAPACITY, "pdmpc_upload_reachable_sets: a hull has more than PDMPC_REACHABLE_MAX_COLS vertices");
        cols = std::max(cols, m);
    }
    if (!sets->x || !sets->y) return fail(PDMPC_ERR_INVALID, "pdmpc_upload_reachable_sets: null coordinates");
    // only step Hp is coupled on (ReachableSetCoupler.m:9-12: reachable_sets(:, end))
    std::vector<int32_t> off((size_t)n_trims + 1, 0);
    for (int t = 0; t < n_trims; ++t) {
        const int p = t * Hp + Hp - 1;
        off[t + 1] = off[t] + (sets->offset[p + 1] - sets->offset[p]);
    }
    const int tot = off[n_trims];
    std::vector<double> xy((size_t)2 * tot);
    for (int t = 0; t < n_trims; ++t) {
        const int p = t * Hp + Hp - 1, a = sets->offset[p], m = sets->offset[p + 1] - a;
        std::memcpy(xy.data() + off[t], sets->x + a, (size_t)m * sizeof(double));
        std::memcpy(xy.data() + tot + off[t], sets->y + a, (size_t)m * sizeof(double));
    }
    ON_DEVICE(h->cfg.device);
    ReachState& R = h->reach;
    R.valid = false;
    const ReachLayout L = reach_layout(h->max_vehicles, cols);
    if (R.local.ensure_exact(xy.size()) || R.off.ensure_exact(off.size()) || R.ws.ensure_exact(L.total) || R.h_in.ensure(L.in_bytes) ||
        R.h_out.ensure(L.total - L.out.adj))
        return fail(PDMPC_ERR_HIP, "hipMalloc failed for the reachable-set coupler");
    HIPCHK(hipMemcpy(R.local.p, xy.data(), xy.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.off.p, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    // ... and every step's hulls for the lanelet bounding (pdmpc_bound_reachable_sets)
    h->bound.valid = false;
    const int all_tot = sets->offset[sets->n_polygons] - sets->offset[0];
    std::vector<double> all_xy((size_t)2 * all_tot);
    std::vector<int32_t> all_off((size_t)sets->n_polygons + 1);
    for (int p = 0; p <= sets->n_polygons; ++p) all_off[p] = sets->offset[p] - sets->offset[0];
    std::memcpy(all_xy.data(), sets->x + sets->offset[0], (size_t)all_tot * sizeof(double));
    std::memcpy(all_xy.data() + all_tot, sets->y + sets->offset[0], (size_t)all_tot * sizeof(double));
    if (R.all.ensure_exact(all_xy.size()) || R.all_off.ensure_exact(all_off.size())) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the reachable-set table");
    HIPCHK(hipMemcpy(R.all.p, all_xy.data(), all_xy.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.all_off.p, all_off.data(), all_off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    R.all_tot = all_tot;
    R.off_host = off;
    R.trims = n_trims;
    R.Hp = Hp;
    R.cols = cols;
    R.valid = true;
    return PDMPC_OK;
}

namespace {
// pdmpc_reachable_set_coupling (group_offset == NULL) and its grouped sibling: one staging copy, the pose pass over all n vehicles, one
// pair pass, one copy back, one synchronisation -- whatever the number of groups
int reachable_coupling(pdmpc_handle* h, const char* who, int32_t n_groups, const int32_t* group_offset, int32_t n, const double* x, const double* y,
                       const double* cos_yaw, const double* sin_yaw, const int32_t* trim, uint8_t* adjacency, double* area) {
    const std::string w(who);
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    ReachState& R = h->reach;
    if (!R.valid) return fail(PDMPC_ERR_INVALID, w + " before pdmpc_upload_reachable_sets");
    if (group_offset)
        if (const int rc = check_groups(who, n_groups, group_offset, &n)) return rc;
    if (n < 0 || !adjacency || (n > 0 && (!x || !y || !cos_yaw || !sin_yaw || !trim))) return fail(PDMPC_ERR_INVALID, w + ": bad argument");
    if (n > h->max_vehicles) return fail(PDMPC_ERR_CAPACITY, w + ": more vehicles than config.max_vehicles");
    if (n == 0) return PDMPC_OK;
    for (int v = 0; v < n; ++v)
        if (trim[v] < 1 || trim[v] > R.trims) return fail(PDMPC_ERR_INVALID, w + ": trim out of range");
    ON_DEVICE(h->cfg.device);
    const ReachLayout L = reach_layout(n, R.cols);
    unsigned char *hin = R.h_in.p, *ws = R.ws.p;
    stage_poses((double*)(hin + L.in), (size_t)n, x, y, cos_yaw, sin_yaw, (int32_t*)(hin + L.trim), trim);
    ReachArgs A;
    A.group = nullptr;
    A.max_group = n;
    size_t entries = (size_t)n * n;
    if (group_offset) {
        entries = stage_groups((PairGroup*)(hin + L.group), n_groups, group_offset, &A.max_group);
        A.group = (const int32_t*)(ws + L.group);
    }
    A.n = n;
    A.max_cols = R.cols;
    A.local_x = R.local.p;
    A.local_y = R.local.p + R.off_host[R.trims];
    A.local_off = R.off.p;
    A.in = (const double*)(ws + L.in);
    A.trim = (const int32_t*)(ws + L.trim);
    A.hull_x = (double*)(ws + L.hull_x);
    A.hull_y = (double*)(ws + L.hull_y);
    A.hull_n = (int32_t*)(ws + L.hull_n);
    A.box = (double*)(ws + L.box);
    A.adjacency = (uint8_t*)(ws + L.out.adj);
    A.area = (double*)(ws + L.out.area);
    HIPCHK(hipMemcpyAsync(ws, hin, L.in_bytes, hipMemcpyHostToDevice, h->stream));
    if (const int rc = timed_launch(h, R.coupling, group_offset ? pdmpc_launch_reachable_coupling_grouped : pdmpc_launch_reachable_coupling, A, "reachable-set coupling"))
        return rc;
    return fetch_pair_out(h, R.coupling, ws, R.h_out.p, L.out, entries, adjacency, area);
}
}  // namespace

int pdmpc_reachable_set_coupling(pdmpc_handle* h, int32_t n, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, const int32_t* trim,
                                 uint8_t* adjacency, double* area) {
    return reachable_coupling(h, "pdmpc_reachable_set_coupling", 0, nullptr, n, x, y, cos_yaw, sin_yaw, trim, adjacency, area);
}

int pdmpc_reachable_set_coupling_grouped(pdmpc_handle* h, int32_t n_groups, const int32_t* group_offset, const double* x, const double* y, const double* cos_yaw,
                                         const double* sin_yaw, const int32_t* trim, uint8_t* adjacency, double* area) {
    if (!group_offset) return fail(PDMPC_ERR_INVALID, "pdmpc_reachable_set_coupling_grouped: null group offsets");
    return reachable_coupling(h, "pdmpc_reachable_set_coupling_grouped", n_groups, group_offset, 0, x, y, cos_yaw, sin_yaw, trim, adjacency, area);
}

int pdmpc_reachable_set_coupling_kernel_ms(pdmpc_handle* h, double* ms) {
    if (!h || !ms) return fail(PDMPC_ERR_INVALID, "null argument");
    *ms = (double)h->reach.coupling.ms;
    return PDMPC_OK;
}

// ---- lanelet bounding and the coupler on the bounded sets (bounded_kernel.hip)
namespace {
// BoundState::in and its pinned staging (the lanelet polygons: x of all n_lan vertices, then y), and BoundState::out
struct BoundLayout {
    size_t in, trim, lan_off, lan_xy, in_bytes, group, in_total, out_bytes;
    PairOut out;
};
BoundLayout bound_layout(int n, int n_lan) {
    Carver c;
    BoundLayout L;
    L.in = c.take<double>((size_t)4 * n);
    L.trim = c.take<int32_t>((size_t)n);
    L.lan_off = c.take<int32_t>((size_t)n + 1);
    L.lan_xy = c.take<double>((size_t)2 * n_lan);
    L.in_bytes = c.at;
    L.group = c.take<int32_t>((size_t)3 * n);  // (PairGroup per vehicle: staged by the grouped coupler, after the bounding call's inputs)
    L.in_total = c.at;
    Carver o;
    L.out = carve_pair_out(o, n);
    L.out_bytes = o.at;
    return L;
}
BoundArgs bound_args(pdmpc_handle* h, int n, int S, int n_lan) {
    const ReachState& R = h->reach;
    BoundState& B = h->bound;
    const BoundLayout L = bound_layout(n, n_lan);
    BoundArgs A;
    A.n = n;
    A.S = S;
    A.Hp = R.Hp;
    A.all_steps = S == R.Hp && S > 1 ? 1 : 0;
    A.local_x = R.all.p;
    A.local_y = R.all.p + R.all_tot;
    A.local_off = R.all_off.p;
    A.in = (const double*)(B.in.p + L.in);
    A.trim = (const int32_t*)(B.in.p + L.trim);
    A.lan_off = (const int32_t*)(B.in.p + L.lan_off);
    A.lan_x = (const double*)(B.in.p + L.lan_xy);
    A.lan_y = A.lan_x + n_lan;
    const size_t slots = (size_t)n * S * PDMPC_BOUND_SLOT;
    A.set_x = B.sets.p;
    A.set_y = B.sets.p + slots;
    A.set_n = B.set_n.p;
    A.set_flags = B.flags.p;
    A.box = B.box.p;
    A.adjacency = B.out.p + L.out.adj;
    A.area = (double*)(B.out.p + L.out.area);
    A.pairs = B.pairs.p;
    A.n_pairs = B.pairs.p + (n > 1 ? (size_t)n * (n - 1) / 2 : 0);
    A.group = (const int32_t*)(B.in.p + L.group);
    A.max_group = n;
    return A;
}
}  // namespace

int pdmpc_bound_reachable_sets(pdmpc_handle* h, int32_t n, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, const int32_t* trim,
                               const pdmpc_polygon_set* lan, int32_t all_steps, int32_t capacity, int32_t* offset, double* out_x, double* out_y, uint8_t* flags) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (!h->reach.valid) return fail(PDMPC_ERR_INVALID, "pdmpc_bound_reachable_sets before pdmpc_upload_reachable_sets");
    if (n < 0 || !offset || !lan || lan->n_polygons != n || (n > 0 && (!x || !y || !cos_yaw || !sin_yaw || !trim || !lan->offset)))
        return fail(PDMPC_ERR_INVALID, "pdmpc_bound_reachable_sets: bad argument");
    if (n > h->max_vehicles) return fail(PDMPC_ERR_CAPACITY, "pdmpc_bound_reachable_sets: more vehicles than config.max_vehicles");
    BoundState& B = h->bound;
    const int Hp = h->reach.Hp, S = all_steps ? Hp : 1;
    B.valid = false;
    offset[0] = 0;
    if (n == 0) {
        B.n = 0;
        B.S = S;
        B.valid = true;
        return PDMPC_OK;
    }
    int n_lan = 0;
    for (int v = 0; v < n; ++v) {
        if (trim[v] < 1 || trim[v] > h->reach.trims) return fail(PDMPC_ERR_INVALID, "pdmpc_bound_reachable_sets: trim out of range");
        const int nl = lan->offset[v + 1] - lan->offset[v];
        if (nl < 0) return fail(PDMPC_ERR_INVALID, "pdmpc_bound_reachable_sets: bad lanelet offsets");
        if (nl > PDMPC_LANELET_POLY_MAX_COLS) return fail(PDMPC_ERR_CAPACITY, "pdmpc_bound_reachable_sets: a lanelet polygon has more than PDMPC_LANELET_POLY_MAX_COLS vertices");
        if (nl && (!lan->x || !lan->y)) return fail(PDMPC_ERR_INVALID, "pdmpc_bound_reachable_sets: null lanelet coordinates");
        n_lan += nl;
    }
    ON_DEVICE(h->cfg.device);
    const BoundLayout L = bound_layout(n, n_lan);
    const size_t sets = (size_t)n * S, max_pairs = (size_t)n * (n - 1) / 2;
    // (the pinned output block serves this call's vertex counts and flags and the coupler's output)
    if (B.in.ensure(L.in_total) || B.sets.ensure(2 * sets * PDMPC_BOUND_SLOT) || B.set_n.ensure(sets) || B.flags.ensure(sets) || B.box.ensure((size_t)4 * n) ||
        B.out.ensure(L.out_bytes) || B.pairs.ensure(max_pairs + 1) || B.h_in.ensure(L.in_total) || B.h_out.ensure(L.out_bytes + sets * (sizeof(int32_t) + 1)))
        return fail(PDMPC_ERR_HIP, "hipMalloc failed for the lanelet bounding");
    // inputs: poses, 0-based trims, the normalized lanelet polygons (pdmpc_lanelet_polygon_normalize, as the host twin)
    unsigned char* hin = B.h_in.p;
    stage_poses((double*)(hin + L.in), (size_t)n, x, y, cos_yaw, sin_yaw, (int32_t*)(hin + L.trim), trim);
    int32_t* hoff = (int32_t*)(hin + L.lan_off);
    double* hlx = (double*)(hin + L.lan_xy);
    double* hly = hlx + n_lan;
    hoff[0] = 0;
    for (int v = 0; v < n; ++v) {
        const int a = lan->offset[v], nl = lan->offset[v + 1] - a;
        const int m = nl ? pdmpc_lanelet_polygon_normalize(lan->x + a, lan->y + a, nl, hlx + hoff[v], hly + hoff[v]) : 0;
        hoff[v + 1] = hoff[v] + m;
    }
    const int n_norm = hoff[n];
    if (n_norm != n_lan) {  // (duplicates dropped: x and y of the normalized polygons are contiguous again)
        std::memmove(hlx + n_norm, hly, (size_t)n_norm * sizeof(double));
    }
    HIPCHK(hipMemcpyAsync(B.in.p, hin, bound_layout(n, n_norm).in_bytes, hipMemcpyHostToDevice, h->stream));
    const BoundArgs A = bound_args(h, n, S, n_norm);
    if (const int rc = timed_launch(h, B.bounding, pdmpc_launch_bound_sets, A, "lanelet bounding")) return rc;
    int32_t* hn = (int32_t*)B.h_out.p;
    uint8_t* hf = (uint8_t*)(hn + sets);
    HIPCHK(hipMemcpyAsync(hn, B.set_n.p, sets * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(hf, B.flags.p, sets, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    B.bounding.fold();
    bool over = false;
    int maxc = 0;
    for (size_t o = 0; o < sets; ++o) {
        if (hf[o] & PDMPC_BOUND_OVERFLOW) over = true;
        offset[o + 1] = offset[o] + hn[o];
        maxc = std::max(maxc, (int)hn[o]);
    }
    if (over) return fail(PDMPC_ERR_CAPACITY, "pdmpc_bound_reachable_sets: a bounded set has more than PDMPC_BOUNDED_MAX_COLS vertices");
    B.n = n;
    B.S = S;
    B.n_lan = n_norm;
    B.valid = true;
    if (!out_x || !out_y || capacity < offset[sets]) return fail(PDMPC_ERR_CAPACITY, "pdmpc_bound_reachable_sets: capacity too small for the bounded sets");
    // read back the used part of every slot (a pitched copy), then pack
    if (B.h_xy.ensure(2 * sets * (size_t)maxc)) return fail(PDMPC_ERR_HIP, "hipHostMalloc failed for the bounded sets");
    double* bx = B.h_xy.p;
    double* by = bx + sets * (size_t)maxc;
    const size_t pitch = (size_t)PDMPC_BOUND_SLOT * sizeof(double), width = (size_t)maxc * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(bx, width, A.set_x, pitch, width, sets, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpy2DAsync(by, width, A.set_y, pitch, width, sets, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    for (size_t o = 0; o < sets; ++o) {
        std::memcpy(out_x + offset[o], bx + o * maxc, (size_t)hn[o] * sizeof(double));
        std::memcpy(out_y + offset[o], by + o * maxc, (size_t)hn[o] * sizeof(double));
    }
    if (flags) std::memcpy(flags, hf, sets);
    return PDMPC_OK;
}

namespace {
// pdmpc_bounded_set_coupling (one group over the bounded vehicles, the ungrouped launcher) and its grouped sibling behind their argument
// checks: the groups cover the B.n vehicles of the last bounding call, whose sets are still on the device
int bounded_coupling(pdmpc_handle* h, int32_t n_groups, const int32_t* group_offset, int (*launch)(const BoundArgs*, void*), uint8_t* adjacency, double* area) {
    BoundState& B = h->bound;
    const int n = B.n;
    if (n == 0) return PDMPC_OK;
    ON_DEVICE(h->cfg.device);
    const BoundLayout L = bound_layout(n, B.n_lan);
    BoundArgs A = bound_args(h, n, B.S, B.n_lan);
    const size_t entries = stage_groups((PairGroup*)(B.h_in.p + L.group), n_groups, group_offset, &A.max_group);
    HIPCHK(hipMemcpyAsync(B.in.p + L.group, B.h_in.p + L.group, (size_t)n * sizeof(PairGroup), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(A.n_pairs, 0, sizeof(int32_t), h->stream));
    if (const int rc = timed_launch(h, B.coupling, launch, A, "bounded-set coupling")) return rc;
    return fetch_pair_out(h, B.coupling, B.out.p, B.h_out.p, L.out, entries, adjacency, area);
}
}  // namespace

int pdmpc_bounded_set_coupling(pdmpc_handle* h, uint8_t* adjacency, double* area) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (!adjacency) return fail(PDMPC_ERR_INVALID, "pdmpc_bounded_set_coupling: null adjacency");
    if (!h->bound.valid) return fail(PDMPC_ERR_INVALID, "pdmpc_bounded_set_coupling without a successful pdmpc_bound_reachable_sets");
    const int32_t all[2] = {0, h->bound.n};
    return bounded_coupling(h, 1, all, pdmpc_launch_bounded_coupling, adjacency, area);
}

int pdmpc_bounded_set_coupling_grouped(pdmpc_handle* h, int32_t n_groups, const int32_t* group_offset, uint8_t* adjacency, double* area) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (!adjacency) return fail(PDMPC_ERR_INVALID, "pdmpc_bounded_set_coupling_grouped: null adjacency");
    if (!h->bound.valid) return fail(PDMPC_ERR_INVALID, "pdmpc_bounded_set_coupling_grouped without a successful pdmpc_bound_reachable_sets");
    int n = 0;
    if (const int rc = check_groups("pdmpc_bounded_set_coupling_grouped", n_groups, group_offset, &n)) return rc;
    if (n > h->max_vehicles) return fail(PDMPC_ERR_CAPACITY, "pdmpc_bounded_set_coupling_grouped: more vehicles than config.max_vehicles");
    if (n != h->bound.n) return fail(PDMPC_ERR_INVALID, "pdmpc_bounded_set_coupling_grouped: the groups do not cover the vehicles of the last pdmpc_bound_reachable_sets");
    return bounded_coupling(h, n_groups, group_offset, pdmpc_launch_bounded_coupling_grouped, adjacency, area);
}

int pdmpc_bounded_reachable_kernel_ms(pdmpc_handle* h, double* ms2) {
    if (!h || !ms2) return fail(PDMPC_ERR_INVALID, "null argument");
    ms2[0] = (double)h->bound.bounding.ms;
    ms2[1] = (double)h->bound.coupling.ms;
    return PDMPC_OK;
}

// ---- future collision assessment on the device (fca_kernel.hip)
namespace {
// pdmpc_fca_collisions (one group, the ungrouped kernel) and pdmpc_fca_collisions_grouped behind their argument
// checks, for n > 0 vehicles in all: the groups' reference points as they come, their polygons one group after the other, their pairs
// rebased to the concatenated vehicles, and the tables the grouped kernels locate an item's group with.  The ungrouped kernel reads
// the same arrays and none of the tables: with one group every offset of its own layout is the one staged here.
int fca_assess(pdmpc_handle* h, const char* who, bool grouped, int32_t n_groups, const pdmpc_fca_group* groups, int32_t n, int32_t Hp, const double* x,
               const double* y, const double* cos_yaw, const double* sin_yaw, int32_t* collisions, int32_t* priorities) {
    const int m = n * Hp;
    // what a group brings: S static polygons of Ns vertices from vertex s0 on, D = R Hp dynamic ones of Nd vertices from d0 on
    struct Sizes {
        int S, D, s0, Ns, d0, Nd;
    };
    auto sizes_of = [](const pdmpc_fca_group& G) {
        Sizes z;
        z.S = G.n && G.obstacles ? G.obstacles->n_polygons : 0;
        z.D = G.n && G.dynamic_rows ? G.dynamic_rows->n_polygons : 0;
        z.s0 = z.S ? G.obstacles->offset[0] : 0;
        z.Ns = z.S ? G.obstacles->offset[z.S] - z.s0 : 0;
        z.d0 = z.D ? G.dynamic_rows->offset[0] : 0;
        z.Nd = z.D ? G.dynamic_rows->offset[z.D] - z.d0 : 0;
        return z;
    };
    int64_t S = 0, D = 0, Ns = 0, Nd = 0, n_pairs = 0;
    for (int g = 0; g < n_groups; ++g) {
        const Sizes z = sizes_of(groups[g]);
        S += z.S;
        D += z.D;
        Ns += z.Ns;
        Nd += z.Nd;
        n_pairs += groups[g].n ? groups[g].n_pairs : 0;
    }
    if (S > INT32_MAX || D > INT32_MAX || Ns > INT32_MAX || Nd > INT32_MAX || n_pairs > INT32_MAX)
        return fail(PDMPC_ERR_CAPACITY, std::string(who) + ": more than 2^31 polygons, vertices or pairs");
    // FcaState::ws and its pinned staging of the inputs, the block's first in_bytes (static and dynamic polygons: x of all their
    // vertices, then y; their offsets rebased to 0), the group tables among them; footprints and counts are on the device only
    Carver c;
    const size_t o_in = c.take<double>((size_t)4 * m);
    const size_t o_stat = c.take<double>((size_t)2 * Ns);
    const size_t o_dyn = c.take<double>((size_t)2 * Nd);
    const size_t o_stat_first = c.take<int64_t>((size_t)n_groups + 1);
    const size_t o_dyn_first = c.take<int64_t>((size_t)n_groups + 1);
    const size_t o_group = c.take<FcaGroup>((size_t)n_groups);
    const size_t o_pairs = c.take<int32_t>((size_t)2 * n_pairs);
    const size_t o_stat_off = c.take<int32_t>((size_t)S + 1);
    const size_t o_dyn_off = c.take<int32_t>((size_t)D + 1);
    const size_t o_vehicle_group = c.take<int32_t>((size_t)n);
    const size_t in_bytes = c.end8();
    const size_t o_fp = c.take<double>((size_t)8 * m);
    const size_t o_counts = c.take<int32_t>((size_t)n);
    const size_t total = c.at;
    ON_DEVICE(h->cfg.device);
    FcaState& F = h->fca;
    if (F.ws.ensure(total) || F.h_in.ensure(in_bytes) || F.h_out.ensure((size_t)n)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the collision assessment");
    unsigned char *hin = F.h_in.p, *ws = F.ws.p;
    stage_poses((double*)(hin + o_in), (size_t)m, x, y, cos_yaw, sin_yaw);
    double *hs = (double*)(hin + o_stat), *hdyn = (double*)(hin + o_dyn);
    int64_t *stat_first = (int64_t*)(hin + o_stat_first), *dyn_first = (int64_t*)(hin + o_dyn_first);
    FcaGroup* hg = (FcaGroup*)(hin + o_group);
    int32_t *hp = (int32_t*)(hin + o_pairs), *soff = (int32_t*)(hin + o_stat_off), *doff = (int32_t*)(hin + o_dyn_off), *vg = (int32_t*)(hin + o_vehicle_group);
    int v0 = 0, sp = 0, dp = 0, sv = 0, dv = 0;  // the next group's first vehicle, polygons and vertices
    int64_t pairs_done = 0;
    stat_first[0] = dyn_first[0] = 0;
    for (int g = 0; g < n_groups; ++g) {
        const pdmpc_fca_group& G = groups[g];
        const Sizes z = sizes_of(G);
        hg[g] = FcaGroup{v0, z.S, z.D / Hp, sp, dp, G.length, G.width, G.offset};
        // (the reference's outer loop stops at n - 1, per group: the last vehicle of a group has no obstacle items)
        stat_first[g + 1] = stat_first[g] + (G.n ? (int64_t)(G.n - 1) * Hp * z.S : 0);
        dyn_first[g + 1] = dyn_first[g] + (G.n ? (int64_t)(G.n - 1) * Hp * (z.D / Hp) : 0);
        if (G.n == 0) continue;
        for (int v = 0; v < G.n; ++v) vg[v0 + v] = g;
        for (int p = 0; p < 2 * G.n_pairs; ++p) hp[2 * pairs_done + p] = v0 + G.pairs[p];
        pairs_done += G.n_pairs;
        if (z.Ns) {
            std::memcpy(hs + sv, G.obstacles->x + z.s0, (size_t)z.Ns * sizeof(double));
            std::memcpy(hs + Ns + sv, G.obstacles->y + z.s0, (size_t)z.Ns * sizeof(double));
        }
        if (z.Nd) {
            std::memcpy(hdyn + dv, G.dynamic_rows->x + z.d0, (size_t)z.Nd * sizeof(double));
            std::memcpy(hdyn + Nd + dv, G.dynamic_rows->y + z.d0, (size_t)z.Nd * sizeof(double));
        }
        for (int p = 0; p < z.S; ++p) soff[sp + p] = sv + G.obstacles->offset[p] - z.s0;
        for (int p = 0; p < z.D; ++p) doff[dp + p] = dv + G.dynamic_rows->offset[p] - z.d0;
        v0 += G.n;
        sp += z.S;
        dp += z.D;
        sv += z.Ns;
        dv += z.Nd;
    }
    soff[S] = (int32_t)Ns;
    doff[D] = (int32_t)Nd;
    FcaGroupedArgs B;
    std::memset(&B, 0, sizeof B);
    FcaArgs& A = B.a;
    A.n = n;
    A.Hp = Hp;
    A.n_pairs = (int32_t)n_pairs;
    A.n_pair_items = n_pairs * Hp;
    A.n_static_items = stat_first[n_groups];
    A.n_items = A.n_pair_items + A.n_static_items + dyn_first[n_groups];
    A.in = (const double*)(ws + o_in);
    A.static_x = (const double*)(ws + o_stat);
    A.static_y = A.static_x + Ns;
    A.dyn_x = (const double*)(ws + o_dyn);
    A.dyn_y = A.dyn_x + Nd;
    A.pairs = (const int32_t*)(ws + o_pairs);
    A.static_off = (const int32_t*)(ws + o_stat_off);
    A.dyn_off = (const int32_t*)(ws + o_dyn_off);
    A.fp = (double*)(ws + o_fp);
    A.counts = (int32_t*)(ws + o_counts);
    B.g.n_groups = n_groups;
    B.g.group = (const FcaGroup*)(ws + o_group);
    B.g.vehicle_group = (const int32_t*)(ws + o_vehicle_group);
    B.g.static_first = (const int64_t*)(ws + o_stat_first);
    B.g.dyn_first = (const int64_t*)(ws + o_dyn_first);
    if (!grouped) {  // (what the ungrouped kernel reads in place of the group table)
        A.n_static = hg[0].n_static;
        A.n_rows = hg[0].n_rows;
        A.length = hg[0].length;
        A.width = hg[0].width;
        A.offset = hg[0].offset;
    }
    HIPCHK(hipMemcpyAsync(ws, hin, in_bytes, hipMemcpyHostToDevice, h->stream));
    if (const int rc = grouped ? timed_launch(h, F.timed, pdmpc_launch_fca_grouped, B, "collision assessment")
                               : timed_launch(h, F.timed, pdmpc_launch_fca, A, "collision assessment"))
        return rc;
    HIPCHK(hipMemcpyAsync(F.h_out.p, ws + o_counts, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    F.timed.fold();
    std::memcpy(collisions, F.h_out.p, (size_t)n * sizeof(int32_t));
    v0 = 0;
    for (int g = 0; g < n_groups; ++g) {  // every group's own index vector
        if (groups[g].n) pdmpc_fca_sort_index(groups[g].n, collisions + v0, priorities + v0);
        v0 += groups[g].n;
    }
    return PDMPC_OK;
}

}  // namespace

int pdmpc_fca_collisions(pdmpc_handle* h, int32_t n, int32_t Hp, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw,
                         int32_t n_pairs, const int32_t* pairs, const pdmpc_polygon_set* obstacles, const pdmpc_polygon_set* dynamic_rows, double length,
                         double width, double offset, int32_t* collisions, int32_t* priorities) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    const char* why = nullptr;
    if (const int rc = pdmpc_fca_check_args(n, Hp, x, y, cos_yaw, sin_yaw, n_pairs, pairs, obstacles, dynamic_rows, collisions, priorities, &why))
        return fail(rc, std::string("pdmpc_fca_collisions: ") + why);
    const pdmpc_fca_group all = {n, n_pairs, pairs, obstacles, dynamic_rows, length, width, offset};
    return fca_assess(h, "pdmpc_fca_collisions", false, 1, &all, n, Hp, x, y, cos_yaw, sin_yaw, collisions, priorities);
}

int pdmpc_fca_collisions_grouped(pdmpc_handle* h, int32_t n_groups, const pdmpc_fca_group* groups, int32_t Hp, const double* x, const double* y,
                                 const double* cos_yaw, const double* sin_yaw, int32_t* collisions, int32_t* priorities) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    char why[160];
    int32_t n = 0;
    if (const int rc = pdmpc_fca_check_groups(n_groups, groups, Hp, x, y, cos_yaw, sin_yaw, collisions, priorities, &n, why, (int32_t)sizeof why))
        return fail(rc, std::string("pdmpc_fca_collisions_grouped: ") + why);
    if (n > h->max_vehicles) return fail(PDMPC_ERR_CAPACITY, "pdmpc_fca_collisions_grouped: more vehicles than config.max_vehicles");
    if (n == 0) return PDMPC_OK;
    return fca_assess(h, "pdmpc_fca_collisions_grouped", true, n_groups, groups, n, Hp, x, y, cos_yaw, sin_yaw, collisions, priorities);
}

int pdmpc_fca_kernel_ms(pdmpc_handle* h, double* ms) {
    if (!h || !ms) return fail(PDMPC_ERR_INVALID, "null argument");
    *ms = (double)h->fca.timed.ms;
    return PDMPC_OK;
}

// ---- human-driven vehicles on the device (hdv_kernel.hip).  The plan of a call is host-only code (hdv_call_host.hpp:
// the workspace layout, the caller's arrays as records, check, zero, stage, arguments, scatter); the handle's buffers, the two copies,
// the launch and the synchronisation are here.
namespace {
// what the kernels read of a map slot: the views into its device table
HdvMapRecord hdv_record(const HdvMapSlot& M) {
    const HdvTable T = hdv_table(M.data.map, M.data.trims * M.data.Hp, M.data.local_tot);
    const unsigned char* tb = M.table.p;
    HdvMapRecord R;
    R.map = M.data.map.view((const int32_t*)(tb + T.pt_off), (const double*)(tb + T.pts), (const int32_t*)(tb + T.succ_off), (const int32_t*)(tb + T.succ_idx), tb + T.rel);
    R.local_x = (const double*)(tb + T.local_xy);
    R.local_y = R.local_x + M.data.local_tot;
    R.local_off = (const int32_t*)(tb + T.local_off);
    return R;
}
}  // namespace

int pdmpc_upload_hdv_map_slot(pdmpc_handle* h, int32_t slot, int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x,
                              const double* left_y, const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index,
                              const uint8_t* relationship, int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    if (slot < 0 || slot >= PDMPC_HDV_MAP_SLOTS) return fail(PDMPC_ERR_INVALID, "pdmpc_upload_hdv_map: map slot out of range");
    HdvState& S = h->hdv;
    HdvMapSlot& M = S.map[slot];
    M.valid = false;
    M.generation = 0;
    const char* why = nullptr;
    int rc = M.data.map.points(n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, &why);
    if (!rc) rc = M.data.map.graph(succ_offset, succ_index, relationship, &why);
    if (!rc) rc = hdv_check_sets(n_trims, Hp, hdv_local_sets, &why);
    if (rc) return fail(rc, std::string("pdmpc_upload_hdv_map: ") + why);
    M.data.keep_sets(n_trims, Hp, hdv_local_sets);
    const HdvMapData& m = M.data.map;
    const int local_tot = M.data.local_tot;
    const HdvTable T = hdv_table(m, n_trims * Hp, local_tot);
    std::vector<unsigned char> stage(T.total, 0);
    std::memcpy(stage.data() + T.pt_off, m.pt_off.data(), m.pt_off.size() * sizeof(int32_t));
    std::memcpy(stage.data() + T.pts, m.pts.data(), m.pts.size() * sizeof(double));
    std::memcpy(stage.data() + T.succ_off, m.succ_off.data(), m.succ_off.size() * sizeof(int32_t));
    if (m.n_succ) std::memcpy(stage.data() + T.succ_idx, m.succ_idx.data(), m.succ_idx.size() * sizeof(int32_t));
    std::memcpy(stage.data() + T.rel, m.rel.data(), m.rel.size());
    std::memcpy(stage.data() + T.local_off, M.data.local_off.data(), M.data.local_off.size() * sizeof(int32_t));
    std::memcpy(stage.data() + T.local_xy, M.data.local_xy.data(), M.data.local_xy.size() * sizeof(double));
    ON_DEVICE(h->cfg.device);
    // (every call synchronises before it returns: no launch reads a table or a record that is replaced here)
    if (M.table.ensure_exact(T.total)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the HDV map");
    if (!S.maps.p) {
        if (S.maps.ensure_exact(PDMPC_HDV_MAP_SLOTS)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the HDV map records");
        HIPCHK(hipMemset(S.maps.p, 0, S.maps.cap * sizeof(HdvMapRecord)));
    }
    HIPCHK(hipMemcpy(M.table.p, stage.data(), T.total, hipMemcpyHostToDevice));
    const HdvMapRecord R = hdv_record(M);
    HIPCHK(hipMemcpy(S.maps.p + slot, &R, sizeof R, hipMemcpyHostToDevice));
    static std::atomic<int64_t> generations{0};  // (of all handles: a remembered generation is found again on the handle and in the slot it came from only)
    M.generation = ++generations;
    S.uploads += 1;
    M.valid = true;
    return PDMPC_OK;
}

int pdmpc_upload_hdv_map(pdmpc_handle* h, int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x, const double* left_y,
                         const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index, const uint8_t* relationship,
                         int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets) {
    return pdmpc_upload_hdv_map_slot(h, 0, n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, succ_offset, succ_index, relationship, n_trims, Hp,
                                     hdv_local_sets);
}

int pdmpc_hdv_map_slot_state(pdmpc_handle* h, int32_t slot, int64_t* generation, int64_t* uploads, int32_t* Hp) {
    if (!h || slot < 0 || slot >= PDMPC_HDV_MAP_SLOTS) return fail(PDMPC_ERR_INVALID, "pdmpc_hdv_map_slot_state: bad argument");
    if (generation) *generation = h->hdv.map[slot].valid ? h->hdv.map[slot].generation : 0;
    if (uploads) *uploads = h->hdv.uploads;
    if (Hp) *Hp = h->hdv.map[slot].valid ? h->hdv.map[slot].data.Hp : 0;
    return PDMPC_OK;
}

int pdmpc_hdv_map_slot_holds(pdmpc_handle* h, int32_t slot, int32_t n_lanelets, const int32_t* left_offset, const int32_t* right_offset, const double* left_x,
                             const double* left_y, const double* right_x, const double* right_y, const int32_t* succ_offset, const int32_t* succ_index,
                             const uint8_t* relationship, int32_t n_trims, int32_t Hp, const pdmpc_polygon_set* hdv_local_sets, int32_t* holds) {
    if (!h || !holds || slot < 0 || slot >= PDMPC_HDV_MAP_SLOTS) return fail(PDMPC_ERR_INVALID, "pdmpc_hdv_map_slot_holds: bad argument");
    const HdvMapSlot& M = h->hdv.map[slot];
    *holds = M.valid && M.data.holds(n_lanelets, left_offset, right_offset, left_x, left_y, right_x, right_y, succ_offset, succ_index, relationship, n_trims, Hp, hdv_local_sets);
    return PDMPC_OK;
}

int pdmpc_hdv_traffic(pdmpc_handle* h, int32_t n_hdv, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, const int32_t* trim,
                      const double* tile_dx, const double* tile_dy, int32_t n_cav, const double* cav_x, const double* cav_y, const int32_t* cav_lanelet,
                      const double* cav_tile_dx, const double* cav_tile_dy, int32_t* closest_offset, int32_t* closest_index, int32_t capacity, int32_t* n_rows,
                      int32_t* row_hdv, int32_t* set_offset, double* set_x, double* set_y, uint8_t* set_flags, uint8_t* adjacency) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    HdvState& S = h->hdv;
    const HdvMapSlot& M0 = S.map[0];
    if (!M0.valid) return fail(PDMPC_ERR_INVALID, "pdmpc_hdv_traffic before pdmpc_upload_hdv_map");
    const char* why = nullptr;
    if (const int rc = hdv_check_call(M0.data.map.n_lanelets, M0.data.trims, n_hdv, x, y, cos_yaw, sin_yaw, trim, tile_dx, tile_dy, n_cav, cav_x, cav_y, cav_lanelet, cav_tile_dx,
                                      cav_tile_dy, closest_offset, closest_index, capacity, n_rows, row_hdv, set_offset, adjacency, &why))
        return fail(rc, std::string("pdmpc_hdv_traffic: ") + why);
    const HdvGroups G{0, nullptr, nullptr, nullptr, tile_dx, tile_dy, cav_x, cav_y, cav_tile_dx, cav_tile_dy};
    const HdvTrafficCall T{x, y, cos_yaw, sin_yaw, trim, cav_lanelet, closest_offset, closest_index, capacity, n_rows, row_hdv, set_offset, nullptr, set_x, set_y, set_flags, adjacency};
    const HdvPlan P = hdv_plan_one(n_hdv, n_cav, M0.data.Hp, T);
    hdv_zero_outputs(G, &T, P);
    if (P.n == 0) return PDMPC_OK;
    ON_DEVICE(h->cfg.device);
    const HdvWs L = hdv_ws(0, P);
    if (S.ws.ensure(L.total) || S.slots.ensure(hdv_slot_doubles(P)) || S.h_in.ensure(L.in_bytes) || S.h_out.ensure(L.total - L.out))
        return fail(PDMPC_ERR_HIP, "hipMalloc failed for the HDV traffic call");
    hdv_stage(S.h_in.p, L, P, G, &T, nullptr);
    const HdvMapRecord R = hdv_record(M0);
    const HdvArgs A = hdv_args(L, P, S.ws.p, S.slots.p, &R);
    HIPCHK(hipMemcpyAsync(S.ws.p, S.h_in.p, L.in_bytes, hipMemcpyHostToDevice, h->stream));
    if (const int rc = timed_launch(h, S.timed, pdmpc_launch_hdv_traffic, A, "HDV traffic")) return rc;
    HIPCHK(hipMemcpyAsync(S.h_out.p, S.ws.p + L.out, L.total - L.out, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    S.timed.fold();
    if (const int rc = hdv_scatter_one(S.h_out.p, L, P, T, &why)) return fail(rc, why);
    return PDMPC_OK;
}

// The grouped calls: the five passes of the traffic call (T), the drive pass in front of them (D and T), or the drive pass alone (D).
static int hdv_call(pdmpc_handle* h, const char* who, const HdvGroups& G, const HdvTrafficCall* T, const HdvDriveCall* D) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    HdvState& S = h->hdv;
    const HdvSlotData* slot[PDMPC_HDV_MAP_SLOTS];
    for (int s = 0; s < PDMPC_HDV_MAP_SLOTS; ++s) slot[s] = S.map[s].valid ? &S.map[s].data : nullptr;
    HdvPlan P;
    std::string why;
    if (const int rc = hdv_check_grouped(who, G, T, D, slot, P, &why)) return fail(rc, why);
    hdv_zero_outputs(G, T, P);
    if (P.n == 0) return PDMPC_OK;
    ON_DEVICE(h->cfg.device);
    const HdvWs L = hdv_ws(G.n_groups, P);
    // (the slots of the lane pass: what this call needs, without head room -- 256 KB x Hp per HDV)
    if (S.ws.ensure(L.total) || (T && S.slots.ensure_exact(hdv_slot_doubles(P))) || S.h_in.ensure(L.in_bytes) || S.h_out.ensure(L.total - L.out))
        return fail(PDMPC_ERR_HIP, "hipMalloc failed for the grouped HDV traffic call");
    hdv_stage(S.h_in.p, L, P, G, T, D);
    HdvDriveTrafficArgs A{};
    A.g = hdv_grouped_args(G.n_groups, L, P, S.ws.p, S.slots.p, S.maps.p);
    if (D) A.d = hdv_drive_args(L, P, S.ws.p, S.maps.p);
    HIPCHK(hipMemcpyAsync(S.ws.p, S.h_in.p, L.in_bytes, hipMemcpyHostToDevice, h->stream));
    if (D && T) {
        if (const int rc = timed_launch(h, S.timed, pdmpc_launch_hdv_drive_traffic_grouped, A, "grouped HDV drive and traffic")) return rc;
    } else if (D) {
        if (const int rc = timed_launch(h, S.timed, pdmpc_launch_hdv_drive, A.d, "grouped HDV drive")) return rc;
    } else {
        if (const int rc = timed_launch(h, S.timed, pdmpc_launch_hdv_traffic_grouped, A.g, "grouped HDV traffic")) return rc;
    }
    HIPCHK(hipMemcpyAsync(S.h_out.p, S.ws.p + L.out, L.total - L.out, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(sync_stream(h));
    S.timed.fold();
    if (const int rc = hdv_scatter(who, S.h_out.p, L, P, G, T, D, &why)) return fail(rc, why);
    return PDMPC_OK;
}

int pdmpc_hdv_traffic_grouped(pdmpc_handle* h, int32_t n_groups, const int32_t* group_slot, const int32_t* hdv_offset, const int32_t* cav_offset, const double* x,
                              const double* y, const double* cos_yaw, const double* sin_yaw, const int32_t* trim, const double* tile_dx, const double* tile_dy,
                              const double* cav_x, const double* cav_y, const int32_t* cav_lanelet, const double* cav_tile_dx, const double* cav_tile_dy,
                              int32_t* closest_offset, int32_t* closest_index, int32_t capacity, int32_t* n_rows, int32_t* row_hdv, int32_t* set_offset,
                              int32_t* set_base, double* set_x, double* set_y, uint8_t* set_flags, uint8_t* adjacency) {
    const HdvGroups G{n_groups, group_slot, hdv_offset, cav_offset, tile_dx, tile_dy, cav_x, cav_y, cav_tile_dx, cav_tile_dy};
    const HdvTrafficCall T{x, y, cos_yaw, sin_yaw, trim, cav_lanelet, closest_offset, closest_index, capacity, n_rows, row_hdv, set_offset, set_base, set_x, set_y, set_flags, adjacency};
    return hdv_call(h, "pdmpc_hdv_traffic_grouped: ", G, &T, nullptr);
}

int pdmpc_hdv_drive_grouped(pdmpc_handle* h, int32_t n_groups, const int32_t* group_slot, const int32_t* hdv_offset, const int32_t* cav_offset, const int32_t* route_offset,
                            const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_seg, const double* state_u, const double* tile_dx, const double* tile_dy,
                            const double* v_des, const double* cav_x, const double* cav_y, const double* cav_tile_dx, const double* cav_tile_dy, const double* parameters,
                            const double* dt, int32_t* new_seg, double* new_u, double* x, double* y, double* cos_yaw, double* sin_yaw, double* speed, double* gap) {
    const HdvGroups G{n_groups, group_slot, hdv_offset, cav_offset, tile_dx, tile_dy, cav_x, cav_y, cav_tile_dx, cav_tile_dy};
    const HdvDriveCall D{nullptr, route_offset, route_lanelet, closed, state_seg, state_u, v_des, parameters, dt, new_seg, new_u, x, y, cos_yaw, sin_yaw, speed, gap};
    return hdv_call(h, "pdmpc_hdv_drive_grouped: ", G, nullptr, &D);
}

int pdmpc_hdv_drive_traffic_grouped(pdmpc_handle* h, int32_t n_groups, const int32_t* group_slot, const int32_t* hdv_offset, const int32_t* cav_offset, const uint8_t* drives,
                                    const int32_t* route_offset, const int32_t* route_lanelet, const uint8_t* closed, const int32_t* state_seg, const double* state_u,
                                    const double* v_des, const double* parameters, const double* dt, int32_t* new_seg, double* new_u, double* speed, double* gap, double* x,
                                    double* y, double* cos_yaw, double* sin_yaw, const int32_t* trim, const double* tile_dx, const double* tile_dy, const double* cav_x,
                                    const double* cav_y, const int32_t* cav_lanelet, const double* cav_tile_dx, const double* cav_tile_dy, int32_t* closest_offset,
                                    int32_t* closest_index, int32_t capacity, int32_t* n_rows, int32_t* row_hdv, int32_t* set_offset, int32_t* set_base, double* set_x,
                                    double* set_y, uint8_t* set_flags, uint8_t* adjacency) {
    if (!drives) return fail(PDMPC_ERR_INVALID, "pdmpc_hdv_drive_traffic_grouped: no drive flags");
    const HdvGroups G{n_groups, group_slot, hdv_offset, cav_offset, tile_dx, tile_dy, cav_x, cav_y, cav_tile_dx, cav_tile_dy};
    const HdvTrafficCall T{x, y, cos_yaw, sin_yaw, trim, cav_lanelet, closest_offset, closest_index, capacity, n_rows, row_hdv, set_offset, set_base, set_x, set_y, set_flags, adjacency};
    const HdvDriveCall D{drives, route_offset, route_lanelet, closed, state_seg, state_u, v_des, parameters, dt, new_seg, new_u, x, y, cos_yaw, sin_yaw, speed, gap};
    return hdv_call(h, "pdmpc_hdv_drive_traffic_grouped: ", G, &T, &D);
}

int pdmpc_hdv_kernel_ms(pdmpc_handle* h, double* ms) {
    if (!h || !ms) return fail(PDMPC_ERR_INVALID, "null argument");
    *ms = (double)h->hdv.timed.ms;
    return PDMPC_OK;
}

}  // extern "C"
