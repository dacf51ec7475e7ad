// pack.cpp — the packer of the C ABI's host side (pdmpc_pack_step / pdmpc_pack_batch, api.cpp): flattens the caller's IterationData
// slices into the pointer-free HBM blob of pdmpc_device.h (this is where vectorize_all_obstacles.m:36-62's "[polygon, NaN]"
// concatenation happens for literal obstacles), in the slot order of coupling_order.hpp, and uploads it with one copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "coupling_order.hpp"
#include "sampled_launch.hpp"

namespace {

int check_set(const pdmpc_polygon_set& s, const char* what) {
    if (s.n_polygons < 0) return fail(PDMPC_ERR_INVALID, std::string(what) + ": negative polygon count");
    if (s.n_polygons > 0 && (!s.offset || !s.x || !s.y)) return fail(PDMPC_ERR_INVALID, std::string(what) + ": null pointer");
    for (int i = 0; i < s.n_polygons; ++i)
        if (s.offset[i + 1] < s.offset[i]) return fail(PDMPC_ERR_INVALID, std::string(what) + ": offsets not monotone");
    return PDMPC_OK;
}

size_t set_points(const pdmpc_polygon_set& s) {  // points of a (checked) set + one separator per polygon
    return s.n_polygons > 0 ? (size_t)(s.offset[s.n_polygons] - s.offset[0]) + (size_t)s.n_polygons : 0;
}

// Slot order -> B.perm / B.inv.  A search spins for predecessors of the same launch, so every predecessor must sit in a lower slot
// than its successors (launch_range: forward progress of oversubscribed launches).  Callers hand the vehicles over in level order
// (kahn.m); a batch that is not is put into level order here -- computation levels by longest path, stable within a level --
// and pdmpc_fetch_results hands the records back in the caller's order.
// Priority order (pdmpc_set_step_weights).  Workgroups are handed out in index order, and a launch of more searches than CUs
// starts its later workgroups when earlier ones end: in level order a heavy search of a late level starts late — behind finished
// searches that hold their CUs while they wait for predecessors (C4: 2.5-4 ms into a 10 ms step).  With an expected work per
// vehicle the slots are filled by PRIORITY instead (coupling_order.hpp): a topological order too — every predecessor in a lower
// slot: the forward-progress argument holds unchanged — and the records go back in the caller's order as for any batch the library
// reorders.
int slot_order(const pdmpc_handle* h, int n, const int32_t* pred_offset, const int32_t* pred_index, const std::vector<double>& weights, PackedStep& B) {
    B.perm.clear();
    B.inv.clear();
    if (!pred_offset) return PDMPC_OK;
    const bool by_priority = (int)weights.size() == n && n > 1;
    bool ordered = true;
    for (int i = 0; i < n && ordered; ++i)
        for (int q = pred_offset[i]; q < pred_offset[i + 1]; ++q) {
            const int ps = pred_index[q];
            if (ps < 0 || ps >= h->max_vehicles) return fail(PDMPC_ERR_INVALID, "predecessor slot out of range");
            if (ps < n && ps >= i) ordered = false;
        }
    if (ordered && !by_priority) return PDMPC_OK;  // (already in level order and no weights: the caller's order stays)
    CouplingOrder order;
    const CouplingOrder::Status st = order.build(n, pred_offset, pred_index, by_priority ? weights.data() : nullptr);
    if (st == CouplingOrder::kSelfEdge) return fail(PDMPC_ERR_INVALID, "a vehicle is its own predecessor");
    if (st == CouplingOrder::kCycle) return fail(PDMPC_ERR_INVALID, "the sequential coupling graph has a cycle");
    B.perm.resize((size_t)n);
    std::iota(B.perm.begin(), B.perm.end(), 0);
    order.sort(B.perm);
    bool identity = true;
    for (int i = 0; i < n && identity; ++i) identity = B.perm[(size_t)i] == i;
    if (identity) {
        B.perm.clear();  // (the caller's order is the order wanted: raw slots are the caller's vehicles)
    } else {
        B.inv.resize((size_t)n);
        for (int sl = 0; sl < n; ++sl) B.inv[(size_t)B.perm[(size_t)sl]] = sl;
    }
    return PDMPC_OK;
}

// One pack into a bank: the batch is written where it is copied from, the bank's pinned blob (BlobRegions).  The points come
// last — their number is known once they are written — and the blob grows with its contents kept.
struct Packer {
    pdmpc_handle* h;
    PackedStep& B;
    const int n;
    const pdmpc_vehicle_in* in;
    const int32_t *pred_offset, *pred_index;
    const pdmpc_polygon_set* fallback;
    const std::vector<uint32_t>* seeds;  // null: not a sampled bank
    size_t veh_bytes = 0, pts_base = 0;
    BlobRegions host;
    size_t n_pred_out = 0, n_pts = 0;  // entries of pred / POINTS (two doubles each) written
    int soup_cap = 0, cand_cap = 0, ll_cap = 0;

    BlobRegions regions(unsigned char* blob) const { return {(DevVehicle*)blob, (int32_t*)(blob + veh_bytes), (double*)(blob + pts_base)}; }
    int vehicle_of(int slot) const { return B.perm.empty() ? slot : B.perm[(size_t)slot]; }  // (the caller's vehicle)
    void put(double x, double y) {
        host.pts[2 * n_pts] = x;
        host.pts[2 * n_pts + 1] = y;
        ++n_pts;
    }
    void append_poly(const pdmpc_polygon_set& s, int p, bool sep) {
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        for (int q = s.offset[p]; q < s.offset[p + 1]; ++q) put(s.x[q], s.y[q]);
        if (sep) put(qnan, qnan);
    }

    // room for `points` more points (what is written so far kept); the host regions follow the blob
    int reserve(size_t points) {
        if (B.h_blob.ensure_keep(pts_base + (n_pts + points) * 16, pts_base + n_pts * 16)) return fail(PDMPC_ERR_HIP, "hipHostMalloc failed");
        host = regions(B.h_blob.p);
        return PDMPC_OK;
    }

    int open() {
        size_t total_pred = 0;
        if (pred_offset)
            for (int vi = 0; vi < n; ++vi) total_pred += (size_t)std::max(0, pred_offset[vi + 1] - pred_offset[vi]);
        veh_bytes = ((size_t)std::max(n, 1) * sizeof(DevVehicle) + 15) & ~(size_t)15;
        const size_t pred_bytes = ((total_pred + 1) * sizeof(int32_t) + 15) & ~(size_t)15;
        pts_base = veh_bytes + pred_bytes;
        B.host = BlobRegions{};
        if (int rc = reserve(256)) return rc;  // (4096 bytes: the trailing pad's room in a batch without points)
        B.lit_cols.assign((size_t)n, 0);
        return PDMPC_OK;
    }

    // Vehicles that hand over THE SAME ARRAYS (same pointers, same counts: the prioritization instances of an explorative step share
    // every input but the predecessor lists, PrioritizedExplorativeController.m:25-91; step_controller.cpp builds one set per distinct
    // content) share one copy of their soups in the pool: a vehicle seen before takes over the offsets of the first one.
    static SoupKey soup_key(const pdmpc_vehicle_in& v, const pdmpc_polygon_set* fbv) {
        SoupKey key;
        std::memset(&key, 0, sizeof key);
        const void* ptrs[13] = {v.obstacles.offset, v.obstacles.x, v.obstacles.y, v.dynamic_obstacles.offset, v.dynamic_obstacles.x, v.dynamic_obstacles.y, v.hdv_reachable_sets.offset,
                                v.hdv_reachable_sets.x, v.left_x, v.right_x, fbv ? fbv->offset : nullptr, fbv ? fbv->x : nullptr, fbv ? fbv->y : nullptr};
        for (int q = 0; q < 13; ++q) key.p[q] = ptrs[q];
        key.c[0] = v.obstacles.n_polygons;
        key.c[1] = v.dynamic_obstacles.n_polygons;
        key.c[2] = v.hdv_reachable_sets.n_polygons;
        key.c[3] = v.n_left;
        key.c[4] = v.n_right;
        key.c[5] = fbv ? fbv->n_polygons : 0;
        return key;
    }
    // ... and vehicles that agree in a PART of their arrays share that part (the vehicles of a centralized step on a road network see
    // the same obstacles inside boundaries of their own): the obstacle, dynamic-obstacle and HDV arrays with their counts decide
    // lit_off / hdv_off, the boundary arrays decide ll_off / ll_len.  Fallback areas are shared by the whole key above only.
    static SoupKey obstacle_key(const pdmpc_vehicle_in& v) {
        SoupKey key;
        std::memset(&key, 0, sizeof key);
        const void* ptrs[9] = {v.obstacles.offset, v.obstacles.x, v.obstacles.y, v.dynamic_obstacles.offset, v.dynamic_obstacles.x, v.dynamic_obstacles.y, v.hdv_reachable_sets.offset,
                               v.hdv_reachable_sets.x, v.hdv_reachable_sets.y};
        for (int q = 0; q < 9; ++q) key.p[q] = ptrs[q];
        key.c[0] = v.obstacles.n_polygons;
        key.c[1] = v.dynamic_obstacles.n_polygons;
        key.c[2] = v.hdv_reachable_sets.n_polygons;
        return key;
    }
    static SoupKey boundary_key(const pdmpc_vehicle_in& v) {
        SoupKey key;
        std::memset(&key, 0, sizeof key);
        const void* ptrs[4] = {v.left_x, v.left_y, v.right_x, v.right_y};
        for (int q = 0; q < 4; ++q) key.p[q] = ptrs[q];
        key.c[3] = v.n_left;
        key.c[4] = v.n_right;
        return key;
    }

    // the sets of a vehicle that brings new arrays
    int check_soups(const pdmpc_vehicle_in& v, const pdmpc_polygon_set* fbv) const {
        const int Hp = h->cfg.Hp;
        int rc;
        if ((rc = check_set(v.obstacles, "obstacles"))) return rc;
        if ((rc = check_set(v.dynamic_obstacles, "dynamic_obstacles"))) return rc;
        if ((rc = check_set(v.hdv_reachable_sets, "hdv_reachable_sets"))) return rc;
        if (v.dynamic_obstacles.n_polygons % Hp) return fail(PDMPC_ERR_INVALID, "dynamic_obstacles must hold n_d * Hp polygons");
        if (v.hdv_reachable_sets.n_polygons % Hp) return fail(PDMPC_ERR_INVALID, "hdv_reachable_sets must hold n_h * Hp polygons");
        if (v.n_left < 0 || v.n_right < 0 || v.n_left == 1 || v.n_right == 1) return fail(PDMPC_ERR_INVALID, "lanelet boundary needs 0 or >= 2 points per side");
        if (fbv) {
            if (fbv->n_polygons != Hp) return fail(PDMPC_ERR_INVALID, "fallback_shapes must hold Hp polygons per vehicle");
            if ((rc = check_set(*fbv, "fallback_shapes"))) return rc;
        }
        return PDMPC_OK;
    }

    // the head of a slot's record and its predecessor slots, for the caller's vehicle vi
    int write_head(int vi, DevVehicle& d) {
        const pdmpc_vehicle_in& v = in[vi];
        std::memset(&d, 0, sizeof d);
        d.x0 = v.x0;
        d.y0 = v.y0;
        d.yaw0 = v.yaw0;
        d.trim0 = v.trim0;
        d.seed = seeds ? (*seeds)[(size_t)vi] : 0u;
        for (int k = 0; k < h->cfg.Hp; ++k) {
            d.ref_x[k] = v.ref_x[k];
            d.ref_y[k] = v.ref_y[k];
            d.v_ref[k] = v.v_ref[k];
        }
        const int n_pred = pred_offset ? pred_offset[vi + 1] - pred_offset[vi] : 0;
        d.n_pred = n_pred;
        d.pred_off = (int32_t)n_pred_out;
        for (int q = 0; q < n_pred; ++q) {
            const int ps = pred_index[pred_offset[vi] + q];
            if (ps < 0 || ps >= h->max_vehicles) return fail(PDMPC_ERR_INVALID, "predecessor slot out of range");
            host.pred[n_pred_out++] = !B.perm.empty() && ps < n ? B.inv[(size_t)ps] : ps;
        }
        return PDMPC_OK;
    }

    // a vehicle seen before: the offsets of the slot its arrays were packed in (validated then)
    void share_soups(int slot, int seen_slot, DevVehicle& d) {
        const DevVehicle& f = host.veh[(size_t)seen_slot];
        std::memcpy(d.lit_off, f.lit_off, sizeof d.lit_off);
        std::memcpy(d.hdv_off, f.hdv_off, sizeof d.hdv_off);
        std::memcpy(d.fb_off, f.fb_off, sizeof d.fb_off);
        d.ll_off = f.ll_off;
        d.ll_len = f.ll_len;
        B.lit_cols[(size_t)slot] = B.lit_cols[(size_t)seen_slot];
    }

    // the soups of a vehicle that was not seen before as a whole: each part appended, or taken over from the slot that packed the same
    // arrays (-1: none)
    int append_soups(int slot, const pdmpc_vehicle_in& v, const pdmpc_polygon_set* fbv, DevVehicle& d, int obstacles_of, int boundary_of) {
        const int Hp = h->cfg.Hp;
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        const int n_dyn = v.dynamic_obstacles.n_polygons / Hp;
        const int n_hdv = v.hdv_reachable_sets.n_polygons / Hp;
        if (obstacles_of >= 0) {
            const DevVehicle& f = host.veh[(size_t)obstacles_of];
            std::memcpy(d.lit_off, f.lit_off, sizeof d.lit_off);
            std::memcpy(d.hdv_off, f.hdv_off, sizeof d.hdv_off);
        } else {
            // vehicle_obstacles{k} = [static..., dynamic(:, k)...], each followed by [NaN; NaN]   vectorize_all_obstacles.m:36-62
            for (int k = 0; k < Hp; ++k) {
                d.lit_off[k] = (int32_t)n_pts;
                for (int p = 0; p < v.obstacles.n_polygons; ++p) append_poly(v.obstacles, p, true);
                for (int r = 0; r < n_dyn; ++r) append_poly(v.dynamic_obstacles, r * Hp + k, true);
            }
            d.lit_off[Hp] = (int32_t)n_pts;
            for (int k = 0; k < Hp; ++k) {
                d.hdv_off[k] = (int32_t)n_pts;
                for (int r = 0; r < n_hdv; ++r) append_poly(v.hdv_reachable_sets, r * Hp + k, true);
            }
            d.hdv_off[Hp] = (int32_t)n_pts;
        }
        if (boundary_of >= 0) {
            d.ll_off = host.veh[(size_t)boundary_of].ll_off;
            d.ll_len = host.veh[(size_t)boundary_of].ll_len;
        } else {
            // lanelet_boundary = [left, NaN, right, NaN]                                          vectorize_all_obstacles.m:27-30
            d.ll_off = (int32_t)n_pts;
            for (int q = 0; q < v.n_left; ++q) put(v.left_x[q], v.left_y[q]);
            put(qnan, qnan);
            for (int q = 0; q < v.n_right; ++q) put(v.right_x[q], v.right_y[q]);
            put(qnan, qnan);
            d.ll_len = (int32_t)n_pts - d.ll_off;
        }
        B.lit_cols[(size_t)slot] = (d.lit_off[Hp] - d.lit_off[0]) + d.ll_len;
        if (fbv) {
            for (int k = 0; k < Hp; ++k) {
                d.fb_off[k] = (int32_t)n_pts;
                if (fbv->offset[k + 1] - fbv->offset[k] > PDMPC_VMAX) return fail(PDMPC_ERR_INVALID, "fallback area has more than PDMPC_VMAX columns");
                append_poly(*fbv, k, false);
            }
            d.fb_off[Hp] = (int32_t)n_pts;
        } else {
            for (int k = 0; k <= Hp; ++k) d.fb_off[k] = -1;
        }
        return PDMPC_OK;
    }

    int pack_vehicle(int slot) {
        const int Hp = h->cfg.Hp;
        const int vi = vehicle_of(slot);
        const pdmpc_vehicle_in& v = in[vi];
        if (!v.ref_x || !v.ref_y || !v.v_ref) return fail(PDMPC_ERR_INVALID, "reference trajectory missing");
        if (v.trim0 < 1 || v.trim0 > h->n_trims) return fail(PDMPC_ERR_INVALID, "trim0 out of range");
        const pdmpc_polygon_set* fbv = fallback && fallback[vi].n_polygons > 0 ? &fallback[vi] : nullptr;
        // seen before?  (looked up first: a vehicle that hands over arrays that are packed already needs neither their checks nor room)
        const SoupKey key = soup_key(v, fbv);
        size_t at = 0;
        const int seen_slot = h->soups.find(key, at);
        const pdmpc_vehicle_in* first_in = seen_slot >= 0 ? &in[vehicle_of(seen_slot)] : nullptr;
        const bool shared = first_in && v.left_y == first_in->left_y && v.right_y == first_in->right_y && v.hdv_reachable_sets.y == first_in->hdv_reachable_sets.y;
        int rc;
        if (!shared) {
            if ((rc = check_soups(v, fbv))) return rc;
            // room for everything this vehicle can add (+ the batch's trailing pad)
            const size_t most = (size_t)Hp * set_points(v.obstacles) + set_points(v.dynamic_obstacles) + set_points(v.hdv_reachable_sets) + (size_t)v.n_left + (size_t)v.n_right + 2 +
                                (fbv ? set_points(*fbv) : 0) + 2;
            if ((rc = reserve(most))) return rc;
        }
        DevVehicle& d = host.veh[(size_t)slot];
        if ((rc = write_head(vi, d))) return rc;
        if (shared) {
            share_soups(slot, seen_slot, d);
        } else {
            if (seen_slot < 0) h->soups.insert(key, slot, at);  // (a key met again with other y arrays keeps its first entry, as the map did)
            // the parts it shares with a slot packed before (the first slot that brought a part's arrays is the one entered)
            const SoupKey okey = obstacle_key(v), bkey = boundary_key(v);
            size_t oat = 0, bat = 0;
            const int obstacles_of = h->obstacle_soups.find(okey, oat), boundary_of = h->boundary_soups.find(bkey, bat);
            if (obstacles_of < 0) h->obstacle_soups.insert(okey, slot, oat);
            if (boundary_of < 0) h->boundary_soups.insert(bkey, slot, bat);
            if ((rc = append_soups(slot, v, fbv, d, obstacles_of, boundary_of))) return rc;
        }
        // what the LDS must hold of this vehicle: its soups of all steps with the predecessors' columns (soup_cap), of one step (cand_cap)
        const int need = (d.lit_off[Hp] - d.lit_off[0]) + Hp * d.n_pred * PDMPC_VMAX + (d.hdv_off[Hp] - d.hdv_off[0]) + d.ll_len;
        soup_cap = std::max(soup_cap, need);
        ll_cap = std::max(ll_cap, (int)d.ll_len);
        for (int k = 0; k < Hp; ++k) cand_cap = std::max(cand_cap, (d.lit_off[k + 1] - d.lit_off[k]) + d.n_pred * PDMPC_VMAX + (d.hdv_off[k + 1] - d.hdv_off[k]) + d.ll_len);
        return PDMPC_OK;
    }

    // pad, upload, mark the bank
    int close() {
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        // a trailing pad so 16-byte staged copies never run past the allocation (room: the blob's first 4096 bytes of points, or a vehicle's)
        put(qnan, qnan);
        host.pred[n_pred_out++] = 0;
        B.soup_cap = soup_cap + 2;
        B.ll_cap = ll_cap;
        B.cand_cap = (cand_cap + 4 + 3) & ~3;
        const size_t pts_bytes = (n_pts * 16 + 15) & ~(size_t)15;
        const size_t total = pts_base + pts_bytes;
        if (B.d_blob.ensure(total)) return fail(PDMPC_ERR_HIP, "hipMalloc failed for the batch blob");
        B.host = host;
        B.dev = regions(B.d_blob.p);
        // one copy, not waited for: whatever the stream does next is ordered behind it, and the next pack into this bank waits (pack_common)
        HIPCHK(hipMemcpyAsync(B.d_blob.p, B.h_blob.p, total, hipMemcpyHostToDevice, h->stream));
        B.staged_serial = h->sync_serial;
        B.n_packed = n;
        B.pack_failed = false;
        return PDMPC_OK;
    }
};

}  // namespace

int pack_common(pdmpc_handle* h, int n, const pdmpc_vehicle_in* in, const int32_t* pred_offset, const int32_t* pred_index, const pdmpc_polygon_set* fallback) {
    if (!h) return fail(PDMPC_ERR_INVALID, "null handle");
    // the weights are this pack's, whether it succeeds or not: a failed pack must not leave them to reorder the next one
    const std::vector<double> weights = std::move(h->next_weights);
    h->next_weights.clear();
    // ... and so are the seeds: a pack that fails leaves no sampled bank behind it
    std::vector<uint32_t> seeds;
    const bool sampled = h->sampled.seeds.take(seeds);
    if (!h->has_mpa) return fail(PDMPC_ERR_NO_MPA, "pdmpc_upload_mpa has not been called");
    if (n < 0 || (n > 0 && !in)) return fail(PDMPC_ERR_INVALID, "bad vehicle array");
    if (n > h->max_vehicles) return fail(PDMPC_ERR_CAPACITY, "batch larger than config.max_vehicles");
    PackedStep& B = h->banks[h->bank];
    // the staging blob is reused: a copy out of it that may still be in flight (no stream synchronisation since it was queued) ends first
    if (B.staged_serial == h->sync_serial) HIPCHK(sync_stream(h));
    B.n_packed = 0;  // (a pack that fails leaves the bank empty: the batch that was in it is being overwritten)
    B.pack_failed = true;
    B.sampled = SampledBank{sampled, h->sampled.budget, sampled ? h->sampled.members : 1};
    if (h->sampled.ensemble_bank == h->bank) h->sampled.ensemble_bank = -1;
    if (sampled && (int)seeds.size() != n) return fail(PDMPC_ERR_INVALID, "pdmpc_set_step_seeds: the seeds are not one per vehicle of the packed step");
    Packer P{h, B, n, in, pred_offset, pred_index, fallback, sampled ? &seeds : nullptr};
    int rc;
    if ((rc = P.open())) return rc;
    if ((rc = slot_order(h, n, pred_offset, pred_index, weights, B))) return rc;
    h->soups.reset(n);
    h->obstacle_soups.reset(n);
    h->boundary_soups.reset(n);
    for (int slot = 0; slot < n; ++slot)
        if ((rc = P.pack_vehicle(slot))) return rc;
    if ((rc = P.close())) return rc;
    if ((rc = reserve_sampled_scratch(h, B))) {
        B.n_packed = 0;
        B.pack_failed = true;
        return rc;
    }
    h->timer.reset();
    std::memset(&h->stats, 0, sizeof h->stats);
    return PDMPC_OK;
}
