// step_hdv_checks.cpp — the batch path of the HDV traffic stage (csrc/step_hdv.hpp: gather, call, scatter) against the solo path, as a
// stand-alone program on maps made here.  The device call is a model: for every group pdmpc_hdv_drive_host (if the group drives) and
// pdmpc_hdv_traffic_host on the group's slices of the call's arrays, every result written into the blocks pdmpc_hdv_grouped_layout_host
// names, set_base as running totals, and the capacity protocol of include/pdmpc.h (too small: lists, rows, offsets, totals and adjacency,
// no vertices).  tests/test_gpu_hdv_drive.py pins that the device calls equal the host twins group by group, so the model is the
// reference here, and every index of it into the call's arrays is checked against the array's size.  After scatter every member's
// HdvTraffic must equal, byte for byte, a copy of the member taken through the solo path.  tests/test_step_hdv_stage.py compiles this
// file with csrc/hdv.cpp (and reachable_sets.cpp, whose bounding hdv.cpp calls) under -fsanitize=address,undefined and runs it; it
// prints "step hdv checks ok" last.
#include <cstdio>
#include <cstdlib>

#include "step_hdv.hpp"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static std::string g_error;  // (api.cpp's, which hdv.cpp expects)
extern "C" void pdmpc_set_last_error(const char* msg) { g_error = msg ? msg : ""; }
extern "C" const char* pdmpc_last_error(void) { return g_error.c_str(); }

namespace {
const double PARAMS[4] = {2.0, 0.3, 1.0, 0.125};

// Four lanelets, 0.5 wide, along y = y0: 1 (x = 0, 1, 2) is followed by 2 (x = 2, 3, 4; on the other map 2, 3, 5); 3 -> 4 -> 3 is a
// ring (x = 0, 1, 2 at y = 9 and back at y = 9.5).  Two trims; the hull of (trim t, step k) is a clockwise box (0.4 (k + 1) (t + 1)) x 0.4.
void make_map(HdvTraffic& H, bool other, int Hp) {
    const std::vector<std::vector<double>> xs = {{0.0, 1.0, 2.0}, {2.0, 3.0, other ? 5.0 : 4.0}, {0.0, 1.0, 2.0}, {2.0, 1.0, 0.0}};
    const double y0[4] = {0.0, 0.0, 9.0, 9.5};
    H.lan_off.assign(1, 0);
    for (size_t i = 0; i < xs.size(); ++i) {
        for (double x : xs[i]) {
            H.left_x.push_back(x);
            H.left_y.push_back(y0[i] + 0.25);
            H.right_x.push_back(x);
            H.right_y.push_back(y0[i] - 0.25);
        }
        H.lan_off.push_back((int32_t)H.left_x.size());
    }
    H.succ_off = {0, 1, 1, 2, 3};
    H.succ_idx = {2, 4, 3, 0};  // (one entry more, as pdmpc_controller_set_hdvs leaves it)
    H.rel.assign(16, 0);
    H.n_trims = 2;
    H.local_off.assign(1, 0);
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < Hp; ++k) {
            const double len = 0.4 * (k + 1) * (t + 1);
            for (double x : {0.0, 0.0, len, len}) H.local_x.push_back(x);
            for (double y : {-0.2, 0.2, 0.2, -0.2}) H.local_y.push_back(y);
            H.local_off.push_back((int32_t)H.local_x.size());
        }
}

struct Member {
    HdvTraffic H;
    std::vector<double> cx, cy;
    std::vector<int32_t> lanelet;
    int Hp = 1;
    HdvMember view() { return HdvMember{&H, (int)cx.size(), Hp, 0.2, cx.data(), cy.data(), lanelet.data()}; }
};
// a member with n_hdv HDVs along lanelet 1 (the third on the ring) and n_cav CAVs ahead of them, measured, or with drivers on routes
Member make_member(bool other_map, int n_hdv, int n_cav, int Hp, bool driven) {
    Member m;
    m.Hp = Hp;
    HdvTraffic& H = m.H;
    make_map(H, other_map, Hp);
    H.n = n_hdv;
    H.tile_dx.assign((size_t)n_hdv, 0.0);
    H.tile_dy.assign((size_t)n_hdv, 0.0);
    H.cav_tile_dx.assign((size_t)n_cav, 0.0);
    H.cav_tile_dy.assign((size_t)n_cav, 0.0);
    for (int q = 0; q < n_hdv; ++q) H.trim.push_back(1 + q % 2);
    for (int v = 0; v < n_cav; ++v) {
        m.cx.push_back(1.0 + 0.75 * v);
        m.cy.push_back(0.0);
        m.lanelet.push_back(m.cx.back() < 2.0 ? 1 : 2);
    }
    std::string why;
    if (driven) {
        std::vector<int32_t> off(1, 0), id;
        std::vector<uint8_t> closed;
        std::vector<double> start, v_des;
        for (int q = 0; q < n_hdv; ++q) {
            const bool ring = q == 2;
            for (int l : {ring ? 3 : 1, ring ? 4 : 2}) id.push_back(l);
            off.push_back((int32_t)id.size());
            closed.push_back(ring ? 1 : 0);
            start.push_back(0.25 + 0.5 * q);
            v_des.push_back(0.5 + 0.25 * q);
        }
        CHECK(hdv_set_drivers(H, 0.2, off.data(), id.data(), closed.data(), start.data(), v_des.data(), PARAMS, &why) == PDMPC_OK);
    } else {
        std::vector<double> x, y, yaw;
        for (int q = 0; q < n_hdv; ++q) {
            x.push_back(0.25 + 0.5 * q);
            y.push_back(q == 2 ? 9.0 : 0.0);
            yaw.push_back(0.125 * q);
        }
        CHECK(hdv_set_poses(H, "set_hdv_measurements", "measured", x.data(), y.data(), yaw.data(), nullptr, nullptr, &why) == PDMPC_OK);
    }
    return m;
}

// ---- the model of pdmpc_hdv_traffic_grouped / pdmpc_hdv_drive_traffic_grouped
template <class T>
T& at(std::vector<T>& v, size_t i) {
    CHECK(i < v.size());
    return v[i];
}
struct Model {
    const HdvTraffic* map_in_slot[PDMPC_HDV_MAP_SLOTS] = {};
    int Hp = 1;
    std::vector<size_t> rooms;     // of every call
    std::vector<bool> with_drive;  // ... and whether it was the call with the drive pass

    int operator()(HdvCallScratch& C, bool any_drives) {
        rooms.push_back(C.set_x.size());
        with_drive.push_back(any_drives);
        const size_t G = C.n_rows.size(), n_all = (size_t)at(C.hdv_offset, G);
        CHECK(C.slot.size() == G && C.drives.size() == G && C.dt.size() == G && C.params.size() == 4 * G && C.set_base.size() == G + 1);
        struct Sets {
            std::vector<double> x, y;
            std::vector<uint8_t> flags;
        };
        std::vector<Sets> sets(G);
        int32_t base = 0;
        for (size_t g = 0; g < G; ++g) {
            CHECK(C.slot[g] >= 0 && C.slot[g] < PDMPC_HDV_MAP_SLOTS && map_in_slot[C.slot[g]]);
            const HdvTraffic& map = *map_in_slot[C.slot[g]];
            const size_t h0 = (size_t)C.hdv_offset[g], nh = (size_t)C.hdv_offset[g + 1] - h0, c0 = (size_t)at(C.cav_offset, g), nc = (size_t)at(C.cav_offset, g + 1) - c0;
            CHECK(nh > 0 && nc > 0);  // (the cases here: a slice's first entry is taken by reference)
            if (any_drives && C.drives[g]) {
                std::vector<int32_t> off, seg(2 * nh), new_seg(2 * nh);
                std::vector<double> new_u(nh), x(nh), y(nh), cs(nh), sn(nh), speed(nh), gap(nh);
                for (size_t q = 0; q <= nh; ++q) off.push_back(at(C.route_off, h0 + q) - C.route_off[h0]);
                for (size_t q = 0; q < nh; ++q) {
                    seg[q] = at(C.seg, h0 + q);
                    seg[nh + q] = at(C.seg, n_all + h0 + q);
                }
                CHECK((size_t)C.route_off[h0] + (size_t)off[nh] < C.route_id.size() && h0 + nh <= C.route_closed.size() && h0 + nh <= C.u.size() && h0 + nh <= C.v_des.size());
                const int rc = hdv_with_lanelets(map, [&](auto... lanelets) {
                    return pdmpc_hdv_drive_host(lanelets..., (int32_t)nh, off.data(), &C.route_id[(size_t)C.route_off[h0]], &C.route_closed[h0], seg.data(), &C.u[h0], &at(C.tile_dx, h0),
                                                &at(C.tile_dy, h0), &C.v_des[h0], (int32_t)nc, &at(C.cav_x, c0), &at(C.cav_y, c0), &at(C.cav_tile_dx, c0), &at(C.cav_tile_dy, c0),
                                                &C.params[4 * g], C.dt[g], new_seg.data(), new_u.data(), x.data(), y.data(), cs.data(), sn.data(), speed.data(), gap.data());
                });
                CHECK(rc == PDMPC_OK);
                for (size_t q = 0; q < nh; ++q) {
                    at(C.new_seg, h0 + q) = new_seg[q];
                    at(C.new_seg, n_all + h0 + q) = new_seg[nh + q];
                    at(C.new_u, h0 + q) = new_u[q];
                    at(C.speed, h0 + q) = speed[q];
                    at(C.gap, h0 + q) = gap[q];
                    at(C.x, h0 + q) = x[q];
                    at(C.y, h0 + q) = y[q];
                    at(C.cos_yaw, h0 + q) = cs[q];
                    at(C.sin_yaw, h0 + q) = sn[q];
                }
            }
            // the group's own traffic call, with arrays of its own: sized by a first call without room
            const size_t lists = nh * PDMPC_HDV_MAX_CHAINS;
            std::vector<int32_t> closest_off(nh + 1), closest_idx(lists), row_hdv(lists), set_off(lists * Hp + 1);
            std::vector<uint8_t> adjacency(nc * nh);
            Sets& S = sets[g];
            S.flags.resize(lists * Hp);
            int32_t n_rows = 0;
            CHECK(h0 + nh <= C.y.size() && h0 + nh <= C.cos_yaw.size() && h0 + nh <= C.sin_yaw.size() && h0 + nh <= C.trim.size() && c0 + nc <= C.cav_lanelet.size());
            auto traffic = [&]() {
                return hdv_with_map(map, Hp, [&](auto... m) {
                    return pdmpc_hdv_traffic_host(m..., (int32_t)nh, &at(C.x, h0), &C.y[h0], &C.cos_yaw[h0], &C.sin_yaw[h0], &C.trim[h0], &C.tile_dx[h0], &C.tile_dy[h0], (int32_t)nc,
                                                  &C.cav_x[c0], &C.cav_y[c0], &C.cav_lanelet[c0], &C.cav_tile_dx[c0], &C.cav_tile_dy[c0], closest_off.data(), closest_idx.data(),
                                                  (int32_t)S.x.size(), &n_rows, row_hdv.data(), set_off.data(), S.x.data(), S.y.data(), S.flags.data(), adjacency.data());
                });
            };
            int rc = traffic();
            if (rc == PDMPC_ERR_CAPACITY) {
                CHECK(n_rows >= 0);
                S.x.resize((size_t)set_off[(size_t)n_rows * Hp]);
                S.y.resize(S.x.size());
                rc = traffic();
            }
            CHECK(rc == PDMPC_OK);
            const size_t n_sets = (size_t)n_rows * Hp;
            S.x.resize((size_t)set_off[n_sets]);
            S.y.resize(S.x.size());
            S.flags.resize(n_sets);
            for (size_t i = 0; i <= nh; ++i) at(C.closest_off, (size_t)at(C.closest_at, g) + i) = closest_off[i];
            for (size_t i = 0; i < (size_t)closest_off[nh]; ++i) at(C.closest_idx, (size_t)at(C.list_at, g) + i) = closest_idx[i];
            for (size_t r = 0; r < (size_t)n_rows; ++r) at(C.row_hdv, (size_t)C.list_at[g] + r) = row_hdv[r];
            for (size_t o = 0; o <= n_sets; ++o) at(C.set_off, (size_t)at(C.set_offset_at, g) + o) = set_off[o];
            for (size_t i = 0; i < nc * nh; ++i) at(C.adjacency, (size_t)at(C.adjacency_at, g) + i) = adjacency[i];
            C.n_rows[g] = n_rows;
            C.set_base[g] = base;
            base += set_off[n_sets];
        }
        C.set_base[G] = base;
        if ((size_t)base > C.set_x.size() || C.set_y.size() != C.set_x.size()) return PDMPC_ERR_CAPACITY;
        for (size_t g = 0; g < G; ++g) {
            for (size_t i = 0; i < sets[g].x.size(); ++i) {
                at(C.set_x, (size_t)C.set_base[g] + i) = sets[g].x[i];
                at(C.set_y, (size_t)C.set_base[g] + i) = sets[g].y[i];
            }
            for (size_t o = 0; o < sets[g].flags.size(); ++o) at(C.set_flags, (size_t)at(C.set_at, g) + o) = sets[g].flags[o];
        }
        return PDMPC_OK;
    }
};

// ---- the comparison: what pdmpc_controller_hdv_info and _hdv_driver_state hand out, and the sets the CAVs' searches receive
template <class T>
bool same_front(const std::vector<T>& a, const std::vector<T>& b, size_t count) {
    return a.size() >= count && b.size() >= count && (count == 0 || !std::memcmp(a.data(), b.data(), count * sizeof(T)));
}
void check_same(const Member& A, const Member& B) {
    const HdvTraffic &a = A.H, &b = B.H;
    const size_t n = (size_t)a.n, nc = A.cx.size();
    CHECK(a.n_rows == b.n_rows && a.n_rows >= 0);
    const size_t rows = (size_t)a.n_rows, n_sets = rows * A.Hp;
    CHECK(same_front(a.closest_off, b.closest_off, n + 1) && same_front(a.closest_idx, b.closest_idx, (size_t)a.closest_off[n]));
    CHECK(same_front(a.row_hdv, b.row_hdv, rows) && same_front(a.set_off, b.set_off, n_sets + 1));
    CHECK(same_front(a.set_flags, b.set_flags, n_sets) && same_front(a.adjacency, b.adjacency, nc * n) && a.adjacency.size() == nc * n && b.adjacency.size() == nc * n);
    const size_t total = (size_t)a.set_off[n_sets];
    CHECK(same_front(a.set_x, b.set_x, total) && same_front(a.set_y, b.set_y, total));
    CHECK(a.cav_off.size() == nc && b.cav_off.size() == nc && a.cav_x.size() == nc && b.cav_x.size() == nc && a.cav_y.size() == nc && b.cav_y.size() == nc);
    for (size_t v = 0; v < nc; ++v) CHECK(same_bytes(a.cav_off[v], b.cav_off[v]) && same_bytes(a.cav_x[v], b.cav_x[v]) && same_bytes(a.cav_y[v], b.cav_y[v]));
    CHECK(a.x.size() == n && same_bytes(a.x, b.x) && same_bytes(a.y, b.y) && same_bytes(a.cos_yaw, b.cos_yaw) && same_bytes(a.sin_yaw, b.sin_yaw) && same_bytes(a.yaw, b.yaw));
    CHECK(a.driven == b.driven && a.driven_builds == b.driven_builds && a.measured && b.measured);
    if (a.driven) CHECK(a.seg.size() == 2 * n && same_bytes(a.seg, b.seg) && a.u.size() == n && same_bytes(a.u, b.u) && same_bytes(a.speed, b.speed) && same_bytes(a.gap, b.gap));
}

// One built step of the members `ms` as ONE grouped call, against copies of them taken through the solo path.  want_drives: which of
// them move their HDVs this step; floor: the least room of the call's vertex arrays; calls: how often the call is made.
size_t run_case(const char* name, std::vector<Member>& ms, const std::vector<int>& want_drives, size_t floor, size_t calls) {
    const size_t M = ms.size();
    std::vector<uint8_t> drives(M);
    std::vector<int32_t> n_hdv(M);
    for (size_t m = 0; m < M; ++m) {
        drives[m] = hdv_begin_build(ms[m].H) ? 1 : 0;
        CHECK(drives[m] == want_drives[m]);
        n_hdv[m] = ms[m].H.n;
    }
    std::vector<Member> solo = ms;
    std::string why;
    for (size_t m = 0; m < M; ++m) CHECK(hdv_solo_step(solo[m].view(), drives[m] != 0, &why) == PDMPC_OK);
    // the batch and its map slots: slot 0 holds somebody else's map, so the maps take the slots 1, 2, ... in member order
    std::vector<HdvBatch> batches = hdv_split_batches((int)M, n_hdv.data(), [&](int a, int b) { return same_hdv_map(ms[(size_t)a].H, ms[(size_t)b].H); });
    CHECK(batches.size() == 1 && batches[0].members.size() == M);
    HdvBatch& B = batches[0];
    std::vector<HdvSlotNote> note(M);
    const int64_t generation[PDMPC_HDV_MAP_SLOTS] = {7, 0, 0, 0, 0, 0, 0, 0};
    CHECK(hdv_assign_slots(B, note.data(), generation, [](int, int) { return false; }) == (int)B.maps.size());
    Model model;
    model.Hp = ms[0].Hp;
    for (size_t d = 0; d < B.maps.size(); ++d) {
        CHECK(B.slot[d] == (int32_t)d + 1 && B.upload[d]);
        model.map_in_slot[B.slot[d]] = &ms[(size_t)B.maps[d]].H;
    }
    std::vector<HdvMember> views;
    for (Member& m : ms) views.push_back(m.view());
    HdvCallScratch C;
    bool any_drives = false;
    CHECK(hdv_gather_batch(views.data(), B, drives.data(), C, &any_drives, floor) == PDMPC_OK);
    CHECK(any_drives == (*std::max_element(drives.begin(), drives.end()) != 0) && C.drives == drives);
    for (size_t g = 0; g < M; ++g) {  // the routes of a member that does not move: none, the offsets flat over its HDVs
        const size_t h0 = (size_t)C.hdv_offset[g], h1 = (size_t)C.hdv_offset[g + 1];
        CHECK(drives[g] ? C.route_off[h1] - C.route_off[h0] == 2 * ms[g].H.n : C.route_off[h1] == C.route_off[h0]);
        CHECK(C.slot[g] == B.slot[(size_t)B.map_of[g]]);
    }
    CHECK(hdv_call_batch(C, any_drives, model) == PDMPC_OK);
    CHECK(model.rooms.size() == calls && model.rooms[0] == floor);
    for (bool d : model.with_drive) CHECK(d == any_drives);
    const size_t need = (size_t)C.set_base[M];
    if (calls == 2) CHECK(model.rooms[0] == floor && need > floor && model.rooms[1] == need + need / 4 && C.set_x.size() == need + need / 4);
    hdv_scatter_batch(views.data(), B, C);
    for (size_t m = 0; m < M; ++m) check_same(ms[m], solo[m]);
    std::printf("%-48s %zu members, %d maps, %s, %zu call(s), %zu vertices\n", name, M, (int)B.maps.size(), any_drives ? "drive + traffic" : "traffic", calls, need);
    return need;
}

// the three members of unequal sizes: (HDVs, CAVs) = (2, 3), (1, 1), (3, 2); members 0 and 2 share a map, member 1 has the other
std::vector<Member> three(int Hp, bool d0, bool d1, bool d2) { return {make_member(false, 2, 3, Hp, d0), make_member(true, 1, 1, Hp, d1), make_member(false, 3, 2, Hp, d2)}; }
}  // namespace

int main() {
    {
        std::vector<Member> one = {make_member(false, 1, 1, 1, false)};
        CHECK(run_case("one member, 1 HDV, 1 CAV, Hp 1", one, {0}, HDV_ROOM_FLOOR, 1) > 0);
    }
    for (int Hp : {1, 3}) {
        std::vector<Member> ms = three(Hp, false, false, false);
        CHECK(!same_hdv_map(ms[0].H, ms[1].H) && same_hdv_map(ms[0].H, ms[2].H));
        CHECK(run_case(Hp == 1 ? "three members, measured, Hp 1" : "three members, measured, Hp 3", ms, {0, 0, 0}, HDV_ROOM_FLOOR, 1) > 0);
    }
    {
        // drivers on members 0 and 2: the first built step is the placement (the traffic call is chosen), every further one drives
        std::vector<Member> ms = three(3, true, false, true);
        run_case("members 0 and 2 with drivers, first step", ms, {0, 0, 0}, HDV_ROOM_FLOOR, 1);
        run_case("members 0 and 2 with drivers, mixed call", ms, {1, 0, 1}, HDV_ROOM_FLOOR, 1);
        run_case("members 0 and 2 with drivers, again", ms, {1, 0, 1}, HDV_ROOM_FLOOR, 1);
        std::vector<Member> all = three(3, true, true, true);
        run_case("all with drivers, first step", all, {0, 0, 0}, HDV_ROOM_FLOOR, 1);
        run_case("all with drivers, all drive", all, {1, 1, 1}, HDV_ROOM_FLOOR, 1);
    }
    {
        // a member on its first built step after its drivers were set beside one on its second
        std::vector<Member> ms = {make_member(false, 2, 3, 1, true), make_member(false, 3, 2, 1, true)};
        CHECK(!hdv_begin_build(ms[1].H) && ms[1].H.driven_builds == 1);
        run_case("first built step beside a second", ms, {0, 1}, HDV_ROOM_FLOOR, 1);
    }
    {
        // the retry: room for 8 vertices, so the call is made twice, the second time with the total and a quarter
        std::vector<Member> ms = three(3, true, false, true);
        run_case("the retry, traffic call", ms, {0, 0, 0}, 8, 2);
        run_case("the retry, mixed call", ms, {1, 0, 1}, 8, 2);
    }
    std::printf("step hdv checks ok\n");
    return 0;
}
