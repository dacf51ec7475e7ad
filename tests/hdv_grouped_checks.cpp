// hdv_grouped_checks.cpp — the host-only rules of the grouped HDV traffic call (csrc/hdv_grouped_host.hpp, csrc/hdv_host.hpp) as a
// stand-alone program: the layout of the groups' blocks against sums written out here, the batches of a lock-step and their map slots
// against a model of a handle (eight slots that hold a map id and a generation), the byte-for-byte content check of a slot, and the
// plan of the HDV device calls (csrc/hdv_call_host.hpp): the workspace layout, the argument records, stage and scatter on heap blocks
// of exactly the computed sizes, and the refusals of the checks with their texts.
// tests/test_hdv_grouped_host.py compiles it with -fsanitize=address,undefined and runs it; it prints "hdv grouped checks ok" last.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hdv_call_host.hpp"
#include "hdv_grouped_host.hpp"
#include "hdv_host.hpp"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

namespace {
const int C = PDMPC_HDV_MAX_CHAINS;

void check_layout(int Hp) {
    const int nh[4] = {2, 0, 1, 3}, nc[4] = {3, 4, 0, 1};
    std::vector<int32_t> ho(5, 0), co(5, 0);
    for (int g = 0; g < 4; ++g) {
        ho[g + 1] = ho[g] + nh[g];
        co[g + 1] = co[g] + nc[g];
    }
    // exactly n_groups + 1 entries each: the sanitizer sees a write behind them
    std::vector<int32_t> closest(5), lists(5), set_off(5), sets(5);
    std::vector<int64_t> adj(5);
    CHECK(hdv_grouped_layout(4, ho.data(), co.data(), Hp, closest.data(), lists.data(), set_off.data(), sets.data(), adj.data()) == PDMPC_OK);
    int h0 = 0;
    int64_t pairs = 0;
    for (int g = 0; g <= 4; ++g) {
        CHECK(closest[g] == h0 + g);
        CHECK(lists[g] == h0 * C);
        CHECK(set_off[g] == h0 * C * Hp + g);
        CHECK(sets[g] == h0 * C * Hp);
        CHECK(adj[g] == pairs);
        if (g < 4) {
            pairs += (int64_t)nc[g] * nh[g];
            h0 += nh[g];
        }
    }
    CHECK(adj[4] == 2 * 3 + 0 + 0 + 3 * 1);
    // any output may be absent; no group at all
    CHECK(hdv_grouped_layout(4, ho.data(), co.data(), Hp, nullptr, nullptr, nullptr, nullptr, adj.data()) == PDMPC_OK);
    int32_t one[1] = {-1}, zero[1] = {0};
    int64_t one64[1] = {-1};
    CHECK(hdv_grouped_layout(0, zero, zero, Hp, one, nullptr, nullptr, nullptr, one64) == PDMPC_OK && one[0] == 0 && one64[0] == 0);
    // refusals
    std::vector<int32_t> down = {0, 2, 1};
    CHECK(hdv_grouped_layout(2, down.data(), co.data(), Hp, nullptr, nullptr, nullptr, nullptr, nullptr) == PDMPC_ERR_INVALID);
    CHECK(hdv_grouped_layout(2, ho.data(), down.data(), Hp, nullptr, nullptr, nullptr, nullptr, nullptr) == PDMPC_ERR_INVALID);
    CHECK(hdv_grouped_layout(-1, ho.data(), co.data(), Hp, nullptr, nullptr, nullptr, nullptr, nullptr) == PDMPC_ERR_INVALID);
    CHECK(hdv_grouped_layout(2, nullptr, co.data(), Hp, nullptr, nullptr, nullptr, nullptr, nullptr) == PDMPC_ERR_INVALID);
    std::vector<int32_t> from_one = {1, 2, 3};
    CHECK(hdv_grouped_layout(2, from_one.data(), co.data(), Hp, nullptr, nullptr, nullptr, nullptr, nullptr) == PDMPC_ERR_INVALID);
}

// a handle as the batching rule sees it: what every slot holds (a map id, 0: nothing) and its generation
struct Model {
    int content[PDMPC_HDV_MAP_SLOTS] = {};
    int64_t generation[PDMPC_HDV_MAP_SLOTS] = {};
    int64_t next = 0;
    int uploads = 0, checks = 0;
};
// one lock-step of members with the maps map_id[m] and n_hdv[m] HDVs: split, assign, upload, note -- what hdv_traffic_stage does
std::vector<HdvBatch> lock_step(Model& H, const std::vector<int>& map_id, const std::vector<int32_t>& n_hdv, std::vector<HdvSlotNote>& note) {
    const int M = (int)map_id.size();
    std::vector<HdvBatch> batches = hdv_split_batches(M, n_hdv.data(), [&](int a, int b) { return map_id[(size_t)a] == map_id[(size_t)b]; });
    H.uploads = H.checks = 0;
    for (HdvBatch& B : batches) {
        H.checks += hdv_assign_slots(B, note.data(), H.generation, [&](int slot, int m) { return H.content[slot] == map_id[(size_t)m]; });
        bool used[PDMPC_HDV_MAP_SLOTS] = {};
        for (size_t d = 0; d < B.maps.size(); ++d) {
            CHECK(B.slot[d] >= 0 && B.slot[d] < PDMPC_HDV_MAP_SLOTS && !used[B.slot[d]]);  // every distinct map a slot of its own
            used[B.slot[d]] = true;
            if (B.upload[d]) {
                H.content[B.slot[d]] = map_id[(size_t)B.maps[d]];
                H.generation[B.slot[d]] = ++H.next;
                H.uploads += 1;
            }
            CHECK(H.content[B.slot[d]] == map_id[(size_t)B.maps[d]]);  // the slot holds the map when the call is made
        }
        for (size_t i = 0; i < B.members.size(); ++i) {
            const int32_t s = B.slot[(size_t)B.map_of[i]];
            CHECK(H.content[s] == map_id[(size_t)B.members[i]]);
            note[(size_t)B.members[i]] = HdvSlotNote{s, H.generation[s]};
        }
    }
    return batches;
}

void check_batches() {
    {  // 9 distinct maps: 8 + 1, slots in member order on a fresh handle
        Model H;
        std::vector<int> ids = {1, 2, 3, 4, 5, 6, 7, 8, 9};
        std::vector<int32_t> n(9, 2);
        std::vector<HdvSlotNote> note(9);
        std::vector<HdvBatch> b = lock_step(H, ids, n, note);
        CHECK(b.size() == 2 && b[0].members.size() == 8 && b[1].members.size() == 1 && b[1].members[0] == 8);
        for (int d = 0; d < 8; ++d) CHECK(b[0].slot[(size_t)d] == d && b[0].upload[(size_t)d]);
        CHECK(H.uploads == 9);
        CHECK(b[1].slot[0] == PDMPC_HDV_MAP_SLOTS - 1 && b[1].upload[0]);  // no slot is free: the last one goes first, slot 0 last
    }
    {  // 60, 60 and 60 HDVs: 120 + 60, whatever the maps
        Model H;
        std::vector<int> ids = {1, 1, 1};
        std::vector<int32_t> n = {60, 60, 60};
        std::vector<HdvSlotNote> note(3);
        std::vector<HdvBatch> b = lock_step(H, ids, n, note);
        CHECK(b.size() == 2 && b[0].n_hdv == 120 && b[1].n_hdv == 60 && b[0].members.size() == 2);
        CHECK(H.uploads == 1);  // (the second batch finds the map of the first resident)
    }
    {  // equal maps share a slot; members without HDVs take no part; a resident map costs no upload and, noted, no check
        Model H;
        std::vector<int> ids = {1, 0, 1, 2, 0};
        std::vector<int32_t> n = {2, 0, 1, 3, 0};
        std::vector<HdvSlotNote> note(5);
        std::vector<HdvBatch> b = lock_step(H, ids, n, note);
        CHECK(b.size() == 1 && b[0].members == std::vector<int>({0, 2, 3}) && b[0].map_of == std::vector<int>({0, 0, 1}) && b[0].maps == std::vector<int>({0, 3}));
        CHECK(H.uploads == 2 && H.checks == 0 && note[0].slot == 0 && note[2].slot == 0 && note[3].slot == 1 && note[1].slot == -1);
        b = lock_step(H, ids, n, note);
        CHECK(b.size() == 1 && H.uploads == 0 && H.checks == 0);
        // a moved generation forces the content check: the same map uploaded again into slot 0 by somebody else ...
        H.generation[0] = ++H.next;
        b = lock_step(H, ids, n, note);
        CHECK(H.uploads == 0 && H.checks >= 1 && note[0].generation == H.generation[0] && note[2].slot == 0);
        b = lock_step(H, ids, n, note);
        CHECK(H.uploads == 0 && H.checks == 0);
        // ... and another map: the check fails and the member's map is uploaded, into a slot that was never used, not over map 2
        H.content[0] = 7;
        H.generation[0] = ++H.next;
        b = lock_step(H, ids, n, note);
        CHECK(H.uploads == 1 && H.checks >= 1 && note[0].slot == 2 && note[2].slot == 2 && note[3].slot == 1);
        // a newcomer with a resident map and no note: found by the check, not uploaded
        std::vector<int> ids2 = {2};
        std::vector<int32_t> n2 = {1};
        std::vector<HdvSlotNote> note2(1);
        b = lock_step(H, ids2, n2, note2);
        CHECK(H.uploads == 0 && H.checks >= 1 && note2[0].slot == 1);
    }
    {  // two controllers with different maps that take turns on one handle: after their first steps no upload, no check
        Model H;
        std::vector<HdvSlotNote> a(1), b(1);
        for (int turn = 0; turn < 3; ++turn) {
            lock_step(H, {1}, {2}, a);
            CHECK(H.uploads == (turn == 0) && (turn == 0 || H.checks == 0));
            lock_step(H, {2}, {2}, b);
            CHECK(H.uploads == (turn == 0) && a[0].slot == 0 && b[0].slot == 1);
        }
    }
    {  // a member above the limit of a call still gets a batch of its own (the call refuses it)
        Model H;
        std::vector<HdvSlotNote> note(2);
        std::vector<HdvBatch> b = lock_step(H, {1, 1}, {1, 200}, note);
        CHECK(b.size() == 2 && b[1].n_hdv == 200);
    }
}

void check_content() {
    // two lanelets of 2 and 3 points, the caller's arrays with a gap in front (offsets that do not start at 0)
    std::vector<int32_t> lo = {1, 3, 6}, so = {0, 1, 1}, si = {2};
    std::vector<double> lx = {9, 0, 1, 1, 2, 3}, ly = {9, .5, .5, .5, .5, .5}, rx = lx, ry = {9, -.5, -.5, -.5, -.5, -.5};
    std::vector<uint8_t> rel = {0, 1, 0, 0};
    std::vector<int32_t> poff = {0, 3, 7};
    std::vector<double> px = {0, 1, 1, 0, 2, 2, 0}, py = {0, 0, 1, 0, 0, 2, 2};
    pdmpc_polygon_set sets{};
    sets.n_polygons = 2;
    sets.offset = poff.data();
    sets.x = px.data();
    sets.y = py.data();
    HdvSlotData S;
    const char* why = nullptr;
    CHECK(S.map.points(2, lo.data(), lo.data(), lx.data(), ly.data(), rx.data(), ry.data(), &why) == PDMPC_OK);
    CHECK(S.map.graph(so.data(), si.data(), rel.data(), &why) == PDMPC_OK);
    CHECK(hdv_check_sets(1, 2, &sets, &why) == PDMPC_OK);
    S.keep_sets(1, 2, &sets);
    auto holds = [&]() { return S.holds(2, lo.data(), lo.data(), lx.data(), ly.data(), rx.data(), ry.data(), so.data(), si.data(), rel.data(), 1, 2, &sets); };
    CHECK(holds());
    // the same content at other offsets is the same map
    std::vector<int32_t> lo0 = {0, 2, 5};
    std::vector<double> lx0(lx.begin() + 1, lx.end()), ly0(ly.begin() + 1, ly.end()), ry0(ry.begin() + 1, ry.end());
    CHECK(S.holds(2, lo0.data(), lo0.data(), lx0.data(), ly0.data(), lx0.data(), ry0.data(), so.data(), si.data(), rel.data(), 1, 2, &sets));
    // one bit anywhere is another map: a point, a sign of zero, a successor, a relationship, a hull vertex, the table's shape
    ly[2] = 0.5000000000000001;
    CHECK(!holds());
    ly[2] = 0.5;
    lx[1] = -0.0;
    CHECK(!holds());
    lx[1] = 0.0;
    si[0] = 1;
    CHECK(!holds());
    si[0] = 2;
    rel[1] = 3;
    CHECK(!holds());
    rel[1] = 1;
    py[6] = 2.5;
    CHECK(!holds());
    py[6] = 2;
    CHECK(holds());
    CHECK(!S.holds(2, lo.data(), lo.data(), lx.data(), ly.data(), rx.data(), ry.data(), so.data(), si.data(), rel.data(), 2, 1, &sets));
    CHECK(!S.holds(1, lo.data(), lo.data(), lx.data(), ly.data(), rx.data(), ry.data(), so.data(), si.data(), rel.data(), 1, 2, &sets));
}
// ---- the plan of the device calls (csrc/hdv_call_host.hpp): workspace layout, arguments, stage and scatter, refusals

enum Part { IN, DEV, OUT };  // the inputs, the device-only regions, what is read back
struct Region {
    const char* name;
    size_t at, count, size, align;
    Part part;
};
// every region of the workspace with the number of its elements counted here, not by the function under test
std::vector<Region> regions(const HdvWs& L, int G, int n, int nc, size_t pairs, int Hp, int cap, int n_route) {
    const size_t N = (size_t)n, NC = (size_t)nc, lists = N * 16, slots = lists * (size_t)Hp;  // 16 = PDMPC_HDV_MAX_CHAINS
    const bool grouped = G > 0, drive = n_route >= 0;
    const size_t g = (size_t)G, gn = grouped ? N : 0, g1 = grouped ? g + 1 : 0, dn = drive ? N : 0, dg = drive ? g : 0;
    return {{"in", L.in, 6 * N, 8, 8, IN},
            {"cav", L.cav, 4 * NC, 8, 8, IN},
            {"trim", L.trim, N, 4, 4, IN},
            {"cav_lanelet", L.cav_lanelet, NC, 4, 4, IN},
            {"groups", L.groups, g, 20, 4, IN},  // five int32 each
            {"group_of", L.group_of, gn, 4, 4, IN},
            {"pair_first", L.pair_first, g1, 4, 4, IN},
            {"drives", L.drives, dg, 1, 1, IN},
            {"route_off", L.route_off, drive ? N + 1 : 0, 4, 4, IN},
            {"route_id", L.route_id, drive ? (size_t)n_route : 0, 4, 4, IN},
            {"closed", L.closed, dn, 1, 1, IN},
            {"state_seg", L.state_seg, 2 * dn, 4, 4, IN},
            {"state_u", L.state_u, dn, 8, 8, IN},
            {"v_des", L.v_des, dn, 8, 8, IN},
            {"params", L.params, 5 * dg, 8, 8, IN},
            {"n_chains", L.n_chains, N, 4, 4, DEV},
            {"chain_id", L.chain_id, lists, 4, 4, DEV},
            {"chain_succ", L.chain_succ, lists, 4, 4, DEV},
            {"slot_n", L.slot_n, slots, 4, 4, DEV},
            {"slot_flags", L.slot_flags, slots, 1, 1, DEV},
            {"slot_before", L.slot_before, grouped ? slots : 0, 4, 4, DEV},
            {"row_base", L.row_base, gn, 4, 4, DEV},
            {"status", L.status, 2, 4, 4, OUT},
            {"n_rows", L.n_rows, g, 4, 4, OUT},
            {"set_base", L.set_base, g1, 4, 4, OUT},
            {"n_closest", L.n_closest, N, 4, 4, OUT},
            {"closest", L.closest, lists, 4, 4, OUT},
            {"row_hdv", L.row_hdv, lists, 4, 4, OUT},
            {"set_off", L.set_off, slots + g + 1, 4, 4, OUT},
            {"set_flags", L.set_flags, slots, 1, 1, OUT},
            {"adjacency", L.adjacency, pairs, 1, 1, OUT},
            {"new_seg", L.new_seg, 2 * dn, 4, 4, OUT},
            {"new_u", L.new_u, dn, 8, 8, OUT},
            {"speed", L.speed, dn, 8, 8, OUT},
            {"gap", L.gap, dn, 8, 8, OUT},
            {"pose", L.pose, 4 * dn, 8, 8, OUT},
            {"set_xy", L.set_xy, 2 * (size_t)cap, 8, 8, OUT}};
}

HdvPlan plan_of(int n, int nc, size_t pairs, int Hp, int cap, int n_route = -1) {
    HdvPlan P;
    P.n = n, P.nc = nc, P.pairs = (int64_t)pairs, P.Hp = Hp, P.cap = cap, P.n_route = n_route;
    return P;
}

void check_ws(int G, int n, int nc, size_t pairs, int Hp, int cap, int n_route) {
    const HdvWs L = hdv_ws(G, plan_of(n, nc, pairs, Hp, cap, n_route));
    const std::vector<Region> R = regions(L, G, n, nc, pairs, Hp, cap, n_route);
    CHECK(L.in_bytes <= L.out && L.out <= L.total && L.in_bytes % 8 == 0 && L.out % 8 == 0);
    size_t sum[3] = {0, 0, 0}, count[3] = {0, 0, 0};
    for (size_t i = 0; i < R.size(); ++i) {
        const size_t first = R[i].at, last = first + R[i].count * R[i].size;
        const size_t lo = R[i].part == IN ? 0 : R[i].part == DEV ? L.in_bytes : L.out, hi = R[i].part == IN ? L.in_bytes : R[i].part == DEV ? L.out : L.total;
        CHECK(first % R[i].align == 0);
        CHECK(lo <= first && last <= hi);
        for (size_t j = 0; j < i; ++j) {
            const size_t other = R[j].at, other_last = other + R[j].count * R[j].size;
            CHECK(first == last || other == other_last || last <= other || other_last <= first);
        }
        sum[R[i].part] += last - first;
        count[R[i].part] += 1;
    }
    // the sizes: the sums of the regions and alignment padding only (less than 8 bytes in front of a region or the end)
    const size_t size[3] = {L.in_bytes, L.out - L.in_bytes, L.total - L.out};
    for (int p = 0; p < 3; ++p) CHECK(size[p] >= sum[p] && size[p] < sum[p] + 8 * (count[p] + 1));
}

void check_workspace() {
    const int nh[4] = {2, 0, 1, 3}, nc[4] = {3, 4, 0, 1};
    size_t pairs = 0;
    int n = 0, c = 0;
    for (int g = 0; g < 4; ++g) {
        pairs += (size_t)nc[g] * nh[g];
        n += nh[g];
        c += nc[g];
    }
    for (int Hp : {1, 6})
        for (int n_route : {-1, 0, 13})
            for (int cap : {0, 1, 77}) check_ws(4, n, c, pairs, Hp, cap, n_route);
    for (int Hp : {1, 6})
        for (int one : {1, 3})
            for (int cavs : {0, 2})
                for (int cap : {0, 5}) check_ws(0, one, cavs, (size_t)cavs * one, Hp, cap, -1);
    // two layouts byte by byte.  The ungrouped call of 1 HDV, no CAV, Hp 1, no room: inputs 6 doubles + 1 trim = 52 -> 56; device only
    // 4 + 64 + 64 + 64 + 16 = 212 -> out at 272; read back 8 + 4 + 64 + 64 + 17 * 4 + 16 = 224
    HdvWs L = hdv_ws(0, plan_of(1, 0, 0, 1, 0));
    CHECK(L.in_bytes == 56 && L.out == 272 && L.total == 496 && L.trim == 48 && L.status == 272 && L.set_xy == 496);
    // one group of 1 HDV and 1 CAV that drives, Hp 1, room for 2 vertices, a route of 3: inputs 48 + 32 + 4 + 4 + 20 + 4 + 8 + 1 (-> 124)
    // + 8 + 12 + 1 (-> 148) + 8 (-> 160) + 8 + 8 + 40 = 216; device only 212 + 64 + 4 = 280; read back 8 + 4 + 8 + 4 + 64 + 64 + 18 * 4 + 16
    // + 1 (-> 244) + 8 (-> 256) + 8 + 8 + 8 + 32 + 32 = 344
    L = hdv_ws(1, plan_of(1, 1, 1, 1, 2, 3));
    CHECK(L.in_bytes == 216 && L.out == 496 && L.total == 840 && L.route_off == 124 && L.state_u == 160 && L.params == 176 && L.new_seg == 496 + 244 && L.new_u == 496 + 256);
}

void check_arguments() {
    const HdvPlan P = plan_of(6, 8, 9, 1, 100, 12);
    const HdvWs L = hdv_ws(4, P);
    std::vector<unsigned char> block(L.total);
    std::vector<double> slots(hdv_slot_doubles(P));
    CHECK(slots.size() == (size_t)2 * 6 * 16 * 1 * 1024);
    HdvMapRecord maps[PDMPC_HDV_MAP_SLOTS];
    unsigned char* ws = block.data();
    const auto at = [&](const void* p, size_t region) { return (const unsigned char*)p == ws + region && region <= L.total; };
    const HdvGroupedArgs GA = hdv_grouped_args(4, L, P, ws, slots.data(), maps);
    const HdvArgs& A = GA.a;
    CHECK(A.n_hdv == 6 && A.n_cav == 8 && A.Hp == 1 && A.capacity == 100 && GA.n_groups == 4 && GA.n_pairs == 9 && GA.maps == maps);
    CHECK(at(A.in, L.in) && at(A.trim, L.trim) && at(A.cav, L.cav) && at(A.cav_lanelet, L.cav_lanelet) && at(A.n_closest, L.n_closest) && at(A.closest, L.closest));
    CHECK(at(A.n_chains, L.n_chains) && at(A.chain_id, L.chain_id) && at(A.chain_succ, L.chain_succ) && at(A.slot_n, L.slot_n) && at(A.slot_flags, L.slot_flags));
    CHECK(at(A.status, L.status) && at(A.row_hdv, L.row_hdv) && at(A.set_off, L.set_off) && at(A.set_flags, L.set_flags) && at(A.adjacency, L.adjacency));
    CHECK(at(A.set_x, L.set_xy) && A.set_y == A.set_x + 100 && (const unsigned char*)(A.set_y + 100) == ws + L.total);
    CHECK(A.slot_x == slots.data() && A.slot_y == slots.data() + slots.size() / 2 && !A.local_x && !A.local_y && !A.local_off && !A.map.pt_off);
    CHECK(at(GA.groups, L.groups) && at(GA.group_of, L.group_of) && at(GA.pair_first, L.pair_first) && at(GA.slot_before, L.slot_before) && at(GA.row_base, L.row_base));
    CHECK(at(GA.n_rows, L.n_rows) && at(GA.set_base, L.set_base));
    const HdvDriveArgs D = hdv_drive_args(L, P, ws, maps);
    CHECK(D.maps == maps && D.n_hdv == 6 && D.n_cav == 8 && at(D.groups, L.groups) && at(D.group_of, L.group_of) && at(D.drives, L.drives) && at(D.route_off, L.route_off));
    CHECK(at(D.route_id, L.route_id) && at(D.closed, L.closed) && at(D.state_seg, L.state_seg) && at(D.state_u, L.state_u) && at(D.v_des, L.v_des) && at(D.params, L.params));
    CHECK(at(D.cav, L.cav) && at(D.in, L.in) && at(D.new_seg, L.new_seg) && at(D.new_u, L.new_u) && at(D.speed, L.speed) && at(D.gap, L.gap) && at(D.pose, L.pose));
    // the ungrouped call: the same block of HdvArgs, the map in the record itself
    HdvMapRecord one{};
    double hull[2] = {0, 0};
    int32_t off[2] = {0, 1};
    one.local_x = hull, one.local_y = hull + 1, one.local_off = off, one.map.n_lanelets = 5;
    const HdvPlan Q = plan_of(3, 2, 6, 1, 7);
    const HdvWs U = hdv_ws(0, Q);
    CHECK(U.total <= L.total);
    const HdvArgs B = hdv_args(U, Q, ws, slots.data(), &one);
    CHECK(B.local_x == hull && B.local_y == hull + 1 && B.local_off == off && B.map.n_lanelets == 5 && B.n_hdv == 3 && B.n_cav == 2 && B.capacity == 7);
    CHECK((const unsigned char*)B.in == ws + U.in && (const unsigned char*)B.set_off == ws + U.set_off && B.adjacency == ws + U.adjacency && B.set_y == B.set_x + 7);
    CHECK((const unsigned char*)(B.set_y + 7) == ws + U.total && B.slot_y == slots.data() + (size_t)3 * 16 * 1024);
}

// a map slot of the model: lanelet 1 from (0, 0) to (1, 0), its successor lanelet 2 on to (3, 0); one trim, Hp triangles
HdvSlotData model_slot(int Hp) {
    std::vector<int32_t> lo = {0, 2, 5}, so = {0, 1, 1}, si = {2}, poff((size_t)Hp + 1);
    std::vector<double> lx = {0, 1, 1, 2, 3}, ly(5, .5), ry(5, -.5), px, py;
    std::vector<uint8_t> rel = {0, 1, 0, 0};
    for (int k = 0; k <= Hp; ++k) poff[(size_t)k] = 3 * k;
    for (int k = 0; k < Hp; ++k) {
        px.insert(px.end(), {0, 1. + k, 0});
        py.insert(py.end(), {0, 0, 1});
    }
    pdmpc_polygon_set sets{};
    sets.n_polygons = Hp;
    sets.offset = poff.data();
    sets.x = px.data();
    sets.y = py.data();
    HdvSlotData S;
    const char* why = nullptr;
    CHECK(S.map.points(2, lo.data(), lo.data(), lx.data(), ly.data(), lx.data(), ry.data(), &why) == PDMPC_OK);
    CHECK(S.map.graph(so.data(), si.data(), rel.data(), &why) == PDMPC_OK);
    CHECK(hdv_check_sets(1, Hp, &sets, &why) == PDMPC_OK);
    S.keep_sets(1, Hp, &sets);
    return S;
}

// The arrays of a grouped call of {2, 0, 1, 3} HDVs with {3, 4, 0, 1} CAVs, every group on map slot `slot`: every HDV on the route
// (1, 2), open, on its first segment.  The outputs have exactly the sizes pdmpc_hdv_grouped_layout_host states and hold values no call writes.
const int32_t NONE = -77;
struct Call {
    int32_t G = 4, n = 6, nc = 8, capacity = 0;
    std::vector<int32_t> slot, ho = {0, 2, 2, 3, 6}, co = {0, 3, 7, 7, 8}, trim, cav_lanelet, route_off, route_id, state_seg;
    std::vector<double> tile_dx, tile_dy, cav_x, cav_y, cav_tdx, cav_tdy, x, y, c, s, state_u, v_des, params, dt;
    std::vector<uint8_t> drives = {1, 1, 1, 1}, closed;
    std::vector<int32_t> closest_offset, closest_index, n_rows, row_hdv, set_offset, set_base, new_seg;
    std::vector<double> set_x, set_y, new_u, dx, dy, dc, ds, speed, gap;
    std::vector<uint8_t> set_flags, adjacency;

    Call(int32_t map_slot, int Hp, int32_t room) : capacity(room), slot(4, map_slot) {
        for (int q = 0; q < n; ++q) {
            x.push_back(10 + q), y.push_back(20 + q), c.push_back(30 + q), s.push_back(40 + q), tile_dx.push_back(50 + q), tile_dy.push_back(60 + q);
            trim.push_back(1), route_off.push_back(2 * q), route_id.insert(route_id.end(), {1, 2}), closed.push_back(0);
            state_u.push_back(0.25 + 0.125 * q), v_des.push_back(0.5 + q);
        }
        route_off.push_back(2 * n);
        state_seg.assign((size_t)2 * n, 0);
        for (int v = 0; v < nc; ++v) cav_x.push_back(70 + v), cav_y.push_back(80 + v), cav_tdx.push_back(90 + v), cav_tdy.push_back(100 + v), cav_lanelet.push_back(1 + v % 2);
        for (int g = 0; g < G; ++g) params.insert(params.end(), {2.0 + g, 0.3, 1.0, 0.125}), dt.push_back(0.2 + 0.1 * g);
        std::vector<int32_t> a(5), b(5), cc(5), d(5);
        std::vector<int64_t> e(5);
        CHECK(hdv_grouped_layout(G, ho.data(), co.data(), Hp, a.data(), b.data(), cc.data(), d.data(), e.data()) == PDMPC_OK);
        closest_offset.assign((size_t)a[4], NONE), closest_index.assign((size_t)b[4], NONE), row_hdv.assign((size_t)b[4], NONE), set_offset.assign((size_t)cc[4], NONE);
        set_flags.assign((size_t)d[4], 0xEE), adjacency.assign((size_t)e[4], 0xEE), n_rows.assign(4, NONE), set_base.assign(5, NONE);
        set_x.assign((size_t)room, NAN), set_y.assign((size_t)room, NAN);
        new_seg.assign((size_t)2 * n, NONE);
        for (std::vector<double>* v : {&new_u, &dx, &dy, &dc, &ds, &speed, &gap}) v->assign((size_t)n, NAN);
    }
    HdvGroups groups() const { return HdvGroups{G, slot.data(), ho.data(), co.data(), tile_dx.data(), tile_dy.data(), cav_x.data(), cav_y.data(), cav_tdx.data(), cav_tdy.data()}; }
    HdvTrafficCall traffic() {
        return HdvTrafficCall{x.data(),      y.data(),       c.data(),          s.data(),        trim.data(),  cav_lanelet.data(), closest_offset.data(), closest_index.data(), capacity,
                              n_rows.data(), row_hdv.data(), set_offset.data(), set_base.data(), set_x.data(), set_y.data(),       set_flags.data(),      adjacency.data()};
    }
    HdvDriveCall drive(bool flags = true) {
        return HdvDriveCall{flags ? drives.data() : nullptr, route_off.data(), route_id.data(), closed.data(), state_seg.data(), state_u.data(), v_des.data(), params.data(), dt.data(),
                            new_seg.data(),                  new_u.data(),     dx.data(),       dy.data(),     dc.data(),        ds.data(),      speed.data(), gap.data()};
    }
};

struct Slots {
    HdvSlotData hp1 = model_slot(1), hp6 = model_slot(6);
    const HdvSlotData* slot[PDMPC_HDV_MAP_SLOTS] = {&hp1, &hp6};  // slot 0: Hp 1, slot 1: Hp 6, the others empty
};

template <class T>
const T* in_block(const std::vector<unsigned char>& block, size_t at) {
    return (const T*)(block.data() + at);
}
bool same(const void* a, const void* b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; }

// What the kernels leave in the read-back block of a grouped call, as this file decides it: rows[g] rows (-1: the group's lists ran
// over and it wrote nothing else), HDV h with 1 + h % 3 closest lanelets 1000 h + i, row r of a group on its HDV r % n_g, 3 vertices in
// every polygon, the flags and the adjacency counted up, vertex v at (0.5 + v, -0.5 - v) while there is room; the new states, speeds,
// gaps and poses counted up from 10, 0.125, 1, 2 and 100 k.  Everything else is 0x55.
std::vector<unsigned char> kernel_output(const HdvWs& L, const HdvPlan& P, const Call& K, const int rows[4], int over_flags, int Hp) {
    std::vector<unsigned char> block(L.total - L.out, 0x55);  // exactly what the call copies back
    const auto ints = [&](size_t at) { return (int32_t*)(block.data() + (at - L.out)); };
    const auto doubles = [&](size_t at) { return (double*)(block.data() + (at - L.out)); };
    ints(L.status)[0] = 0;
    ints(L.status)[1] = over_flags;
    int32_t base = 0;
    for (int g = 0; g < 4; ++g) {
        const int h0 = K.ho[(size_t)g], ng = K.ho[(size_t)g + 1] - h0;
        ints(L.n_rows)[g] = rows[g];
        ints(L.set_base)[g] = base;
        if (rows[g] < 0) continue;
        for (int h = h0; h < h0 + ng; ++h) {
            ints(L.n_closest)[h] = 1 + h % 3;
            for (int i = 0; i < 1 + h % 3; ++i) ints(L.closest)[h * C + i] = 1000 * h + i;
        }
        for (int r = 0; r < rows[g]; ++r) ints(L.row_hdv)[P.list_at[(size_t)g] + r] = r % ng;
        for (int i = 0; i <= rows[g] * Hp; ++i) ints(L.set_off)[P.set_offset_at[(size_t)g] + i] = 3 * i;
        for (int i = 0; i < rows[g] * Hp; ++i) (block.data() + (L.set_flags - L.out))[P.set_at[(size_t)g] + i] = (uint8_t)(16 * g + i);
        base += 3 * rows[g] * Hp;
    }
    ints(L.set_base)[4] = base;
    for (int64_t i = 0; i < P.pairs; ++i) (block.data() + (L.adjacency - L.out))[i] = (uint8_t)(i % 2);
    for (int v = 0; v < base && v < P.cap; ++v) doubles(L.set_xy)[v] = 0.5 + v, doubles(L.set_xy)[P.cap + v] = -0.5 - v;
    if (P.n_route >= 0)
        for (int h = 0; h < K.n; ++h) {
            ints(L.new_seg)[h] = 10 + h, ints(L.new_seg)[K.n + h] = 10 + K.n + h;
            doubles(L.new_u)[h] = 0.125 * h, doubles(L.speed)[h] = 1 + h, doubles(L.gap)[h] = 2 + h;
            for (int k = 0; k < 4; ++k) doubles(L.pose)[k * K.n + h] = 100 * k + h;
        }
    return block;
}

// One grouped call from the checks to the scatter: capacity `room`, the groups' rows, the status flags, which parts it has -> its
// return code; the staged bytes and every output are compared with what this file put there.
int round_trip(int Hp, int room, const int rows[4], int over_flags, bool traffic, bool drive, bool flags, const char* expect_text) {
    const Slots M;
    Call K(Hp == 1 ? 0 : 1, Hp, room);
    if (flags) K.drives = {1, 1, 0, 1};  // (group 2: HDV 2)
    const HdvGroups G = K.groups();
    const HdvTrafficCall Tr = K.traffic();
    const HdvDriveCall Dr = K.drive(flags);
    const HdvTrafficCall* T = traffic ? &Tr : nullptr;
    const HdvDriveCall* D = drive ? &Dr : nullptr;
    const char* who = "who: ";
    HdvPlan P;
    std::string why;
    CHECK(hdv_check_grouped(who, G, T, D, M.slot, P, &why) == PDMPC_OK && why.empty());
    const int eff = traffic ? Hp : 1;  // (without the traffic passes no slot's Hp is read)
    CHECK(P.n == 6 && P.nc == 8 && P.Hp == eff && P.pairs == 9 && P.n_route == (drive ? 12 : -1) && P.cap == (traffic ? room : 0));
    CHECK(P.closest_at.size() == 5 && P.list_at[4] == 6 * C && P.set_offset_at[3] == 3 * C * eff + 3 && P.set_at[2] == 2 * C * eff && P.adjacency_at[3] == 6);
    hdv_zero_outputs(G, T, P);
    for (size_t i = 0; traffic && i < K.closest_offset.size(); ++i) CHECK(K.closest_offset[i] == (i == 0 || i == 3 || i == 4 || i == 6 ? 0 : NONE));
    for (size_t i = 0; traffic && i < K.set_offset.size(); ++i) {
        const size_t e = (size_t)C * eff;
        CHECK(K.set_offset[i] == (i == 0 || i == 2 * e + 1 || i == 2 * e + 2 || i == 3 * e + 3 ? 0 : NONE));
    }
    if (traffic) CHECK(K.n_rows == std::vector<int32_t>(4, 0) && K.set_base == std::vector<int32_t>(5, 0));
    if (!traffic) CHECK(K.n_rows == std::vector<int32_t>(4, NONE) && K.set_base == std::vector<int32_t>(5, NONE));
    const HdvWs L = hdv_ws(4, P);
    // stage: a block of exactly in_bytes bytes
    std::vector<unsigned char> in(L.in_bytes, 0x55);
    hdv_stage(in.data(), L, P, G, T, D);
    const double* pose = in_block<double>(in, L.in);
    const std::vector<double> zeros(6, 0.0);
    CHECK(same(pose, traffic ? K.x.data() : zeros.data(), 48) && same(pose + 6, traffic ? K.y.data() : zeros.data(), 48));
    CHECK(same(pose + 12, traffic ? K.c.data() : zeros.data(), 48) && same(pose + 18, traffic ? K.s.data() : zeros.data(), 48));
    CHECK(same(pose + 24, K.tile_dx.data(), 48) && same(pose + 30, K.tile_dy.data(), 48));
    const double* cav = in_block<double>(in, L.cav);
    CHECK(same(cav, K.cav_x.data(), 64) && same(cav + 8, K.cav_y.data(), 64) && same(cav + 16, K.cav_tdx.data(), 64) && same(cav + 24, K.cav_tdy.data(), 64));
    for (int q = 0; traffic && q < 6; ++q) CHECK(in_block<int32_t>(in, L.trim)[q] == 0);  // 0-based
    if (traffic) CHECK(same(in_block<int32_t>(in, L.cav_lanelet), K.cav_lanelet.data(), 32));
    const int32_t want_groups[4][5] = {{K.slot[0], 0, 2, 0, 3}, {K.slot[0], 2, 0, 3, 4}, {K.slot[0], 2, 1, 7, 0}, {K.slot[0], 3, 3, 7, 1}};
    const int32_t want_group_of[6] = {0, 0, 2, 3, 3, 3}, want_pair_first[5] = {0, 6, 6, 6, 9};
    CHECK(sizeof(HdvGroup) == 20 && same(in_block<HdvGroup>(in, L.groups), want_groups, 80));
    CHECK(same(in_block<int32_t>(in, L.group_of), want_group_of, 24) && same(in_block<int32_t>(in, L.pair_first), want_pair_first, 20));
    if (drive) {
        const uint8_t all[4] = {1, 1, 1, 1};
        CHECK(same(in_block<uint8_t>(in, L.drives), flags ? K.drives.data() : all, 4));
        CHECK(same(in_block<int32_t>(in, L.route_off), K.route_off.data(), 28) && same(in_block<int32_t>(in, L.route_id), K.route_id.data(), 48));
        CHECK(same(in_block<uint8_t>(in, L.closed), K.closed.data(), 6) && same(in_block<int32_t>(in, L.state_seg), K.state_seg.data(), 48));
        CHECK(same(in_block<double>(in, L.state_u), K.state_u.data(), 48) && same(in_block<double>(in, L.v_des), K.v_des.data(), 48));
        for (int g = 0; g < 4; ++g) {
            const double* p = in_block<double>(in, L.params) + 5 * g;
            CHECK(same(p, K.params.data() + 4 * g, 32) && p[4] == K.dt[(size_t)g]);
        }
    }
    // scatter: from a block of exactly total - out bytes
    const std::vector<unsigned char> out = kernel_output(L, P, K, rows, over_flags, eff);
    const int rc = hdv_scatter(who, out.data(), L, P, G, T, D, &why);
    CHECK(why == (expect_text ? std::string(who) + expect_text : std::string()));
    for (int h = 0; h < 6; ++h) {  // the drive results of the groups that drove; group 2 (HDV 2) does not with the flags
        const bool drove = drive && !(flags && h == 2);
        CHECK(K.new_seg[(size_t)h] == (drove ? 10 + h : NONE) && K.new_seg[(size_t)(6 + h)] == (drove ? 16 + h : NONE));
        if (drove)
            CHECK(K.new_u[(size_t)h] == 0.125 * h && K.speed[(size_t)h] == 1 + h && K.gap[(size_t)h] == 2 + h && K.dx[(size_t)h] == h && K.dy[(size_t)h] == 100 + h &&
                  K.dc[(size_t)h] == 200 + h && K.ds[(size_t)h] == 300 + h);
        else
            CHECK(std::isnan(K.new_u[(size_t)h]) && std::isnan(K.speed[(size_t)h]) && std::isnan(K.gap[(size_t)h]) && std::isnan(K.dx[(size_t)h]) && std::isnan(K.ds[(size_t)h]));
    }
    if (!traffic) return rc;
    int32_t base = 0;
    for (int g = 0; g < 4; ++g) {
        const int h0 = K.ho[(size_t)g], ng = K.ho[(size_t)g + 1] - h0, e = C * eff;
        CHECK(K.n_rows[(size_t)g] == rows[g] && K.set_base[(size_t)g] == base);
        const int32_t* co = K.closest_offset.data() + h0 + g;
        if (rows[g] < 0) {  // nothing but n_rows: what the zero stage left
            for (int q = 1; q <= ng; ++q) CHECK(co[q] == NONE);
            for (int i = 0; i < ng * C; ++i) CHECK(K.closest_index[(size_t)(h0 * C + i)] == NONE && K.row_hdv[(size_t)(h0 * C + i)] == NONE);
            for (int i = 1; i <= ng * e; ++i) CHECK(K.set_offset[(size_t)(h0 * e + g + i)] == NONE);
            continue;
        }
        int listed = 0;
        for (int q = 0; q < ng; ++q) {
            CHECK(co[q] == listed && co[q + 1] == listed + 1 + (h0 + q) % 3);
            for (int i = 0; i < 1 + (h0 + q) % 3; ++i) CHECK(K.closest_index[(size_t)(h0 * C + listed + i)] == 1000 * (h0 + q) + i);
            listed += 1 + (h0 + q) % 3;
        }
        for (int i = listed; i < ng * C; ++i) CHECK(K.closest_index[(size_t)(h0 * C + i)] == NONE);
        for (int r = 0; r < ng * C; ++r) CHECK(K.row_hdv[(size_t)(h0 * C + r)] == (r < rows[g] ? r % ng : NONE));
        for (int i = 0; i <= ng * e; ++i) CHECK(K.set_offset[(size_t)(h0 * e + g + i)] == (i <= rows[g] * eff ? 3 * i : NONE));
        for (int i = 0; i < ng * e; ++i) CHECK(K.set_flags[(size_t)(h0 * e + i)] == (i < rows[g] * eff ? (uint8_t)(16 * g + i) : 0xEE));
        base += 3 * rows[g] * eff;
    }
    CHECK(K.set_base[4] == base);
    for (size_t i = 0; i < 9; ++i) CHECK(K.adjacency[i] == i % 2);
    const bool vertices = room >= base && !(over_flags & PDMPC_HDV_OVER_SLOT);  // (a group that ran over its lists does not keep the others' from coming back)
    for (int v = 0; v < room; ++v) {
        if (vertices && v < base)
            CHECK(K.set_x[(size_t)v] == 0.5 + v && K.set_y[(size_t)v] == -0.5 - v);
        else
            CHECK(std::isnan(K.set_x[(size_t)v]) && std::isnan(K.set_y[(size_t)v]));
    }
    return rc;
}

void check_round_trips() {
    const int whole[4] = {3, 0, 1, 4}, over[4] = {3, 0, -1, 4};
    const char *lists = "group 2: an HDV has more than PDMPC_HDV_MAX_CHAINS closest lanelets or chains", *slot = "a reachable lane has more than PDMPC_BOUNDED_MAX_COLS vertices",
               *room = "capacity too small for the reachable lanes";
    for (int Hp : {1, 6}) {
        const int total = 3 * 8 * Hp, without = 3 * 7 * Hp;
        CHECK(round_trip(Hp, total, whole, 0, true, false, false, nullptr) == PDMPC_OK);                   // exactly the room
        CHECK(round_trip(Hp, total + 9, whole, 0, true, true, true, nullptr) == PDMPC_OK);                 // drive and traffic, group 2 does not drive
        CHECK(round_trip(Hp, 0, whole, 0, false, true, false, nullptr) == PDMPC_OK);                       // the drive pass alone
        CHECK(round_trip(Hp, total - 1, whole, 0, true, false, false, room) == PDMPC_ERR_CAPACITY);        // one vertex short: all but the vertices
        CHECK(round_trip(Hp, total - 1, whole, 0, true, true, true, room) == PDMPC_ERR_CAPACITY);          // ... and the drive results are there
        CHECK(round_trip(Hp, 0, whole, 0, true, false, false, room) == PDMPC_ERR_CAPACITY);
        CHECK(round_trip(Hp, without, over, PDMPC_HDV_OVER_LISTS, true, false, false, lists) == PDMPC_ERR_CAPACITY);  // the other groups whole, with vertices
        CHECK(round_trip(Hp, total, whole, PDMPC_HDV_OVER_SLOT, true, false, false, slot) == PDMPC_ERR_CAPACITY);
        // the precedence: lists over, then slot over, then capacity
        CHECK(round_trip(Hp, without - 1, over, PDMPC_HDV_OVER_LISTS | PDMPC_HDV_OVER_SLOT, true, false, false, lists) == PDMPC_ERR_CAPACITY);
        CHECK(round_trip(Hp, total - 1, whole, PDMPC_HDV_OVER_SLOT, true, false, false, slot) == PDMPC_ERR_CAPACITY);
    }
}

// the ungrouped call through the same stage and the same read-back arithmetic: 3 HDVs and 2 CAVs at Hp 6
void check_ungrouped_round_trip() {
    const int n = 3, nc = 2, Hp = 6, rows = 4, total = 3 * rows * Hp;
    for (int variant = 0; variant < 4; ++variant) {  // whole; one vertex short; a slot ran over; the lists ran over
        const int room = variant == 1 ? total - 1 : total;
        std::vector<double> x = {1, 2, 3}, y = {4, 5, 6}, c = {7, 8, 9}, s = {10, 11, 12}, tx = {13, 14, 15}, ty = {16, 17, 18}, cx = {19, 20}, cy = {21, 22}, ctx = {23, 24}, cty = {25, 26};
        std::vector<int32_t> trim = {1, 2, 1}, lanelet = {2, 1};
        std::vector<int32_t> closest_offset((size_t)n + 1, NONE), closest_index((size_t)n * C, NONE), n_rows(1, NONE), row_hdv((size_t)n * C, NONE), set_offset((size_t)n * C * Hp + 1, NONE);
        std::vector<double> set_x((size_t)room, NAN), set_y((size_t)room, NAN);
        std::vector<uint8_t> set_flags((size_t)n * C * Hp, 0xEE), adjacency((size_t)nc * n, 0xEE);
        const HdvGroups G{0, nullptr, nullptr, nullptr, tx.data(), ty.data(), cx.data(), cy.data(), ctx.data(), cty.data()};
        const HdvTrafficCall T{x.data(),      y.data(),       c.data(),          s.data(), trim.data(),  lanelet.data(), closest_offset.data(), closest_index.data(), room,
                               n_rows.data(), row_hdv.data(), set_offset.data(), nullptr,  set_x.data(), set_y.data(),   set_flags.data(),      adjacency.data()};
        const HdvPlan P = hdv_plan_one(n, nc, Hp, T);
        CHECK(P.n == n && P.nc == nc && P.Hp == Hp && P.pairs == 6 && P.cap == room && P.n_route == -1 && P.closest_at.empty());
        hdv_zero_outputs(G, &T, P);
        CHECK(n_rows[0] == 0 && closest_offset[0] == 0 && closest_offset[1] == NONE && set_offset[0] == 0 && set_offset[1] == NONE);
        const HdvWs L = hdv_ws(0, P);
        std::vector<unsigned char> in(L.in_bytes, 0x55);
        hdv_stage(in.data(), L, P, G, &T, nullptr);
        const double* pose = in_block<double>(in, L.in);
        CHECK(same(pose, x.data(), 24) && same(pose + 3, y.data(), 24) && same(pose + 6, c.data(), 24) && same(pose + 9, s.data(), 24) && same(pose + 12, tx.data(), 24) && same(pose + 15, ty.data(), 24));
        const double* cav = in_block<double>(in, L.cav);
        CHECK(same(cav, cx.data(), 16) && same(cav + 2, cy.data(), 16) && same(cav + 4, ctx.data(), 16) && same(cav + 6, cty.data(), 16));
        const int32_t trim0[3] = {0, 1, 0};
        CHECK(same(in_block<int32_t>(in, L.trim), trim0, 12) && same(in_block<int32_t>(in, L.cav_lanelet), lanelet.data(), 8));
        std::vector<unsigned char> out(L.total - L.out, 0x55);
        const auto ints = [&](size_t at) { return (int32_t*)(out.data() + (at - L.out)); };
        ints(L.status)[0] = rows;
        ints(L.status)[1] = variant == 2 ? PDMPC_HDV_OVER_SLOT : variant == 3 ? PDMPC_HDV_OVER_LISTS : 0;
        for (int h = 0; h < n; ++h) {
            ints(L.n_closest)[h] = 1 + h;
            for (int i = 0; i <= h; ++i) ints(L.closest)[h * C + i] = 1000 * h + i;
        }
        for (int r = 0; r < rows; ++r) ints(L.row_hdv)[r] = r % n;
        for (int i = 0; i <= rows * Hp; ++i) ints(L.set_off)[i] = 3 * i;
        for (int i = 0; i < rows * Hp; ++i) (out.data() + (L.set_flags - L.out))[i] = (uint8_t)i;
        for (int i = 0; i < nc * n; ++i) (out.data() + (L.adjacency - L.out))[i] = (uint8_t)(i % 2);
        double* xy = (double*)(out.data() + (L.set_xy - L.out));
        for (int v = 0; v < total && v < room; ++v) xy[v] = 0.5 + v, xy[room + v] = -0.5 - v;
        const char* why = nullptr;
        const int rc = hdv_scatter_one(out.data(), L, P, T, &why);
        if (variant == 3) {  // n_rows -1 and nothing else
            CHECK(rc == PDMPC_ERR_CAPACITY && std::string(why) == "pdmpc_hdv_traffic: an HDV has more than PDMPC_HDV_MAX_CHAINS closest lanelets or chains");
            CHECK(n_rows[0] == -1 && closest_offset[1] == NONE && closest_index[0] == NONE && row_hdv[0] == NONE && set_offset[1] == NONE && adjacency[0] == 0xEE && std::isnan(set_x[0]));
            continue;
        }
        CHECK(n_rows[0] == rows && closest_offset == std::vector<int32_t>({0, 1, 3, 6}));
        for (int h = 0, listed = 0; h < n; listed += 1 + h, ++h)
            for (int i = 0; i <= h; ++i) CHECK(closest_index[(size_t)(listed + i)] == 1000 * h + i);
        CHECK(closest_index[6] == NONE);
        for (int r = 0; r < n * C; ++r) CHECK(row_hdv[(size_t)r] == (r < rows ? r % n : NONE));
        for (int i = 0; i <= n * C * Hp; ++i) CHECK(set_offset[(size_t)i] == (i <= rows * Hp ? 3 * i : NONE));
        for (int i = 0; i < nc * n; ++i) CHECK(adjacency[(size_t)i] == i % 2);
        if (variant == 0) {
            CHECK(rc == PDMPC_OK);
            for (int v = 0; v < total; ++v) CHECK(set_x[(size_t)v] == 0.5 + v && set_y[(size_t)v] == -0.5 - v);
            for (int i = 0; i < n * C * Hp; ++i) CHECK(set_flags[(size_t)i] == (i < rows * Hp ? (uint8_t)i : 0xEE));
        } else {  // no vertices and no flags
            CHECK(rc == PDMPC_ERR_CAPACITY && std::string(why) == (variant == 1 ? "pdmpc_hdv_traffic: capacity too small for the reachable lanes"
                                                                                : "pdmpc_hdv_traffic: a reachable lane has more than PDMPC_BOUNDED_MAX_COLS vertices"));
            for (int v = 0; v < room; ++v) CHECK(std::isnan(set_x[(size_t)v]) && std::isnan(set_y[(size_t)v]));
            for (int i = 0; i < n * C * Hp; ++i) CHECK(set_flags[(size_t)i] == 0xEE);
        }
    }
}

// The refusals of the checks, texts as pdmpc_hdv_*_grouped have given them: a good call on slot 0 (Hp 1), one thing made wrong in the
// arrays (K) or the records, the parts the call has, the code and the text behind the call's name.
struct Records {
    HdvGroups G;
    HdvTrafficCall T;
    HdvDriveCall D;
};
struct Bad {
    const char* name;
    void (*spoil)(Call& K, Records& R);
    bool traffic, drive;
    int code;
    const char* text;
};
const Bad BAD[] = {
    {"no groups array", [](Call&, Records& R) { R.G.group_slot = nullptr; }, true, false, PDMPC_ERR_INVALID, "bad argument"},
    {"a negative number of groups", [](Call&, Records& R) { R.G.n_groups = -1; }, false, true, PDMPC_ERR_INVALID, "bad argument"},
    {"a negative capacity", [](Call&, Records& R) { R.T.capacity = -1; }, true, false, PDMPC_ERR_INVALID, "bad argument"},
    {"no set_base", [](Call&, Records& R) { R.T.set_base = nullptr; }, true, true, PDMPC_ERR_INVALID, "bad argument"},
    {"no n_rows", [](Call&, Records& R) { R.T.n_rows = nullptr; }, true, false, PDMPC_ERR_INVALID, "bad argument"},
    {"no CAV offsets", [](Call&, Records& R) { R.G.cav_offset = nullptr; }, false, true, PDMPC_ERR_INVALID, "bad argument"},
    {"HDV offsets from 1", [](Call& K, Records&) { K.ho[0] = 1; }, true, false, PDMPC_ERR_INVALID, "offsets that do not start at 0"},
    {"CAV offsets from 1", [](Call& K, Records&) { K.co[0] = 1; }, false, true, PDMPC_ERR_INVALID, "offsets that do not start at 0"},
    {"HDV offsets decrease", [](Call& K, Records&) { K.ho[2] = 1; }, true, false, PDMPC_ERR_INVALID, "group 1: offsets decrease"},
    {"CAV offsets decrease", [](Call& K, Records&) { K.co[3] = 6; }, true, true, PDMPC_ERR_INVALID, "group 2: offsets decrease"},
    {"slot 8", [](Call& K, Records&) { K.slot[3] = PDMPC_HDV_MAP_SLOTS; }, true, false, PDMPC_ERR_INVALID, "group 3: map slot out of range"},
    {"slot -1", [](Call& K, Records&) { K.slot[0] = -1; }, false, true, PDMPC_ERR_INVALID, "group 0: map slot out of range"},
    {"an empty slot", [](Call& K, Records&) { K.slot[1] = 2; }, true, false, PDMPC_ERR_INVALID, "group 1: no map was uploaded into its slot"},
    {"slots of two Hp", [](Call& K, Records&) { K.slot[2] = 1; }, true, false, PDMPC_ERR_INVALID, "group 2: the Hp of its slot differs from the slots of the groups before"},
    {"slots of two Hp, drive alone: no Hp is read", [](Call& K, Records&) { K.slot[2] = 1; }, false, true, PDMPC_OK, ""},
    {"too many slots for 32-bit blocks", [](Call& K, Records&) { K.ho[4] = 200000000; }, true, false, PDMPC_ERR_CAPACITY, "bad offsets"},
    {"65 HDVs in a group", [](Call& K, Records&) { K.ho = {0, 65, 65, 66, 69}; }, true, false, PDMPC_ERR_CAPACITY, "group 0: more than PDMPC_HDV_MAX_VEHICLES HDVs or PDMPC_HDV_MAX_CAVS CAVs"},
    {"129 HDVs in the call", [](Call& K, Records&) { K.ho = {0, 43, 43, 86, 129}; }, false, true, PDMPC_ERR_CAPACITY, "more than PDMPC_HDV_GROUPED_MAX_VEHICLES HDVs in the call"},
    {"no tiles", [](Call&, Records& R) { R.G.tile_dy = nullptr; }, false, true, PDMPC_ERR_INVALID, "a null HDV array"},
    {"no poses", [](Call&, Records& R) { R.T.cos_yaw = nullptr; }, true, false, PDMPC_ERR_INVALID, "a null HDV array"},
    {"no row_hdv", [](Call&, Records& R) { R.T.row_hdv = nullptr; }, true, true, PDMPC_ERR_INVALID, "a null HDV array"},
    {"no CAV positions", [](Call&, Records& R) { R.G.cav_y = nullptr; }, false, true, PDMPC_ERR_INVALID, "a null CAV array"},
    {"no CAV lanelets", [](Call&, Records& R) { R.T.cav_lanelet = nullptr; }, true, false, PDMPC_ERR_INVALID, "a null CAV array"},
    {"no CAV lanelets, drive alone: not read", [](Call&, Records& R) { R.T.cav_lanelet = nullptr; }, false, true, PDMPC_OK, ""},
    {"no adjacency", [](Call&, Records& R) { R.T.adjacency = nullptr; }, true, false, PDMPC_ERR_INVALID, "no adjacency array"},
    {"no route offsets", [](Call&, Records& R) { R.D.route_offset = nullptr; }, false, true, PDMPC_ERR_INVALID, "a null driver array, or route offsets that do not start at 0"},
    {"route offsets from 1", [](Call& K, Records&) { K.route_off[0] = 1; }, true, true, PDMPC_ERR_INVALID, "a null driver array, or route offsets that do not start at 0"},
    {"no parameters", [](Call&, Records& R) { R.D.parameters = nullptr; }, false, true, PDMPC_ERR_INVALID, "a null driver array, or route offsets that do not start at 0"},
    {"no gap output", [](Call&, Records& R) { R.D.gap = nullptr; }, false, true, PDMPC_ERR_INVALID, "a null driver array, or route offsets that do not start at 0"},
    {"route offsets decrease", [](Call& K, Records&) { K.route_off[3] = 3; }, false, true, PDMPC_ERR_INVALID, "route offsets decrease"},
    {"a route against the map", [](Call& K, Records&) { K.route_id[8] = 2, K.route_id[9] = 1; }, false, true, PDMPC_ERR_INVALID,
     "group 3: HDV 1: route position 1: lanelet 1 is no successor of lanelet 2"},
    {"a route of no lanelet", [](Call& K, Records&) { K.route_off[1] = 0; }, true, true, PDMPC_ERR_INVALID, "group 0: HDV 0: a route of 0 lanelets (1 .. PDMPC_HDV_ROUTE_MAX)"},
    {"a state off its route", [](Call& K, Records&) { K.state_seg[6 + 1] = 10000; }, false, true, PDMPC_ERR_INVALID, "group 0: HDV 1: a state that is not on its route"},
    {"headway below dt", [](Call& K, Records&) { K.dt[2] = 1.5; }, false, true, PDMPC_ERR_INVALID, "group 2: headway < dt: an HDV could close more than gap - gap_min in one step"},
    {"a negative desired speed", [](Call& K, Records&) { K.v_des[4] = -1.0; }, true, true, PDMPC_ERR_INVALID, "group 3: a desired speed that is negative or not finite"},
    {"a bad route in a group that does not drive: not read", [](Call& K, Records&) { K.drives[3] = 0, K.route_id[8] = 77; }, true, true, PDMPC_OK, ""},
    {"trim 0", [](Call& K, Records&) { K.trim[2] = 0; }, true, false, PDMPC_ERR_INVALID, "group 2: trim out of range"},
    {"trim 2 of 1", [](Call& K, Records&) { K.trim[5] = 2; }, true, true, PDMPC_ERR_INVALID, "group 3: trim out of range"},
    {"a CAV on lanelet 3 of 2", [](Call& K, Records&) { K.cav_lanelet[7] = 3; }, true, false, PDMPC_ERR_INVALID, "group 3: a CAV's lanelet id out of range"},
    {"a CAV of a group without HDVs on lanelet 0", [](Call& K, Records&) { K.cav_lanelet[4] = 0; }, true, false, PDMPC_ERR_INVALID, "group 1: a CAV's lanelet id out of range"},
    // two faults: the order of the checks decides
    {"an empty slot in group 0 and decreasing offsets in group 2", [](Call& K, Records&) { K.slot[0] = 5, K.co[3] = 6; }, true, false, PDMPC_ERR_INVALID,
     "group 0: no map was uploaded into its slot"},
    {"a bad trim in group 0 and a bad route in group 3", [](Call& K, Records&) { K.trim[0] = 9, K.route_id[8] = 2, K.route_id[9] = 1; }, true, true, PDMPC_ERR_INVALID,
     "group 3: HDV 1: route position 1: lanelet 1 is no successor of lanelet 2"},
    {"129 HDVs and no tiles", [](Call& K, Records& R) { K.ho = {0, 43, 43, 86, 129}, R.G.tile_dx = nullptr; }, true, false, PDMPC_ERR_CAPACITY,
     "more than PDMPC_HDV_GROUPED_MAX_VEHICLES HDVs in the call"},
    {"a bad CAV lanelet in group 0 and a bad trim in group 3", [](Call& K, Records&) { K.cav_lanelet[0] = 3, K.trim[5] = 0; }, true, false, PDMPC_ERR_INVALID,
     "group 0: a CAV's lanelet id out of range"},
};

void check_refusals() {
    const Slots M;
    for (const Bad& B : BAD) {
        Call K(0, 1, 64);
        Records R{K.groups(), K.traffic(), K.drive()};
        B.spoil(K, R);
        const char* who = B.traffic && B.drive ? "pdmpc_hdv_drive_traffic_grouped: " : B.drive ? "pdmpc_hdv_drive_grouped: " : "pdmpc_hdv_traffic_grouped: ";
        HdvPlan P;
        std::string why;
        const int rc = hdv_check_grouped(who, R.G, B.traffic ? &R.T : nullptr, B.drive ? &R.D : nullptr, M.slot, P, &why);
        if (rc != B.code || why != (B.code ? std::string(who) + B.text : std::string())) {
            std::printf("FAILED refusal '%s': code %d, text '%s'\n", B.name, rc, why.c_str());
            std::exit(1);
        }
        CHECK(K.n_rows[0] == NONE && K.set_base[0] == NONE);  // a check writes nothing
    }
    // no group at all: accepted without any array but set_base, which the zero stage then sizes
    int32_t set_base[1] = {NONE};
    HdvTrafficCall T{};
    T.set_base = set_base;
    const HdvGroups none{};
    HdvPlan P;
    std::string why;
    CHECK(hdv_check_grouped("who: ", none, &T, nullptr, M.slot, P, &why) == PDMPC_OK && P.n == 0 && P.closest_at.empty());
    hdv_zero_outputs(none, &T, P);
    CHECK(set_base[0] == 0);
    CHECK(hdv_check_grouped("who: ", none, nullptr, nullptr, M.slot, P, &why) == PDMPC_OK);
    hdv_zero_outputs(none, nullptr, P);
}
}  // namespace

int main() {
    check_layout(1);
    check_layout(6);
    check_batches();
    check_content();
    check_workspace();
    check_arguments();
    check_round_trips();
    check_ungrouped_round_trip();
    check_refusals();
    std::printf("hdv grouped checks ok\n");
    return 0;
}
