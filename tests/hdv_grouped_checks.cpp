// hdv_grouped_checks.cpp — the host-only rules of the grouped HDV traffic call (csrc/hdv_grouped_host.hpp, csrc/hdv_host.hpp) as a
// stand-alone program: the layout of the groups' blocks against sums written out here, the batches of a lock-step and their map slots
// against a model of a handle (eight slots that hold a map id and a generation), and the byte-for-byte content check of a slot.
// tests/test_hdv_grouped_host.py compiles it with -fsanitize=address,undefined and runs it; it prints "hdv grouped checks ok" last.
#include <cstdio>
#include <cstdlib>
#include <vector>

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
}  // namespace

int main() {
    check_layout(1);
    check_layout(6);
    check_batches();
    check_content();
    std::printf("hdv grouped checks ok\n");
    return 0;
}
