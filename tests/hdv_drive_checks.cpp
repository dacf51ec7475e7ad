// hdv_drive_checks.cpp — the HDV driver model on the host (include/pdmpc_hdv.h: "the driver model"; csrc/hdv_drive_host.hpp) as a
// stand-alone program on maps made here: the route checks, the placement, the window builder (the segment of length 0, the cap, the
// wrap, the end of an open route) and the step of a member (free road, slowed, stopped, beside the route, behind, another tile, the
// simultaneous update), every array of exactly the size the call may touch.  tests/test_hdv_drive_host.py compiles it with
// -fsanitize=address,undefined and runs it; it prints "hdv drive checks ok" last.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "hdv_drive_host.hpp"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

namespace {
// Five lanelets, 0.5 wide, each along a line y = y0.  1: x = 0, 1, 1, 2 (a segment of length 0), followed by 2: x = 2, 3, 4.
// 3, alone: 101 points 0.01 m apart.  4 -> 5 -> 4 is a ring of two lanelets (x = 0, 1, 2 at y = 9 and back x = 2, 1, 0 at y = 9.5, the
// joints 0.5 m long): closed routes wrap on it.
struct Map {
    HdvMapData data;
    Map() {
        std::vector<std::vector<double>> xs = {{0.0, 1.0, 1.0, 2.0}, {2.0, 3.0, 4.0}, {}, {0.0, 1.0, 2.0}, {2.0, 1.0, 0.0}};
        for (int q = 0; q <= 100; ++q) xs[2].push_back(0.01 * q);
        const double y0[5] = {0.0, 0.0, 5.0, 9.0, 9.5};
        std::vector<int32_t> off(1, 0), so = {0, 1, 1, 1, 2, 3}, si = {2, 5, 4};
        std::vector<double> lx, ly, rx, ry;
        for (size_t i = 0; i < xs.size(); ++i) {
            for (double x : xs[i]) {
                lx.push_back(x);
                ly.push_back(y0[i] + 0.25);
                rx.push_back(x);
                ry.push_back(y0[i] - 0.25);
            }
            off.push_back((int32_t)lx.size());
        }
        std::vector<uint8_t> rel(25, 0);
        const char* why = nullptr;
        CHECK(data.points(5, off.data(), off.data(), lx.data(), ly.data(), rx.data(), ry.data(), &why) == PDMPC_OK);
        CHECK(data.graph(so.data(), si.data(), rel.data(), &why) == PDMPC_OK);
    }
};

struct Routes {
    std::vector<int32_t> off{0}, id;
    std::vector<uint8_t> closed;
    void add(std::vector<int32_t> ids, bool c) {
        id.insert(id.end(), ids.begin(), ids.end());
        off.push_back((int32_t)id.size());
        closed.push_back(c ? 1 : 0);
    }
    int n() const { return (int)closed.size(); }
};

int check_routes(const Map& m, const Routes& r, std::string* why) {
    // (copies of exactly the sizes: the sanitizer sees a read behind them)
    std::unique_ptr<int32_t[]> off(new int32_t[r.off.size()]), id(new int32_t[r.id.size()]);
    std::unique_ptr<uint8_t[]> closed(new uint8_t[r.closed.size()]);
    std::copy(r.off.begin(), r.off.end(), off.get());
    std::copy(r.id.begin(), r.id.end(), id.get());
    std::copy(r.closed.begin(), r.closed.end(), closed.get());
    return hdv_check_routes(m.data, r.n(), off.get(), id.get(), closed.get(), why);
}

void check_route_rules(const Map& m) {
    std::string why;
    Routes ok;
    ok.add({1, 2}, false);
    ok.add({4, 5}, true);
    ok.add({3}, false);
    ok.add({5, 4, 5}, false);
    CHECK(check_routes(m, ok, &why) == PDMPC_OK);
    Routes bad;
    bad.add({1, 2}, false);
    bad.add({2, 1}, false);
    CHECK(check_routes(m, bad, &why) == PDMPC_ERR_INVALID && why == "HDV 1: route position 1: lanelet 1 is no successor of lanelet 2");
    Routes open_ring;
    open_ring.add({1, 2}, true);
    CHECK(check_routes(m, open_ring, &why) == PDMPC_ERR_INVALID && why.find("HDV 0: route position 0: lanelet 1 is no successor of lanelet 2") == 0);
    Routes range;
    range.add({4, 6}, false);
    CHECK(check_routes(m, range, &why) == PDMPC_ERR_INVALID && why == "HDV 0: route position 1: lanelet id 6 out of range");
    Routes longer, limit;
    std::vector<int32_t> ring;
    for (int q = 0; q < PDMPC_HDV_ROUTE_MAX + 1; ++q) ring.push_back(q % 2 ? 5 : 4);
    longer.add(ring, false);
    CHECK(check_routes(m, longer, &why) == PDMPC_ERR_INVALID && why.find("a route of 65 lanelets") != std::string::npos);
    ring.pop_back();
    limit.add(ring, true);
    CHECK(check_routes(m, limit, &why) == PDMPC_OK);
    Routes none;
    none.add({}, false);
    CHECK(check_routes(m, none, &why) == PDMPC_ERR_INVALID);
}

pdmpc_hdv_drive_state place(const Map& m, const pdmpc_hdv_route& R, double d) {
    pdmpc_hdv_drive_state S;
    std::string why;
    CHECK(hdv_place(m.data.view(), R, d, &S, &why) == PDMPC_OK);
    return S;
}

void check_walk_and_window(const Map& m) {
    const pdmpc_hdv_map M = m.data.view();
    std::string why;
    const int32_t r12[2] = {1, 2}, r3[1] = {3}, r45[2] = {4, 5};
    const pdmpc_hdv_route A{r12, 2, 0}, B{r3, 1, 0}, C{r45, 2, 1};
    CHECK(pdmpc_hdv_route_segments(&M, &A, 0) == 4 && pdmpc_hdv_route_segments(&M, &A, 1) == 2 && pdmpc_hdv_route_total(&M, &A) == 6);
    CHECK(pdmpc_hdv_route_segments(&M, &C, 1) == 3 && pdmpc_hdv_route_total(&M, &C) == 6);
    // over the segment of length 0 and the joint (length 0 here too: lanelet 2 starts where 1 ends)
    pdmpc_hdv_drive_state S = place(m, A, 0.75);
    CHECK(S.r == 0 && S.j == 0 && S.u == 0.75);
    CHECK(pdmpc_hdv_walk(&M, &A, &S, 0.5) == 0 && S.r == 0 && S.j == 2 && S.u == 0.25);
    CHECK(pdmpc_hdv_walk(&M, &A, &S, 1.0) == 0 && S.r == 1 && S.j == 0 && S.u == 0.25);
    // the end of the open route: it stops there, and stays
    CHECK(pdmpc_hdv_walk(&M, &A, &S, 5.0) == 1 && S.r == 1 && S.j == 1 && S.u == 1.0);
    CHECK(pdmpc_hdv_walk(&M, &A, &S, 0.1) == 1 && S.r == 1 && S.j == 1 && S.u == 1.0);
    pdmpc_hdv_drive_state E;
    CHECK(hdv_place(M, A, 4.0, &E, &why) == PDMPC_ERR_INVALID && hdv_place(M, A, -1.0, &E, &why) == PDMPC_ERR_INVALID);
    CHECK(hdv_place(M, A, (double)NAN, &E, &why) == PDMPC_ERR_INVALID);
    // the window: segments of length 0 are not listed, the sum runs from -u, an open route ends it
    std::unique_ptr<pdmpc_hdv_window> W(new pdmpc_hdv_window);
    S = place(m, A, 0.75);
    int nw = pdmpc_hdv_build_window(&M, &A, &S, 2.0, W.get());
    CHECK(nw == 3 && W->start[0] == -0.75 && W->start[1] == 0.25 && W->start[2] == 1.25 && W->ax[1] == 1.0 && W->ax[2] == 2.0);
    nw = pdmpc_hdv_build_window(&M, &A, &S, 100.0, W.get());
    CHECK(nw == 4 && W->start[3] == 2.25);
    nw = pdmpc_hdv_build_window(&M, &A, &S, 0.2, W.get());
    CHECK(nw == 1);
    // the cap: 100 segments of 0.01 m inside a look-ahead of 2 m
    S = place(m, B, 0.005);
    nw = pdmpc_hdv_build_window(&M, &B, &S, 2.0, W.get());
    CHECK(nw == PDMPC_HDV_WINDOW_MAX && W->start[0] == -0.005 && std::fabs(W->start[63] + W->len[63] - 0.635) < 1e-12);
    S = place(m, B, 0.505);
    nw = pdmpc_hdv_build_window(&M, &B, &S, 2.0, W.get());
    CHECK(nw == 50);  // (the open route ends it)
    // the wrap of a closed route, window and walk (the joints of the ring are 0.5 m long)
    S = place(m, C, 4.9);
    CHECK(S.r == 1 && S.j == 2);
    nw = pdmpc_hdv_build_window(&M, &C, &S, 1.0, W.get());
    CHECK(nw == 2 && W->ax[1] == 0.0 && W->ay[1] == 9.0);
    CHECK(pdmpc_hdv_walk(&M, &C, &S, 0.2) == 0 && S.r == 0 && S.j == 0 && std::fabs(S.u - 0.1) < 1e-12);
    CHECK(pdmpc_hdv_walk(&M, &C, &S, 50.0) == 0 && S.r == 0 && S.j == 0);  // ten times round
}

// one step of a member with arrays of exactly the sizes
struct Step {
    std::vector<int32_t> seg;
    std::vector<double> u, x, y, c, s, speed, gap;
};
Step drive(const Map& m, const Routes& R, const std::vector<pdmpc_hdv_drive_state>& S, const std::vector<double>& tdx, const std::vector<double>& v_des,
           const std::vector<double>& cx, const std::vector<double>& cy, const std::vector<double>& ctx, const double* par, double dt) {
    const int n = R.n(), nc = (int)cx.size();
    std::vector<int32_t> seg((size_t)2 * n);
    std::vector<double> u((size_t)n), tdy((size_t)n, 0.0), cty((size_t)nc, 0.0);
    for (int h = 0; h < n; ++h) {
        seg[(size_t)h] = S[(size_t)h].r;
        seg[(size_t)(n + h)] = S[(size_t)h].j;
        u[(size_t)h] = S[(size_t)h].u;
    }
    std::string why;
    CHECK(hdv_check_states(m.data, n, R.off.data(), R.id.data(), R.closed.data(), seg.data(), seg.data() + n, u.data(), &why) == PDMPC_OK);
    CHECK(hdv_check_drive(par, dt, n, v_des.data(), &why) == PDMPC_OK);
    Step o;
    o.seg.resize((size_t)2 * n);
    for (auto* v : {&o.u, &o.x, &o.y, &o.c, &o.s, &o.speed, &o.gap}) v->resize((size_t)n);
    hdv_drive_member(m.data.view(), n, R.off.data(), R.id.data(), R.closed.data(), seg.data(), u.data(), tdx.data(), tdy.data(), v_des.data(), nc, cx.data(), cy.data(), ctx.data(),
                     cty.data(), par, dt, o.seg.data(), o.u.data(), o.x.data(), o.y.data(), o.c.data(), o.s.data(), o.speed.data(), o.gap.data());
    return o;
}

void check_steps(const Map& m) {
    const double par[4] = {2.0, 0.3, 1.0, 0.125};
    Routes R;
    R.add({1, 2}, false);
    const pdmpc_hdv_route A = hdv_route(R.off.data(), R.id.data(), R.closed.data(), 0);
    const std::vector<pdmpc_hdv_drive_state> S = {place(m, A, 0.5)};
    // free road; the pose is the point reached and the segment's direction
    Step o = drive(m, R, S, {0.0}, {0.5}, {}, {}, {}, par, 0.2);
    CHECK(o.speed[0] == 0.5 && std::isinf(o.gap[0]) && o.u[0] == 0.6 && o.x[0] == 0.6 && o.y[0] == 0.0 && o.c[0] == 1.0 && o.s[0] == 0.0);
    // a CAV 0.7 m ahead behind the segment of length 0: slowed to (0.7 - 0.3) / 1
    o = drive(m, R, S, {0.0}, {0.5}, {1.2}, {0.0}, {0.0}, par, 0.2);
    CHECK(o.gap[0] == 0.7 && std::fabs(o.speed[0] - 0.4) < 1e-15);
    // at gap_min exactly: it stands; beside the route at `lateral` exactly: seen, beyond it: not; behind: not; on another tile: not
    o = drive(m, R, S, {0.0}, {0.5}, {0.8}, {0.0}, {0.0}, par, 0.2);
    CHECK(o.gap[0] == 0.30000000000000004 || o.gap[0] == 0.3);
    o = drive(m, R, S, {0.0}, {0.5}, {0.75}, {0.0}, {0.0}, par, 0.2);
    CHECK(o.gap[0] == 0.25 && o.speed[0] == 0.0 && o.u[0] == 0.5);
    o = drive(m, R, S, {0.0}, {0.5}, {0.75}, {0.125}, {0.0}, par, 0.2);
    CHECK(o.gap[0] == 0.25);
    o = drive(m, R, S, {0.0}, {0.5}, {0.75}, {0.126}, {0.0}, par, 0.2);
    CHECK(std::isinf(o.gap[0]) && o.speed[0] == 0.5);
    o = drive(m, R, S, {0.0}, {0.5}, {0.25}, {0.0}, {0.0}, par, 0.2);
    CHECK(std::isinf(o.gap[0]));
    o = drive(m, R, S, {0.0}, {0.5}, {0.75}, {0.0}, {12.0}, par, 0.2);
    CHECK(std::isinf(o.gap[0]));
    o = drive(m, R, S, {12.0}, {0.5}, {12.75}, {0.0}, {12.0}, par, 0.2);
    CHECK(o.gap[0] == 0.25 && o.x[0] == 12.5);
    // the end of the open route: speed 0 there
    o = drive(m, R, {place(m, A, 3.95)}, {0.0}, {0.5}, {}, {}, {}, par, 0.2);
    CHECK(o.speed[0] == 0.0 && o.seg[0] == 1 && o.seg[1] == 1 && o.u[0] == 1.0 && o.x[0] == 4.0);
    // two HDVs: the follower's gap is to where the leader stood, in either order of the call
    Routes R2;
    R2.add({1, 2}, false);
    R2.add({1, 2}, false);
    o = drive(m, R2, {place(m, A, 0.25), place(m, A, 0.75)}, {0.0, 0.0}, {0.5, 0.5}, {}, {}, {}, par, 0.2);
    CHECK(o.gap[0] == 0.5 && std::isinf(o.gap[1]) && std::fabs(o.speed[0] - 0.2) < 1e-15 && o.speed[1] == 0.5);
    Step p = drive(m, R2, {place(m, A, 0.75), place(m, A, 0.25)}, {0.0, 0.0}, {0.5, 0.5}, {}, {}, {}, par, 0.2);
    CHECK(p.gap[1] == o.gap[0] && p.u[1] == o.u[0] && p.u[0] == o.u[1]);
    // the refusals of a step
    std::string why;
    const double bad[4] = {2.0, 0.3, 0.1, 0.125}, v[1] = {0.5}, neg[1] = {-0.5};
    CHECK(hdv_check_drive(bad, 0.2, 1, v, &why) == PDMPC_ERR_INVALID && why.find("headway < dt") == 0);
    CHECK(hdv_check_drive(par, 0.2, 1, neg, &why) == PDMPC_ERR_INVALID && hdv_check_drive(par, 0.0, 1, v, &why) == PDMPC_ERR_INVALID);
    const int32_t seg_bad[2] = {1, 2};  // (lanelet 2 of the open route has two segments)
    const double u0[1] = {0.0};
    CHECK(hdv_check_states(m.data, 1, R.off.data(), R.id.data(), R.closed.data(), seg_bad, seg_bad + 1, u0, &why) == PDMPC_ERR_INVALID);
}
}  // namespace

int main() {
    const Map m;
    check_route_rules(m);
    check_walk_and_window(m);
    check_steps(m);
    std::printf("hdv drive checks ok\n");
    return 0;
}
