// mpa_reach.hpp — where the automaton can go (include/pdmpc_reach.h): its reach (Dmax, Amax), its reach rectangles per trim and step, and the
// host twins of the kernel's reach lists under both rules.  Pure geometry over a pdmpc_mpa.  Host only: no HIP header, no handle, no device —
// pdmpc_upload_mpa (api.cpp) writes the reach and the rectangles behind the maneuver areas, and the *_host entry points of include/pdmpc.h check
// their arguments and call in here.  `make host-parts` compiles this header alone with the host compiler; tests/host_only_checks.cpp checks it
// against an enumeration of every trim path.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pdmpc.h"
#include "../../include/pdmpc_math.h"
#include "../../include/pdmpc_reach.h"

// The automaton's reach (include/pdmpc_reach.h): the longest maneuver displacement and the largest |area point| over the used columns
// of the three area variants.
inline void mpa_reach(const pdmpc_mpa* mpa, double& dmax, double& amax) {
    dmax = 0.0;
    amax = 0.0;
    for (int t = 0; t < mpa->n_maneuvers; ++t) {
        const pdmpc_maneuver& m = mpa->maneuvers[t];
        dmax = std::max(dmax, hypot(m.dx, m.dy));
        const double(*src[3])[PDMPC_VMAX] = {m.area, m.area_without_offset, m.area_large_offset};
        for (int a = 0; a < 3; ++a)
            for (int v = 0; v < m.n_cols && v < PDMPC_VMAX; ++v) amax = std::max(amax, hypot(src[a][0][v], src[a][1][v]));
    }
}

// The automaton's reach rectangles (include/pdmpc_reach.h, the oriented rule): rects[(r * Hp + K - 1) * 4 ..] = (x_lo, x_hi, y_lo, y_hi), in
// the frame of a root at the origin with yaw 0 in trim r, of every point of every area (three variants, used columns) of a maneuver
// of step K that the transition masks of steps 1 .. K allow; NaN where no such maneuver exists.  Paths are not enumerated: convex
// hulls compose — hull(i, k -> K) = hull of the union over the successors j of i at step k of maneuver(i, j) applied to
// hull(j, k + 1 -> K), the areas of the maneuvers leaving i at step K being the base case — and the bounding box of the hull is the
// bounding box of the union.  n * Hp^2 / 2 hulls of a few hundred points.
typedef std::pair<double, double> ReachPt;
// convex hull in place (Andrew's monotone chain; collinear points dropped, which moves no bounding box)
inline void reach_hull(std::vector<ReachPt>& P, std::vector<ReachPt>& H) {
    std::sort(P.begin(), P.end());
    P.erase(std::unique(P.begin(), P.end()), P.end());
    const size_t n = P.size();
    if (n < 3) return;
    auto cross = [](const ReachPt& o, const ReachPt& a, const ReachPt& b) { return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first); };
    H.clear();
    for (size_t i = 0; i < n; ++i) {
        while (H.size() >= 2 && cross(H[H.size() - 2], H.back(), P[i]) <= 0) H.pop_back();
        H.push_back(P[i]);
    }
    const size_t lower = H.size() + 1;
    for (size_t i = n - 1; i-- > 0;) {
        while (H.size() >= lower && cross(H[H.size() - 2], H.back(), P[i]) <= 0) H.pop_back();
        H.push_back(P[i]);
    }
    H.pop_back();
    P.swap(H);
}
inline void mpa_reach_rects(const pdmpc_mpa* mpa, int Hp, double* rects) {
    const int n = mpa->n_trims, T = mpa->n_maneuvers;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> cs((size_t)std::max(T, 1)), sn((size_t)std::max(T, 1));
    for (int t = 0; t < T; ++t) pdmpc_sincos(mpa->maneuvers[t].dyaw, &sn[t], &cs[t]);
    auto maneuver = [&](int k, int i, int j) {  // of step k (1-based) from trim i to trim j, or -1
        if (!mpa->transition[((size_t)(k - 1) * n + i) * n + j]) return -1;
        const int t = mpa->maneuver_index[(size_t)i * n + j];
        return t >= 0 && t < T ? t : -1;
    };
    // (hull(i, k -> K) depends on the masks of steps k .. K alone, and most steps share one mask — the recursive-feasibility mask differs
    // near the horizon only —: a table per distinct sequence of masks, not per (k, K))
    std::vector<int> slice((size_t)Hp);
    for (int k = 0; k < Hp; ++k) {
        slice[k] = k;
        for (int q = 0; q < k; ++q)
            if (!memcmp(mpa->transition + (size_t)q * n * n, mpa->transition + (size_t)k * n * n, (size_t)n * n)) {
                slice[k] = slice[q];
                break;
            }
    }
    typedef std::vector<std::vector<ReachPt>> Table;  // one hull per trim
    std::map<std::vector<int>, size_t> known;
    std::vector<Table> tables;
    std::vector<ReachPt> scratch;
    for (int K = 1; K <= Hp; ++K) {
        size_t at = 0;
        for (int k = K; k >= 1; --k) {
            const std::vector<int> key(slice.begin() + (k - 1), slice.begin() + K);
            const auto found = known.find(key);
            if (found != known.end()) {
                at = found->second;
                continue;
            }
            Table t((size_t)n);
            for (int i = 0; i < n; ++i) {
                for (int j = 0; j < n; ++j) {
                    const int mi = maneuver(k, i, j);
                    if (mi < 0) continue;
                    const pdmpc_maneuver& m = mpa->maneuvers[mi];
                    if (k == K) {
                        const double(*src[3])[PDMPC_VMAX] = {m.area, m.area_without_offset, m.area_large_offset};
                        for (int a = 0; a < 3; ++a)
                            for (int v = 0; v < m.n_cols && v < PDMPC_VMAX; ++v) t[i].push_back(ReachPt(src[a][0][v], src[a][1][v]));
                    } else {
                        for (const ReachPt& p : tables[at][j]) t[i].push_back(ReachPt(cs[mi] * p.first - sn[mi] * p.second + m.dx, sn[mi] * p.first + cs[mi] * p.second + m.dy));
                    }
                }
                reach_hull(t[i], scratch);
            }
            at = tables.size();
            tables.push_back(std::move(t));
            known[key] = at;
        }
        const Table& cur = tables[at];
        for (int i = 0; i < n; ++i) {
            double* r = rects + ((size_t)i * Hp + (K - 1)) * 4;
            r[0] = r[1] = r[2] = r[3] = qnan;
            for (const ReachPt& p : cur[i]) {
                r[0] = p.first < r[0] || r[0] != r[0] ? p.first : r[0];
                r[1] = p.first > r[1] || r[1] != r[1] ? p.first : r[1];
                r[2] = p.second < r[2] || r[2] != r[2] ? p.second : r[2];
                r[3] = p.second > r[3] || r[3] != r[3] ? p.second : r[3];
            }
        }
    }
}

// The reach lists of one search under the disc rule (pdmpc_reach_box, pdmpc_reach_in), as pdmpc_reach_lists_host returns them: per step k the
// segments j of its soup (columns step_first[k - 1] .. + step_count[k - 1] of x, y) that are in reach.  A step of fewer than two columns has
// no segment and lists nothing.
inline int reach_lists(int Hp, double dmax, double amax, double root_x, double root_y, const double* x, const double* y, const int32_t* step_first, const int32_t* step_count,
                       int32_t* list_offset, int32_t* list, std::string& err) {
    int32_t n = 0;
    for (int k = 1; k <= Hp; ++k) {
        const int32_t a = step_first[k - 1], c = step_count[k - 1];
        if (a < 0 || c < 0 || (c > 1 && (!x || !y || !list))) {
            err = "pdmpc_reach_lists_host: bad step ranges";
            return PDMPC_ERR_INVALID;
        }
        double box[4];
        pdmpc_reach_box(dmax, amax, k, root_x, root_y, box);
        list_offset[k - 1] = n;
        for (int32_t j = 0; j + 1 < c; ++j)
            if (pdmpc_reach_in(x[a + j], y[a + j], x[a + j + 1], y[a + j + 1], box[0], box[1], box[2], box[3])) list[n++] = j;
    }
    list_offset[Hp] = n;
    return PDMPC_OK;
}

// ... under the oriented rule (pdmpc_reach_rect_box, pdmpc_reach_in_oriented) with the rectangles of mpa_reach_rects, as
// pdmpc_reach_lists_oriented_host returns them; root_trim is 1-based
inline int reach_lists_oriented(int Hp, const double* rects, int root_trim, double root_x, double root_y, double root_yaw, const double* x, const double* y, const int32_t* step_first,
                                const int32_t* step_count, int32_t* list_offset, int32_t* list, std::string& err) {
    double cs, sn;
    pdmpc_sincos(root_yaw, &sn, &cs);
    int32_t n = 0;
    for (int k = 1; k <= Hp; ++k) {
        const int32_t a = step_first[k - 1], c = step_count[k - 1];
        if (a < 0 || c < 0 || (c > 1 && (!x || !y || !list))) {
            err = "pdmpc_reach_lists_oriented_host: bad step ranges";
            return PDMPC_ERR_INVALID;
        }
        double box[4];
        pdmpc_reach_rect_box(rects + ((size_t)(root_trim - 1) * Hp + (k - 1)) * 4, root_x, root_y, box);
        list_offset[k - 1] = n;
        for (int32_t j = 0; j + 1 < c; ++j)
            if (pdmpc_reach_in_oriented(x[a + j], y[a + j], x[a + j + 1], y[a + j + 1], root_x, root_y, cs, sn, box[0], box[1], box[2], box[3])) list[n++] = j;
    }
    list_offset[Hp] = n;
    return PDMPC_OK;
}
