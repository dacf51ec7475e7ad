// fca.cpp — the host twin of the future collision assessment (FcaPrioritizer.m:11-92) and the parts it shares with
// the device entry points (step_prep.cpp: pdmpc_fca_collisions, pdmpc_fca_collisions_grouped): the argument checks and the stable
// descending sort of the counts; the grouped host twin loops over the ungrouped one.  Host code only; the C++ twin of pdmpc.prioritizer.fca_priorities.  The footprints and the separating-axis test are include/pdmpc_geometry.h,
// which the kernel (fca_kernel.hip) compiles too, so the twin and the kernel decide every test with the same bits.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/pdmpc.h"
#include "../../include/pdmpc_geometry.h"
#include "pdmpc_device.h"

namespace {
bool bad_set(const pdmpc_polygon_set* s) {
    if (!s) return false;
    if (s->n_polygons < 0 || (s->n_polygons > 0 && (!s->offset || !s->x || !s->y))) return true;
    for (int p = 0; p < s->n_polygons; ++p)
        if (s->offset[p + 1] - s->offset[p] < 1 || s->offset[p] < 0) return true;
    return false;
}
}  // namespace

extern "C" {

int pdmpc_fca_check_args(int32_t n, int32_t Hp, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, int32_t n_pairs,
                         const int32_t* pairs, const pdmpc_polygon_set* obstacles, const pdmpc_polygon_set* dynamic_rows, const int32_t* collisions,
                         const int32_t* priorities, const char** why) {
    if (n < 1) return *why = "n must be at least 1", PDMPC_ERR_INVALID;
    if (Hp < 2) return *why = "Hp must be at least 2 (calculate_yaw needs two reference points)", PDMPC_ERR_INVALID;
    if (!x || !y || !cos_yaw || !sin_yaw || !collisions || !priorities) return *why = "null argument", PDMPC_ERR_INVALID;
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return *why = "bad pair list", PDMPC_ERR_INVALID;
    for (int p = 0; p < n_pairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || b >= n || !(a < b)) return *why = "every pair (a, b) needs 0 <= a < b < n", PDMPC_ERR_INVALID;
        if (p > 0) {
            const int pa = pairs[2 * p - 2], pb = pairs[2 * p - 1];
            if (!(pa < a || (pa == a && pb < b))) return *why = "the pairs must be ascending by (a, b) without repeats", PDMPC_ERR_INVALID;
        }
    }
    if (bad_set(obstacles)) return *why = "bad static obstacle set (every polygon needs a vertex)", PDMPC_ERR_INVALID;
    if (bad_set(dynamic_rows)) return *why = "bad dynamic obstacle set (every polygon needs a vertex)", PDMPC_ERR_INVALID;
    if (dynamic_rows && dynamic_rows->n_polygons % Hp != 0) return *why = "dynamic obstacles: n_polygons must be a multiple of Hp", PDMPC_ERR_INVALID;
    return PDMPC_OK;
}

void pdmpc_fca_sort_index(int32_t n, const int32_t* collisions, int32_t* priorities) {
    // [~, current_priorities] = sort(collisions, 'descend') (FcaPrioritizer.m:91): MATLAB's sort is stable
    std::vector<int32_t> idx((size_t)n);
    for (int v = 0; v < n; ++v) idx[v] = v;
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return collisions[a] > collisions[b]; });
    for (int r = 0; r < n; ++r) priorities[r] = idx[r] + 1;
}

int pdmpc_fca_collisions_host(int32_t n, int32_t Hp, const double* x, const double* y, const double* cos_yaw, const double* sin_yaw, int32_t n_pairs,
                              const int32_t* pairs, const pdmpc_polygon_set* obstacles, const pdmpc_polygon_set* dynamic_rows, double length, double width,
                              double offset, int32_t* collisions, int32_t* priorities) {
    const char* why = nullptr;
    if (const int rc = pdmpc_fca_check_args(n, Hp, x, y, cos_yaw, sin_yaw, n_pairs, pairs, obstacles, dynamic_rows, collisions, priorities, &why)) return rc;
    const int m = n * Hp;
    std::vector<double> fp((size_t)8 * m);  // footprint of (v, k) at 8 (v Hp + k): x of the corners, then y
    for (int i = 0; i < m; ++i) pdmpc_fca_footprint(cos_yaw[i], sin_yaw[i], x[i], y[i], length, width, offset, &fp[(size_t)8 * i], &fp[(size_t)8 * i + 4]);
    for (int v = 0; v < n; ++v) collisions[v] = 0;
    auto foot = [&](int v, int k) { return fp.data() + (size_t)8 * ((size_t)v * Hp + k); };
    auto hits = [](const double* f, const pdmpc_polygon_set* s, int q) {
        const int a = s->offset[q], mq = s->offset[q + 1] - a;
        return pdmpc_sat_intersect(f, f + 4, 4, s->x + a, s->y + a, mq) != 0;
    };
    const int n_rows = dynamic_rows ? dynamic_rows->n_polygons / Hp : 0;
    for (int v = 0; v + 1 < n; ++v)  // the reference's outer loop stops at n - 1 (FcaPrioritizer.m:24)
        for (int k = 0; k < Hp; ++k) {
            const double* f = foot(v, k);
            for (int o = 0; obstacles && o < obstacles->n_polygons; ++o) collisions[v] += hits(f, obstacles, o);
            for (int r = 0; r < n_rows; ++r) collisions[v] += hits(f, dynamic_rows, r * Hp + k);
        }
    for (int p = 0; p < n_pairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        for (int k = 0; k < Hp; ++k) {
            const double *fa = foot(a, k), *fb = foot(b, k);
            if (pdmpc_sat_intersect(fa, fa + 4, 4, fb, fb + 4, 4)) {
                collisions[a] += 1;
                collisions[b] += 1;
            }
        }
    }
    pdmpc_fca_sort_index(n, collisions, priorities);
    return PDMPC_OK;
}

int pdmpc_fca_check_groups(int32_t n_groups, const pdmpc_fca_group* groups, int32_t Hp, const double* x, const double* y, const double* cos_yaw,
                           const double* sin_yaw, const int32_t* collisions, const int32_t* priorities, int32_t* n_total, char* why, int32_t why_size) {
    auto refuse = [&](int rc, int g, const char* what) {
        if (g < 0)
            snprintf(why, (size_t)why_size, "%s", what);
        else
            snprintf(why, (size_t)why_size, "group %d: %s", g, what);
        return rc;
    };
    *n_total = 0;
    if (n_groups < 0 || (n_groups > 0 && !groups)) return refuse(PDMPC_ERR_INVALID, -1, "bad groups");
    if (Hp < 2) return refuse(PDMPC_ERR_INVALID, -1, "Hp must be at least 2 (calculate_yaw needs two reference points)");
    int64_t N = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (groups[g].n < 0) return refuse(PDMPC_ERR_INVALID, g, "n must not be negative");
        N += groups[g].n;
    }
    if (N * Hp > INT32_MAX) return refuse(PDMPC_ERR_CAPACITY, -1, "more than 2^31 reference points");
    *n_total = (int32_t)N;
    if (N > 0 && (!x || !y || !cos_yaw || !sin_yaw || !collisions || !priorities)) return refuse(PDMPC_ERR_INVALID, -1, "null argument");
    size_t v0 = 0;
    for (int g = 0; g < n_groups; ++g) {
        const pdmpc_fca_group& G = groups[g];
        if (G.n == 0) continue;  // (legal: nothing to assess, nothing written)
        const size_t i0 = v0 * Hp;
        const char* w = nullptr;
        if (const int rc = pdmpc_fca_check_args(G.n, Hp, x + i0, y + i0, cos_yaw + i0, sin_yaw + i0, G.n_pairs, G.pairs, G.obstacles, G.dynamic_rows, collisions + v0,
                                                priorities + v0, &w))
            return refuse(rc, g, w);
        v0 += (size_t)G.n;
    }
    return PDMPC_OK;
}

int pdmpc_fca_collisions_grouped_host(int32_t n_groups, const pdmpc_fca_group* groups, int32_t Hp, const double* x, const double* y, const double* cos_yaw,
                                      const double* sin_yaw, int32_t* collisions, int32_t* priorities) {
    char why[160];
    int32_t N = 0;
    if (const int rc = pdmpc_fca_check_groups(n_groups, groups, Hp, x, y, cos_yaw, sin_yaw, collisions, priorities, &N, why, (int32_t)sizeof why)) return rc;
    size_t v0 = 0;
    for (int g = 0; g < n_groups; ++g) {
        const pdmpc_fca_group& G = groups[g];
        if (G.n == 0) continue;
        const size_t i0 = v0 * Hp;
        if (const int rc = pdmpc_fca_collisions_host(G.n, Hp, x + i0, y + i0, cos_yaw + i0, sin_yaw + i0, G.n_pairs, G.pairs, G.obstacles, G.dynamic_rows, G.length,
                                                     G.width, G.offset, collisions + v0, priorities + v0))
            return rc;
        v0 += (size_t)G.n;
    }
    return PDMPC_OK;
}

}  // extern "C"
