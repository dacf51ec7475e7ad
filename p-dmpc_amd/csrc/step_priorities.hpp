// step_priorities.hpp — from couplings to a prioritization (step_controller.cpp, stage 4 of 9): computation levels, the colouring, the
// grouping with its weighers and cutter, random priorities, the level permutations of the explorative step, the unique prioritizations
// of the optimal-priority step.  Plain arrays and Lists in, plain arrays out: nothing of the controller's state is known here.
// What it restates (file:line relative to the reference root):
//   priorities -> DAG         ConstantPrioritizer.m:14-20, Prioritizer.m:36-77, ColoringPrioritizer.m:11-131, RandomPrioritizer.m:15-25
//   grouping                  PrioritizedController.group (hlc/controller/prioritized/PrioritizedController.m:375-389),
//                             weight/DistanceWeigher.m:12-39, weight/ConstantWeigher.m:15-17, weight/RandomWeigher.m:13-21,
//                             cut/GreedyCutter.m:5-86
//   computation levels        utility/kahn.m:1-24
//   level permutations        PrioritizedExplorativeController.computation_level_permutations (:241-309)
//   unique prioritizations    Prioritizer.unique_priorities (Prioritizer.m:97-140)
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>

#include "mt19937ar.hpp"
#include "step_types.hpp"

namespace {
// utility/kahn.m:1-24: computation level (1-based) of every vertex of a DAG given as successor lists (false: a cycle)
struct KahnScratch { std::vector<int> indeg, cur, next; };
inline bool kahn_lists(const Lists& succ, int n, std::vector<int32_t>& L, KahnScratch& K) {
    L.assign(n, 0);
    K.indeg.assign(n, 0);
    K.cur.clear();
    for (int32_t j : succ.idx) ++K.indeg[j];
    for (int j = 0; j < n; ++j)
        if (K.indeg[j] == 0) K.cur.push_back(j);
    int n_done = 0, level = 1;
    while (n_done < n) {
        if (K.cur.empty()) return false;  // a cycle
        K.next.clear();
        for (int v : K.cur) {
            L[v] = level;
            ++n_done;
        }
        for (int v : K.cur)
            for (const int32_t* q = succ.begin(v); q != succ.end(v); ++q)
                if (--K.indeg[*q] == 0) K.next.push_back(*q);
        K.cur.swap(K.next);
        ++level;
    }
    return true;
}

// ColoringPrioritizer.prioritize (:11-27): directed coupling from a colouring of the undirected graph
inline void coloring_directed(const std::vector<uint8_t>& adjacency, int n, std::vector<uint8_t>& directed) {
    // neighbour lists of the graph without self-loops; the degrees the selection compares are the matrix's column sums (:38-45)
    Lists nb;
    nb.off.assign((size_t)n + 1, 0);
    nb.idx.clear();
    std::vector<int> degree(n, 0), color(n, 0);
    std::vector<long> deg(n, 0);  // column counts of the matrix as given (order_topo, :93)
    for (int i = 0; i < n; ++i) {
        for_each_set(adjacency.data() + (size_t)i * n, n, [&](int j) {
            ++deg[j];
            if (j == i) return;
            nb.idx.push_back(j);
            degree[j] += adjacency[(size_t)i * n + j];
        });
        nb.off[i + 1] = (int32_t)nb.idx.size();
    }
    for (int i = 0; i < n; ++i)
        if (degree[i] == 0) color[i] = 1;  // :45
    // per vertex the distinct colours its neighbours carry, as a bit set (kept up to date as vertices are coloured: the selection
    // below is then a scan of the vertices, not of the matrix — 512 vehicles: 63 ms -> well under 1 ms per step)
    const int cw = (n + 2 + 63) / 64;
    std::vector<int> ncol(n, 0);                   // distinct colours among the coloured neighbours
    std::vector<uint64_t> has((size_t)n * cw, 0);  // bit c of has[i]: a neighbour of i carries colour c
    auto mark = [&](int j, int col) {
        uint64_t& w = has[(size_t)j * cw + (col >> 6)];
        const uint64_t bit = 1ull << (col & 63);
        if (!(w & bit)) {
            w |= bit;
            ++ncol[j];
        }
    };
    // vertex_sdo_ldo (:65-89) scans the uncoloured vertices for the most distinct neighbour colours and, among equals, moves on to
    // a vertex only if its degree is strictly larger than the current pick's: the pick is the first uncoloured vertex with the
    // largest (colours, degree) pair.  key = that pair for an uncoloured vertex, -1 for a coloured one.
    // The largest key is found over blocks of 32 vertices whose maxima are kept up to date (keys of uncoloured vertices only grow;
    // the picked vertex's block is rescanned).
    constexpr int KB = 32;
    const int nblk = (n + KB - 1) / KB;
    std::vector<int64_t> key(n), bmax((size_t)nblk, -1);
    auto key_of = [&](int i) { return color[i] != 0 ? (int64_t)-1 : ((int64_t)ncol[i] << 32) | (int64_t)(uint32_t)degree[i]; };
    int left = 0;
    for (int i = 0; i < n; ++i) left += color[i] == 0;
    for (int i = 0; i < n; ++i)
        if (color[i] != 0)
            for (const int32_t* q = nb.begin(i); q != nb.end(i); ++q) mark(*q, color[i]);
    for (int i = 0; i < n; ++i) {
        key[i] = key_of(i);
        bmax[i / KB] = std::max(bmax[i / KB], key[i]);
    }
    while (left > 0) {
        int blk = 0;
        for (int b = 1; b < nblk; ++b)
            if (bmax[b] > bmax[blk]) blk = b;  // the first block that holds the largest key
        int idx = blk * KB;
        while (key[idx] != bmax[blk]) ++idx;
        int cpick = 1;
        while (has[(size_t)idx * cw + (cpick >> 6)] >> (cpick & 63) & 1) ++cpick;  // the smallest colour no neighbour carries
        color[idx] = cpick;
        --left;
        key[idx] = -1;
        bmax[blk] = -1;
        for (int i = blk * KB; i < std::min(n, blk * KB + KB); ++i) bmax[blk] = std::max(bmax[blk], key[i]);
        for (const int32_t* q = nb.begin(idx); q != nb.end(idx); ++q) {
            const int j = *q;
            mark(j, cpick);
            key[j] = key_of(j);
            bmax[j / KB] = std::max(bmax[j / KB], key[j]);
        }
    }
    // level matrix rows = colours in ascending order; order_topo (:91-131)
    int cmax = 0;
    for (int i = 0; i < n; ++i) cmax = std::max(cmax, color[i]);
    std::vector<int> row_of_colour((size_t)cmax + 1, -1);
    for (int i = 0; i < n; ++i) row_of_colour[color[i]] = 0;
    int nl = 0;
    for (int col = 0; col <= cmax; ++col)
        if (row_of_colour[col] == 0) row_of_colour[col] = nl++;
    std::vector<int> row(n);  // the level-matrix row a vertex stands in
    for (int v = 0; v < n; ++v) row[v] = row_of_colour[color[v]];
    std::vector<int> order;
    std::vector<int> place((size_t)nl, -1);  // position of a row in `order`
    long total = 0;
    for (long d : deg) total += d;
    if (total == 0) {
        for (int g = 0; g < nl; ++g) order.push_back(g);
    } else {
        while (total != 0) {
            int max_idx = 0;
            for (int i = 1; i < n; ++i)
                if (deg[i] > deg[max_idx]) max_idx = i;  // first index of the maximum
            const int lvl = row[max_idx];
            order.push_back(lvl);
            for (int i = 0; i < n; ++i)
                if (row[i] == lvl) deg[i] = 0;
            total = 0;
            for (long d : deg) total += d;
        }
        for (int g = 0; g < nl; ++g)
            if (std::find(order.begin(), order.end(), g) == order.end()) order.push_back(g);
    }
    for (size_t q = 0; q < order.size(); ++q)
        if (place[order[q]] < 0) place[order[q]] = (int)q;  // (find: the first position)
    std::vector<int> level(n, 0);
    for (int v = 0; v < n; ++v) level[v] = place[row[v]] + 1;
    directed.assign((size_t)n * n, 0);
    for (int i = 0; i < n; ++i)
        for_each_set(adjacency.data() + (size_t)i * n, n, [&](int j) {
            if (i != j && !(level[i] > level[j])) at(directed, n, i, j) = 1;  // Prioritizer.m:52-55
        });
}

// PrioritizedController.group (:375-389): weigh + GreedyCutter.cut (cut/GreedyCutter.m:5-86)
// (dir_succ / dir_pred: `directed` as lists by row / by column; uncut = nothing had to be cut: seq is `directed` and L its levels)
// G: what it reads of a controller -- the depth limit, and the weigher with the inputs of its strategy
struct Grouping {
    int max_num_CLs, weight_strategy;
    const std::vector<double>& trim_speed;  // DistanceWeigher: the trims' speeds, the time step's length and the horizon
    double dt_seconds;
    int Hp;
    const std::vector<double>&x, &y;        // ... and the measured positions
    int time_step;                          // RandomWeigher's seed
};
inline bool group(int n, const Grouping& G, const std::vector<uint8_t>& directed, const Lists& dir_succ, const Lists& dir_pred, KahnScratch& K, std::vector<uint8_t>& seq,
           std::vector<int32_t>& L, bool& uncut) {
    uncut = false;
    if (!kahn_lists(dir_succ, n, L, K)) return false;
    int depth = 0;
    for (int v : L) depth = std::max(depth, v);
    if (depth <= G.max_num_CLs) {
        seq = directed;  // every sub-graph of the DAG is at most as deep: the cutter accepts every edge
        uncut = true;
        return true;
    }
    seq.assign((size_t)n * n, 0);
    if (G.max_num_CLs == 1) return true;
    // weights; [row, col] = find(M): column-major order
    struct Edge { int a, b; double w; };
    std::vector<Edge> edges;
    const double vmax = *std::max_element(G.trim_speed.begin(), G.trim_speed.end());
    const double max_distance = 2 * vmax * G.dt_seconds * G.Hp;
    Mt19937ar rng((uint32_t)G.time_step);  // RandomWeigher (weight/RandomWeigher.m:13-21): one draw per edge in find() order, seeded with the time step
    for (int b = 0; b < n; ++b)
        for (const int32_t* q = dir_pred.begin(b); q != dir_pred.end(b); ++q) {
            const int a = *q;
            double w = 0.5;  // ConstantWeigher
            if (G.weight_strategy == PDMPC_WEIGHT_DISTANCE) {
                const double dx = G.x[a] - G.x[b], dy = G.y[a] - G.y[b];
                w = 1 - std::sqrt(dx * dx + dy * dy) / max_distance;
            } else if (G.weight_strategy == PDMPC_WEIGHT_RANDOM) {
                w = rng.rand();
            }
            if (w != 0) edges.push_back({a, b, w});  // (find() on the weighted matrix skips exact zeros)
        }
    std::stable_sort(edges.begin(), edges.end(), [](const Edge& p, const Edge& q) { return p.w > q.w; });
    // GreedyCutter.cut (:25-86) accepts an edge if the graph stays acyclic and at most max_num_CLs levels deep.  The levels are
    // longest-path layers (kahn), edges are only ever added, so the layers only grow: instead of a trial copy of the matrix and a
    // kahn pass per edge (128 vehicles: 6 ms per step), the new layers are relaxed from the edge's head through the accepted
    // successors; reaching the edge's tail again is a cycle, a layer beyond the limit a rejection (both undo the relaxation).
    std::vector<int32_t> levels((size_t)n, 1);  // (kahn of the graph without edges)
    std::vector<std::vector<int>> succ(n);
    std::vector<std::pair<int, int32_t>> undo;
    std::vector<int> work;
    for (const Edge& e : edges) {
        if (levels[e.a] < levels[e.b]) {
            at(seq, n, e.a, e.b) = 1;
            succ[e.a].push_back(e.b);
            continue;
        }
        undo.clear();
        work.clear();
        bool ok = levels[e.a] + 1 <= G.max_num_CLs;
        if (ok) {
            undo.emplace_back(e.b, levels[e.b]);
            levels[e.b] = levels[e.a] + 1;
            work.push_back(e.b);
        }
        while (ok && !work.empty()) {
            const int u = work.back();
            work.pop_back();
            for (int w : succ[u]) {
                if (levels[w] >= levels[u] + 1) continue;
                if (w == e.a || levels[u] + 1 > G.max_num_CLs) {  // a cycle / too deep
                    ok = false;
                    break;
                }
                undo.emplace_back(w, levels[w]);
                levels[w] = levels[u] + 1;
                work.push_back(w);
            }
        }
        if (ok) {
            at(seq, n, e.a, e.b) = 1;
            succ[e.a].push_back(e.b);
        } else {
            for (auto it = undo.rbegin(); it != undo.rend(); ++it) levels[it->first] = it->second;
        }
    }
    return true;
}

// Prioritizer.directed_coupling_from_priorities (Prioritizer.m:64-77): keep i -> j iff priority(j) is not below priority(i)
inline void direct_by(const std::vector<uint8_t>& adjacency, int n, const int32_t* prio, std::vector<uint8_t>& directed) {
    directed.assign((size_t)n * n, 0);
    for (int i = 0; i < n; ++i)
        for_each_set(adjacency.data() + (size_t)i * n, n, [&](int j) {
            if (!(prio[j] < prio[i])) at(directed, n, i, j) = 1;
        });
}

// RandomPrioritizer.m:15-25 (prioritizer.random_priorities): a Fisher-Yates shuffle of 1 .. n on the mt19937ar doubles of the time step
inline void random_priorities(int time_step, int n, std::vector<int32_t>& p) {
    Mt19937ar rng((uint32_t)time_step);
    for (int i = n - 1; i > 0; --i) {
        const int j = (int)(rng.rand() * (i + 1));
        std::swap(p[i], p[j]);
    }
}

// PrioritizedExplorativeController.computation_level_permutations (:241-309): n_perm x n_levels table, row-major, row 0 = 1..n;
// rows up to n_levels form a Latin square built "fewest possibilities first" with random choices from
// RandStream("mt19937ar", Seed = seed) / randi (:249, :283-286), a row that meets a dead end is drawn again; further rows
// (the reference stops at n_levels; BASELINE config C5 asks for 64) are Fisher-Yates shuffles from the same stream.
// The twin of pdmpc.explorative.computation_level_permutations (behind pdmpc_exploration_permutations, which checks the arguments).
inline void exploration_permutations(int32_t n_levels, int32_t n_perm, uint32_t seed, int32_t* out) {
    Mt19937ar rng(seed);
    const int n = n_levels;
    std::vector<std::vector<int32_t>> rows;
    rows.emplace_back();
    for (int j = 0; j < n; ++j) rows[0].push_back(j + 1);
    while ((int)rows.size() < std::min(n_perm, n_levels)) {
        std::vector<uint8_t> allowed((size_t)n * n, 1);  // [level][class]
        for (int col = 0; col < n; ++col)
            for (const auto& r : rows) allowed[(size_t)(r[(size_t)col] - 1) * n + col] = 0;
        std::vector<int32_t> perm((size_t)n, 0);
        bool ok = true;
        for (int filled = 0; filled < n && ok; ++filled) {
            int best_col = 0, best_cnt = n + 1;
            for (int col = 0; col < n; ++col) {  // [n_possibilities, i_cell] = min(sum(is_level_allowed, 1)): the first minimum
                int cnt = 0;
                for (int l = 0; l < n; ++l) cnt += allowed[(size_t)l * n + col];
                if (cnt < best_cnt) {
                    best_cnt = cnt;
                    best_col = col;
                }
            }
            if (best_cnt == 0) {
                ok = false;
                break;
            }
            const int pick = rng.randi(best_cnt);  // 1-based position among find(is_level_allowed(:, i_cell))
            int lvl = -1;
            for (int l = 0, seen = 0; l < n; ++l)
                if (allowed[(size_t)l * n + best_col] && ++seen == pick) {
                    lvl = l;
                    break;
                }
            perm[(size_t)best_col] = lvl + 1;
            for (int col = 0; col < n; ++col) allowed[(size_t)lvl * n + col] = 0;
            for (int l = 0; l < n; ++l) allowed[(size_t)l * n + best_col] = 1;
        }
        if (ok) rows.push_back(perm);
    }
    while ((int)rows.size() < n_perm) {
        std::vector<int32_t> perm((size_t)n);
        for (int j = 0; j < n; ++j) perm[(size_t)j] = j + 1;
        for (int i = n - 1; i > 0; --i) std::swap(perm[(size_t)i], perm[(size_t)(rng.randi(i + 1) - 1)]);
        rows.push_back(perm);
    }
    for (int p = 0; p < n_perm; ++p)
        for (int j = 0; j < n; ++j) out[(size_t)p * n + j] = rows[(size_t)p][(size_t)j];
}

// Prioritizer.unique_priorities (Prioritizer.m:97-140) on the host: the twin of the device enumeration (csrc/priority_kernel.hip) and its
// checker.  Every orientation is tested by peeling its sources off vertex by vertex over explicit edge lists (the kernel peels bit sets);
// the priorities follow the smallest-index-first topological order (toposort(..., 'Order', 'stable')).
// the enumeration behind pdmpc_unique_priorities_host and its grouped sibling (arguments checked by them): PDMPC_OK, or
// PDMPC_ERR_CAPACITY with *why set
inline int enumerate_on_host(int32_t n, const uint8_t* adjacency, int64_t max_out, int64_t* n_out, uint32_t* masks, int32_t* priorities, const char** why) {
    *n_out = -1;
    *why = "more than 64 vehicles";
    if (n > 64) return PDMPC_ERR_CAPACITY;
    std::vector<int> er, ec;  // [edge_row, edge_col] = find(triu(adjacency, 1)): by column, then by row
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < c; ++r)
            if (adjacency[(size_t)r * n + c]) {
                er.push_back(r);
                ec.push_back(c);
            }
    const int E = (int)er.size();
    *why = "more than 32 coupling edges";
    if (E > 32) return PDMPC_ERR_CAPACITY;
    const uint64_t n_masks = 1ull << E;
    std::vector<int> head((size_t)E), tail((size_t)E), indeg((size_t)n), order((size_t)n);
    std::vector<uint8_t> placed((size_t)n);
    // the lexicographically smallest topological order of orientation m, false if m has a cycle (Kahn, smallest available vertex first)
    auto toposort = [&](uint64_t m) {
        std::fill(indeg.begin(), indeg.end(), 0);
        for (int e = 0; e < E; ++e) {
            const bool flip = (m >> (E - 1 - e)) & 1u;  // dec2bin(m, E) == '1': edge 1 is the most significant bit
            tail[(size_t)e] = flip ? ec[(size_t)e] : er[(size_t)e];
            head[(size_t)e] = flip ? er[(size_t)e] : ec[(size_t)e];
            ++indeg[(size_t)head[(size_t)e]];
        }
        std::fill(placed.begin(), placed.end(), 0);
        for (int pos = 0; pos < n; ++pos) {
            int v = 0;
            while (v < n && (placed[(size_t)v] || indeg[(size_t)v] != 0)) ++v;
            if (v == n) return false;
            placed[(size_t)v] = 1;
            order[(size_t)pos] = v;
            for (int e = 0; e < E; ++e)
                if (tail[(size_t)e] == v) --indeg[(size_t)head[(size_t)e]];
        }
        return true;
    };
    int64_t K = 0;
    for (uint64_t m = 0; m < n_masks; ++m) {
        if (!toposort(m)) continue;
        if (K < max_out) {
            masks[K] = (uint32_t)m;
            for (int pos = 0; pos < n; ++pos) priorities[(size_t)K * n + order[(size_t)pos]] = pos + 1;  // priority(topological_order) = 1:n
        }
        ++K;
    }
    *n_out = K;
    *why = "more unique prioritizations than max_out";
    if (K > max_out) return PDMPC_ERR_CAPACITY;
    return PDMPC_OK;
}
}  // namespace
