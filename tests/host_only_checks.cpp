// host_only_checks.cpp — the host-only parts of p-dmpc_amd/csrc (reference_tree.hpp, mpa_reach.hpp, choice_host.hpp, and launch_plan.hpp's sampled
// scratch and pending seeds) against expectations that do not share their rules: a literal best-first search, an enumeration of every trim path,
// values, counts and staged words written out.  A stand-alone program
// (tests/test_host_only_parts.py builds it with the host compiler under the address and undefined-behaviour sanitizers and runs it): exit
// status 0 and "host-only checks ok", or 1 and a line that names the first case that failed.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "choice_host.hpp"
#include "launch_plan.hpp"
#include "mpa_reach.hpp"
#include "reference_tree.hpp"

namespace {

[[noreturn]] void failed(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fputs("FAILED ", stdout);
    vprintf(fmt, ap);
    putchar('\n');
    va_end(ap);
    exit(1);
}

NodeRec node(uint32_t parent, int k) {
    NodeRec r{};
    r.parent = parent;
    r.packed = 1u | ((uint32_t)k << 10);
    return r;
}

// ---- the reference's tree out of a raw arena

struct Arena {
    int Hp;
    int32_t status;
    std::vector<NodeRec> rec;
    std::vector<double> key;
    std::vector<uint8_t> vs;
    std::vector<uint32_t> first_child, n_child;
};

// Children are consecutive and come after their parent; every node below the horizon may have 0 to 3 of them, collision-free or not (the
// kernel's arena holds nodes the reference never creates).  Keys are a permutation: pairwise distinct, a child's as often below as above its
// parent's.
Arena draw_arena(std::mt19937& rng, int tree) {
    Arena A;
    A.Hp = 1 + tree % 3;
    A.status = rng() % 3u ? PDMPC_OK : PDMPC_EXHAUSTED;
    const size_t max_nodes = 40;
    A.rec.push_back(node(0, 0));
    for (size_t i = 0; i < A.rec.size(); ++i) {
        const int k = NODE_K(A.rec[i].packed);
        size_t c = k < A.Hp ? rng() % 4u : 0u;
        if (i == 0 && c == 0 && (rng() & 3u)) c = 2;  // (most trees grow beyond the root)
        c = std::min(c, max_nodes - A.rec.size());
        A.first_child.push_back(c ? (uint32_t)A.rec.size() : 0u);
        A.n_child.push_back((uint32_t)c);
        for (size_t q = 0; q < c; ++q) A.rec.push_back(node((uint32_t)i + 1u, k + 1));
    }
    const size_t n = A.rec.size();
    std::vector<int> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = (int)i;
    for (size_t i = n; i-- > 1;) std::swap(perm[i], perm[rng() % (i + 1)]);
    for (size_t i = 0; i < n; ++i) A.key.push_back(0.5 * (perm[i] + 1));
    for (size_t i = 0; i < n; ++i) A.vs.push_back(rng() % 5u ? 1 : (uint8_t)(rng() & 2u));  // 1: collision-free; 0 and 2 are not
    return A;
}

struct Expected {
    std::vector<uint32_t> pops, ref_nodes, ref_id;
    bool goal = false, below_parent = false;
};

// GraphSearch.m as it stands: the open set starts with the root; the smallest key is popped (linear scan) and recorded; a node that
// collides is discarded; a collision-free node at the horizon ends a search that found a plan; else the node's children are opened and
// take the next ids in creation order.
Expected best_first(const Arena& A) {
    Expected E;
    E.ref_id.assign(A.rec.size(), 0);
    E.ref_nodes.push_back(0);
    E.ref_id[0] = 1;
    std::vector<uint32_t> open(1, 0u);
    while (!open.empty()) {
        size_t at = 0;
        for (size_t q = 1; q < open.size(); ++q)
            if (A.key[open[q]] < A.key[open[at]]) at = q;
        const uint32_t x = open[at];
        open.erase(open.begin() + (long)at);
        E.pops.push_back(x);
        if (x != 0 && A.key[x] < A.key[A.rec[x].parent - 1]) E.below_parent = true;
        if (A.vs[x] != 1) continue;
        if (NODE_K(A.rec[x].packed) == A.Hp && A.status == PDMPC_OK) {
            E.goal = true;
            break;
        }
        for (uint32_t c = 0; c < A.n_child[x]; ++c) {
            open.push_back(A.first_child[x] + c);
            E.ref_nodes.push_back(A.first_child[x] + c);
            E.ref_id[A.first_child[x] + c] = (uint32_t)E.ref_nodes.size();
        }
    }
    return E;
}

int reconstruct(const Arena& A, const std::vector<uint32_t>* replayed, RefTree& T, std::string& err) {
    return reconstruct_reference_tree(A.rec.data(), (uint32_t)A.rec.size(), A.key.data(), A.vs.data(), A.Hp, A.status, replayed, T, err);
}

void check_reference_trees() {
    std::mt19937 rng(20261019u);
    int goals = 0, emptied = 0, below_parent = 0, invalid_inner = 0, statuses[2] = {0, 0};
    for (int tree = 0; tree < 300; ++tree) {
        const Arena A = draw_arena(rng, tree);
        if (std::set<double>(A.key.begin(), A.key.end()).size() != A.key.size()) failed("tree %d: the generator drew equal keys", tree);
        const Expected E = best_first(A);
        RefTree T;
        std::string err;
        if (const int rc = reconstruct(A, nullptr, T, err)) failed("tree %d: refused (%d): %s", tree, rc, err.c_str());
        if (T.pops != E.pops) failed("tree %d (Hp %d, %zu nodes): pops differ from the best-first search's", tree, A.Hp, A.rec.size());
        if (T.ref_nodes != E.ref_nodes) failed("tree %d (Hp %d, %zu nodes): ref_nodes differ from the best-first search's", tree, A.Hp, A.rec.size());
        if (T.ref_id != E.ref_id) failed("tree %d (Hp %d, %zu nodes): ref_id differs from the best-first search's", tree, A.Hp, A.rec.size());
        // the replayed path: the order comes from outside, the tree is the same
        RefTree R;
        if (const int rc = reconstruct(A, &E.pops, R, err)) failed("tree %d replayed: refused (%d): %s", tree, rc, err.c_str());
        if (R.pops != E.pops || R.ref_nodes != E.ref_nodes || R.ref_id != E.ref_id) failed("tree %d replayed: the tree differs from the best-first search's", tree);
        goals += E.goal;
        emptied += !E.goal;
        below_parent += E.below_parent;
        statuses[A.status == PDMPC_OK] += 1;
        for (size_t i = 0; i < A.rec.size(); ++i) invalid_inner += A.vs[i] != 1 && A.n_child[i] > 0;
    }
    printf("reference trees: 300, %d ended on a goal, %d ran the open set empty, %d popped a child with a smaller key than its parent, %d invalid inner nodes\n", goals, emptied, below_parent,
           invalid_inner);
    if (goals < 100 || emptied < 100 || below_parent < 50 || invalid_inner < 1 || !statuses[0] || !statuses[1]) failed("the tree generator misses the mix of cases it owes");

    // malformed arenas are refused before anything is indexed with them: root, a child, and a third node
    struct Bad {
        const char* what;
        int Hp;
        NodeRec third;
        int n_replayed;  // >= 0: a replayed search whose last pop is node 3 of 3
        const char* names;
    };
    const Bad bad[] = {{"parent 0 on a non-root node", 2, node(0, 1), -1, "node 2"},
                       {"parent above the node's own index", 2, node(3, 1), -1, "node 2"},
                       {"parent far outside the arena", 2, node(0x7fffffffu, 1), -1, "node 2"},
                       {"depth jump of 2", 3, node(1, 2), -1, "node 2"},
                       {"depth Hp + 1", 1, node(2, 2), -1, "node 2"},
                       {"replayed pop == raw_n", 2, node(1, 1), 2, "node 3"}};
    for (const Bad& b : bad) {
        Arena A{b.Hp, PDMPC_OK, {node(0, 0), node(1, 1), b.third}, {1.0, 2.0, 3.0}, {1, 1, 1}, {}, {}};
        std::vector<uint32_t> replayed;
        for (int q = 0; q < b.n_replayed; ++q) replayed.push_back(q + 1 < b.n_replayed ? (uint32_t)q : 3u);
        RefTree T;
        std::string err;
        const int rc = reconstruct(A, b.n_replayed >= 0 ? &replayed : nullptr, T, err);
        if (rc != PDMPC_ERR_INVALID) failed("malformed arena (%s): returned %d, not PDMPC_ERR_INVALID", b.what, rc);
        if (err.find(b.names) == std::string::npos) failed("malformed arena (%s): the message '%s' does not name %s", b.what, err.c_str(), b.names);
    }
    {
        RefTree T;
        std::string err;
        if (reconstruct_reference_tree(nullptr, 0, nullptr, nullptr, 2, PDMPC_OK, nullptr, T, err) != PDMPC_ERR_INVALID) failed("an empty arena is not refused");
    }
}

// ---- the automaton's reach

struct Automaton {
    int n, Hp;
    std::vector<uint8_t> transition;
    std::vector<int32_t> index;
    std::vector<pdmpc_maneuver> man;
    pdmpc_mpa mpa() const { return {n, Hp, transition.data(), index.data(), (int32_t)man.size(), man.data()}; }
    int maneuver(int k, int i, int j) const {  // of step k (1-based), or -1
        const int t = index[(size_t)i * n + j];
        return transition[((size_t)(k - 1) * n + i) * n + j] && t >= 0 && t < (int)man.size() ? t : -1;
    }
};

// kind 0: every step has one random mask; 1: trim 0 has no successor at the last step; 2: the last step has a mask of its own
Automaton draw_automaton(std::mt19937& rng, int n, int Hp, int kind) {
    std::uniform_real_distribution<double> len(-1.5, 1.5), turn(-0.9, 0.9);
    Automaton A{n, Hp, {}, {}, {}};
    const int T = 2 + (int)(rng() % 3u);
    const int cols[3] = {2, 3, PDMPC_VMAX};
    for (int t = 0; t < T; ++t) {
        pdmpc_maneuver m{};
        m.dx = 1.0 + len(rng);
        m.dy = len(rng);
        m.dyaw = turn(rng);
        m.n_cols = cols[(t + n + kind) % 3];
        double(*area[3])[PDMPC_VMAX] = {m.area, m.area_without_offset, m.area_large_offset};
        for (int a = 0; a < 3; ++a)
            for (int v = 0; v < PDMPC_VMAX; ++v) {
                area[a][0][v] = v < m.n_cols ? 2.0 * len(rng) : 1e9;  // (a column past n_cols must not be read)
                area[a][1][v] = v < m.n_cols ? len(rng) : -1e9;
            }
        A.man.push_back(m);
    }
    A.index.assign((size_t)n * n, -1);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (i == j || (rng() & 1u)) A.index[(size_t)i * n + j] = (int32_t)(rng() % (unsigned)T);
    std::vector<uint8_t> mask((size_t)n * n), last((size_t)n * n);
    for (uint8_t& b : mask) b = (rng() % 4u) != 0;
    for (uint8_t& b : last) b = (rng() & 1u) != 0;
    for (int k = 0; k < Hp; ++k) A.transition.insert(A.transition.end(), mask.begin(), mask.end());
    uint8_t* final_mask = A.transition.data() + (size_t)(Hp - 1) * n * n;
    if (kind == 1) std::memset(final_mask, 0, (size_t)n);  // row of trim 0
    if (kind == 2) std::memcpy(final_mask, last.data(), last.size());
    return A;
}

// every point of every area (three variants, used columns) of the last maneuver of every allowed trim path of K steps from trim i at
// `pose` = (x, y, yaw), k its next step: into box = (x_lo, x_hi, y_lo, y_hi)
void enumerate_paths(const Automaton& A, int K, int k, int i, const double pose[3], double box[4]) {
    for (int j = 0; j < A.n; ++j) {
        const int t = A.maneuver(k, i, j);
        if (t < 0) continue;
        const pdmpc_maneuver& m = A.man[(size_t)t];
        const double c = std::cos(pose[2]), s = std::sin(pose[2]);
        if (k < K) {
            const double next[3] = {pose[0] + c * m.dx - s * m.dy, pose[1] + s * m.dx + c * m.dy, pose[2] + m.dyaw};
            enumerate_paths(A, K, k + 1, j, next, box);
            continue;
        }
        const double(*area[3])[PDMPC_VMAX] = {m.area, m.area_without_offset, m.area_large_offset};
        for (int a = 0; a < 3; ++a)
            for (int v = 0; v < m.n_cols; ++v) {
                const double px = pose[0] + c * area[a][0][v] - s * area[a][1][v], py = pose[1] + s * area[a][0][v] + c * area[a][1][v];
                box[0] = box[0] != box[0] ? px : std::min(box[0], px);
                box[1] = box[1] != box[1] ? px : std::max(box[1], px);
                box[2] = box[2] != box[2] ? py : std::min(box[2], py);
                box[3] = box[3] != box[3] ? py : std::max(box[3], py);
            }
    }
}

const double kRectTolerance = 1e-12;  // absolute; the largest difference this program sees is printed

void check_reach_rects() {
    std::mt19937 rng(950u);
    double worst = 0.0;
    int nan_rects = 0, automata = 0;
    for (int n = 2; n <= 3; ++n)
        for (int Hp = 1; Hp <= 3; ++Hp)
            for (int kind = 0; kind < 3; ++kind, ++automata) {
                const Automaton A = draw_automaton(rng, n, Hp, kind);
                const pdmpc_mpa mpa = A.mpa();
                double dmax = -1.0, amax = -1.0, want_d = 0.0, want_a = 0.0;
                mpa_reach(&mpa, dmax, amax);
                for (const pdmpc_maneuver& m : A.man) {
                    want_d = std::max(want_d, hypot(m.dx, m.dy));
                    for (int v = 0; v < m.n_cols; ++v)
                        want_a = std::max({want_a, hypot(m.area[0][v], m.area[1][v]), hypot(m.area_without_offset[0][v], m.area_without_offset[1][v]),
                                           hypot(m.area_large_offset[0][v], m.area_large_offset[1][v])});
                }
                if (dmax != want_d || amax != want_a) failed("automaton %d (n %d, Hp %d, kind %d): mpa_reach gives (%.17g, %.17g), the maneuvers (%.17g, %.17g)", automata, n, Hp, kind, dmax, amax, want_d, want_a);
                std::vector<double> rects((size_t)n * Hp * 4, 12345.0);
                mpa_reach_rects(&mpa, Hp, rects.data());
                for (int r = 0; r < n; ++r)
                    for (int K = 1; K <= Hp; ++K) {
                        const double qnan = std::numeric_limits<double>::quiet_NaN(), origin[3] = {0.0, 0.0, 0.0};
                        double want[4] = {qnan, qnan, qnan, qnan};
                        enumerate_paths(A, K, 1, r, origin, want);
                        const double* got = &rects[((size_t)r * Hp + (K - 1)) * 4];
                        for (int q = 0; q < 4; ++q) {
                            if ((want[q] != want[q]) != (got[q] != got[q]) || std::fabs(got[q] - want[q]) > kRectTolerance)
                                failed("automaton %d (n %d, Hp %d, kind %d) trim %d step %d: rectangle[%d] is %.17g, every path gives %.17g", automata, n, Hp, kind, r, K, q, got[q], want[q]);
                            if (want[q] == want[q]) worst = std::max(worst, std::fabs(got[q] - want[q]));
                        }
                        nan_rects += want[0] != want[0];
                    }
            }
    printf("reach rectangles: %d automata, largest |hull composition - path enumeration| %.3g, %d rectangles without a path\n", automata, worst, nan_rects);
    if (nan_rects < 1) failed("the automata hold no trim without a path");
}

void expect_lists(const char* what, int rc, const std::vector<int32_t>& offset, const std::vector<int32_t>& list, const std::vector<int32_t>& want_offset, const std::vector<int32_t>& want_list) {
    if (rc != PDMPC_OK) failed("%s: returned %d", what, rc);
    if (offset != want_offset) failed("%s: list offsets differ", what);
    if (!std::equal(want_list.begin(), want_list.end(), list.begin())) failed("%s: the lists differ", what);
}

void check_reach_lists() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::string err;
    {
        // the disc rule around (0, 0) with Dmax 1, Amax 2: squares of half width 2 and 3 (and a margin of 1e-6)
        const double x[] = {0, 1, 5, 6, 6, nan, 0.5, 0.6, /* step 2 */ 2.5, 2.9, 3.5, 4, -10, 10};
        const double y[] = {0, 1, 5, 5, -6, nan, 0.5, 0.5, /* step 2 */ 0, 0, 0, 0, -10, 10};
        const int32_t first[] = {0, 8}, count[] = {8, 6};
        std::vector<int32_t> offset(3, -1), list(12, -1);
        // step 1: inside, straddling, outside, outside, NaN, NaN, inside; step 2: inside (outside step 1's square), straddling, outside, box overlaps, crosses
        const int rc = reach_lists(2, 1.0, 2.0, 0.0, 0.0, x, y, first, count, offset.data(), list.data(), err);
        expect_lists("reach_lists", rc, offset, list, {0, 3, 7}, {0, 1, 6, 0, 1, 3, 4});
        const int32_t none[] = {0, 1};
        offset.assign(3, -1);
        expect_lists("reach_lists without segments", reach_lists(2, 1.0, 2.0, 0.0, 0.0, nullptr, nullptr, first, none, offset.data(), nullptr, err), offset, list, {0, 0, 0}, {});
        const int32_t negative[] = {0, -1};
        if (reach_lists(2, 1.0, 2.0, 0.0, 0.0, x, y, first, negative, offset.data(), list.data(), err) != PDMPC_ERR_INVALID || err != "pdmpc_reach_lists_host: bad step ranges")
            failed("reach_lists: a negative step count is not refused");
    }
    {
        // the oriented rule: root at (10, 20) heading along +y in trim 2 of 2, whose rectangles are (0, 2) x (-1, 1) and (1, 4) x (-2, 2);
        // a point (u, v) of the root's frame lies at (10 - v, 20 + u)
        const double rects[] = {nan, nan, nan, nan, nan, nan, nan, nan, 0, 2, -1, 1, 1, 4, -2, 2};
        const double u[] = {0.5, 1.5, 3, 3, -1, -1, /* step 2 */ 0.5, 0.9, 2, 3, 5, 6};
        const double v[] = {0, 0.5, 0, 5, 0, -3, /* step 2 */ 0, 1, 1, -1, -1, -1};
        double x[12], y[12];
        for (int i = 0; i < 12; ++i) {
            x[i] = 10.0 - v[i];
            y[i] = 20.0 + u[i];
        }
        const int32_t first[] = {0, 6}, count[] = {6, 6};
        std::vector<int32_t> offset(3, -1), list(10, -1);
        // step 1: inside, straddling, outside, box overlaps, outside; step 2: outside (inside step 1's rectangle), straddling, inside, straddling, outside
        const int rc = reach_lists_oriented(2, rects, 2, 10.0, 20.0, 1.5707963267948966, x, y, first, count, offset.data(), list.data(), err);
        expect_lists("reach_lists_oriented", rc, offset, list, {0, 3, 6}, {0, 1, 3, 1, 2, 3});
        const int32_t none[] = {1, 0};
        offset.assign(3, -1);
        expect_lists("reach_lists_oriented without segments", reach_lists_oriented(2, rects, 2, 10.0, 20.0, 1.5707963267948966, nullptr, nullptr, first, none, offset.data(), nullptr, err), offset,
                     list, {0, 0, 0}, {});
        const int32_t negative[] = {-1, 6};
        if (reach_lists_oriented(2, rects, 2, 10.0, 20.0, 0.0, x, y, negative, count, offset.data(), list.data(), err) != PDMPC_ERR_INVALID || err != "pdmpc_reach_lists_oriented_host: bad step ranges")
            failed("reach_lists_oriented: a negative step start is not refused");
    }
}

// ---- the checked choice

void expect_refusal(const char* want, int32_t n, const pdmpc_choice* ch) {
    std::string err;
    const int rc = check_choice(n, ch, err);
    if (rc != PDMPC_ERR_INVALID || err != want) failed("check_choice: returned %d '%s', not PDMPC_ERR_INVALID '%s'", rc, err.c_str(), want);
}

// the words a choice is staged in for the kernels, against arrays written out by hand: cell_offset | cell slots | graph_offset | pick_graph |
// pick_offset | pick slots
void expect_words(const char* what, const pdmpc_choice& ch, const std::vector<int32_t>& perm, const std::vector<int32_t>& want) {
    const ChoiceLists W(ch);
    if (W.words != want.size()) failed("ChoiceLists (%s): %zu words, not %zu", what, W.words, want.size());
    std::vector<int32_t> w(W.words, -99);  // (exactly as many: the sanitizer sees a word written beyond them)
    stage_choice_lists(ch, W, w.data(), [&perm](const int32_t* slot, int count, int32_t* to) {
        for (int q = 0; q < count; ++q) to[q] = perm.empty() ? slot[q] : perm[(size_t)slot[q]];
    });
    for (size_t q = 0; q < want.size(); ++q)
        if (w[q] != want[q]) failed("stage_choice_lists (%s): word %zu is %d, not %d", what, q, w[q], want[q]);
}

void check_staged_lists(const pdmpc_choice& good) {
    const ChoiceLists W(good);
    if (W.cell_offset != 0 || W.cell_slot != 6 || W.graph_offset != 13 || W.pick_graph != 16 || W.pick_offset != 18 || W.pick_slot != 21 || W.words != 25)
        failed("ChoiceLists: (%zu, %zu, %zu, %zu, %zu, %zu, %zu)", W.cell_offset, W.cell_slot, W.graph_offset, W.pick_graph, W.pick_offset, W.pick_slot, W.words);
    expect_words("identity", good, {}, {0, 2, 4, 5, 6, 7, /**/ 0, 1, 2, 0, 4, 1, 3, /**/ 0, 3, 5, /**/ 0, -1, /**/ 0, 3, 4, /**/ 0, 2, 4, 3});
    // slot s is found at perm[s]: offsets and pick_graph are no slots and stay
    expect_words("permuted", good, {3, 0, 4, 1, 2}, {0, 2, 4, 5, 6, 7, /**/ 3, 0, 4, 3, 2, 0, 1, /**/ 0, 3, 5, /**/ 0, -1, /**/ 0, 3, 4, /**/ 3, 4, 2, 1});
    // no cell, no graph, no pick: the three offset lists are their first entry, 0, and no list is read
    const pdmpc_choice none{0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    expect_words("empty", none, {}, {0, 0, 0});
}

// a block as the device leaves it, built by hand, into the caller's arrays; a counter of records that are no planning results refuses it
void check_delivery(const pdmpc_choice& good, const ChoiceLayout& L) {
    const char* refusal = "a result record carries an error status: not a planning result";
    std::vector<unsigned char> blk(L.bytes, 0);
    const int32_t want_chosen[2] = {2, 0};
    const double want_cost[5] = {3.0, std::numeric_limits<double>::infinity(), 0.12345679, 2.0, 2.0};
    std::vector<pdmpc_vehicle_out> want_picks(2);
    for (size_t i = 0; i < 2; ++i) std::memset(&want_picks[i], (int)(0x5a + i), sizeof(pdmpc_vehicle_out));
    std::memcpy(blk.data() + 16, want_chosen, sizeof want_chosen);
    std::memcpy(blk.data() + 24, want_cost, sizeof want_cost);
    std::memcpy(blk.data() + 64, want_picks.data(), 2 * sizeof(pdmpc_vehicle_out));
    for (int without = 0; without < 3; ++without) {  // 0: every array; 1: chosen null; 2: cell_cost null
        int32_t chosen[2] = {-1, -1};
        double cell_cost[5] = {-1, -1, -1, -1, -1};
        std::vector<pdmpc_vehicle_out> picks(2);
        std::string err = "unset";
        if (!deliver_choice(good, L, blk.data(), without == 1 ? nullptr : chosen, without == 2 ? nullptr : cell_cost, picks.data(), err) || err != "unset")
            failed("deliver_choice (%d): a block of planning results is refused: %s", without, err.c_str());
        const int32_t untouched_chosen[2] = {-1, -1};
        const double untouched_cost[5] = {-1, -1, -1, -1, -1};
        if (std::memcmp(chosen, without == 1 ? untouched_chosen : want_chosen, sizeof chosen) != 0) failed("deliver_choice (%d): chosen differs", without);
        if (std::memcmp(cell_cost, without == 2 ? untouched_cost : want_cost, sizeof cell_cost) != 0) failed("deliver_choice (%d): cell_cost differs", without);
        if (std::memcmp(picks.data(), want_picks.data(), 2 * sizeof(pdmpc_vehicle_out)) != 0) failed("deliver_choice (%d): the picked records differ", without);
    }
    for (int counter : {(int)PDMPC_CHOICE_OVERFLOW, (int)PDMPC_CHOICE_TIMED_OUT, (int)PDMPC_CHOICE_OTHER}) {
        std::vector<unsigned char> bad = blk;
        const int32_t one = 1;
        std::memcpy(bad.data() + (size_t)counter * sizeof one, &one, sizeof one);
        int32_t chosen[2] = {-1, -1};
        double cell_cost[5] = {-1, -1, -1, -1, -1};
        std::vector<pdmpc_vehicle_out> picks(2);
        std::string err;
        if (deliver_choice(good, L, bad.data(), chosen, cell_cost, picks.data(), err)) failed("deliver_choice: a block with counter %d set is delivered", counter);
        if (err != refusal) failed("deliver_choice: counter %d is refused with '%s'", counter, err.c_str());
        if (chosen[0] != -1 || cell_cost[0] != -1) failed("deliver_choice: a refused block was delivered in part (counter %d)", counter);
    }
}

void check_choices() {
    // five records; graph 0 chooses among cells 0 .. 2, graph 1 among cells 3 and 4; pick 0 follows graph 0, pick 1 its own slot
    const int32_t status[] = {PDMPC_OK, PDMPC_OK, PDMPC_EXHAUSTED, PDMPC_OK, PDMPC_OK};
    const double cost[] = {1.0, 2.0, 9.0, 2.0, 0.123456789012};
    const int32_t cell_offset[] = {0, 2, 4, 5, 6, 7}, cell_slot[] = {0, 1, 2, 0, 4, 1, 3}, graph_offset[] = {0, 3, 5};
    const int32_t pick_graph[] = {0, -1}, pick_offset[] = {0, 3, 4}, pick_slot[] = {0, 2, 4, 3};
    const pdmpc_choice good{5, 2, 2, 0, cell_offset, cell_slot, graph_offset, pick_graph, pick_offset, pick_slot};
    std::string err;
    if (const int rc = check_choice(5, &good, err)) failed("check_choice: the well-formed choice is refused (%d): %s", rc, err.c_str());
    int32_t chosen[2] = {-1, -1};
    double cell_cost[5] = {-1, -1, -1, -1, -1};
    choose_host(status, cost, &good, chosen, cell_cost);
    // 1 + 2; an exhausted slot: +inf; round(., 8); a tie of 2 and 2: the first
    const double want_cost[5] = {3.0, std::numeric_limits<double>::infinity(), 0.12345679, 2.0, 2.0};
    for (int c = 0; c < 5; ++c)
        if (cell_cost[c] != want_cost[c]) failed("choose_host: cell %d costs %.17g, not %.17g", c, cell_cost[c], want_cost[c]);
    if (chosen[0] != 2 || chosen[1] != 0) failed("choose_host: chose (%d, %d), not (2, 0)", chosen[0], chosen[1]);
    choose_host(status, cost, &good, nullptr, nullptr);  // (both outputs are optional)
    const ChoiceLayout L(good);
    if (L.chosen != 16 || L.cell_cost != 24 || L.picks != 64 || L.bytes != 64 + 2 * sizeof(pdmpc_vehicle_out)) failed("ChoiceLayout: (%zu, %zu, %zu, %zu)", L.chosen, L.cell_cost, L.picks, L.bytes);

    check_staged_lists(good);
    check_delivery(good, L);

    // every refusal once, in the order of the checks
    expect_refusal("pdmpc_choice: bad argument", 5, nullptr);
    pdmpc_choice ch = good;
    ch.n_picks = -1;
    expect_refusal("pdmpc_choice: bad argument", 5, &ch);
    ch = good;
    ch.pick_offset = nullptr;
    expect_refusal("pdmpc_choice: null list", 5, &ch);
    const int32_t cells_decrease[] = {0, 2, 1, 5, 6, 7}, graphs_decrease[] = {0, 3, 2}, graphs_beyond[] = {0, 3, 6}, picks_negative[] = {-1, 2, 3};
    ch = good;
    ch.cell_offset = cells_decrease;
    expect_refusal("pdmpc_choice: cell offsets are negative or decrease", 5, &ch);
    expect_refusal("pdmpc_choice: a cell lists a slot outside the batch", 4, &good);
    ch = good;
    ch.graph_offset = graphs_decrease;
    expect_refusal("pdmpc_choice: graph offsets are negative or decrease", 5, &ch);
    ch.graph_offset = graphs_beyond;
    expect_refusal("pdmpc_choice: a graph's candidates lie outside the cells", 5, &ch);
    ch = good;
    ch.pick_offset = picks_negative;
    expect_refusal("pdmpc_choice: pick offsets are negative or decrease", 5, &ch);
    const int32_t no_such_graph[] = {0, 2}, two_own_slots[] = {0, 3, 5}, slots_beyond[] = {0, 2, 5, 3}, own_slots[] = {0, 2, 4, 3, 3};
    ch = good;
    ch.pick_graph = no_such_graph;
    expect_refusal("pdmpc_choice: pick_graph outside [-1, n_graphs)", 5, &ch);
    ch = good;
    ch.pick_offset = two_own_slots;
    ch.pick_slot = own_slots;
    expect_refusal("pdmpc_choice: a pick lists another number of slots than its graph has candidates", 5, &ch);
    ch = good;
    ch.pick_slot = slots_beyond;
    expect_refusal("pdmpc_choice: a pick lists a slot outside the batch", 5, &ch);
}

// ---- the scratch of a sampled bank (sampled_need) and the seeds on their way to a pack (PendingSeeds)

// A bank of 7 slots at (budget, members), planned for a small automaton: where the tree lives is the planner's, the counts are written out.
// By sampled_budget.h a tree has (budget + PDMPC_HP_MAX + 2 + 7) & ~7 rows of PDMPC_SB_ROW = 18 words: 272 rows at 250 and at 251
// (275 & ~7, 276 & ~7), 16 408 rows = 295 344 words at 16 384 (16 409 & ~7).  In HBM every slot and member has a tree of its own:
// 7 * 295 344 = 2 067 408 words, 14 * 295 344 = 4 134 816, 112 * 295 344 = 33 078 528.  An ensemble of E keeps 7 * E member records,
// entries and tree sizes and 7 tickets and chosen members; one member keeps none.
void expect_need(int budget, int members, bool want_in_lds, size_t want_tree, size_t want_per_member, size_t want_per_slot) {
    LaunchDims d{PDMPC_CHECK_INTERX, 5, 12, 0, 40, 0, 0, 256, 1, 32768u, true, 400, 60, 120};
    mpa_table_sizes(d);
    LaunchPlan plan;
    SampledExtra extra;
    std::string err;
    if (const int rc = plan_sampled(Tuning{}, d, budget, members, 7, false, plan, extra, err)) failed("sampled need (%d, %d): plan_sampled returned %d: %s", budget, members, rc, err.c_str());
    if ((extra.tree_in_lds != 0) != want_in_lds) failed("sampled need (%d, %d): tree_in_lds is %d", budget, members, extra.tree_in_lds);
    const SampledNeed need = sampled_need(SampledBank{true, budget, members}, 7, extra);
    if (need.tree != want_tree || need.per_member != want_per_member || need.per_slot != want_per_slot)
        failed("sampled need (%d, %d): tree %zu per member %zu per slot %zu, expected %zu %zu %zu", budget, members, need.tree, need.per_member, need.per_slot, want_tree, want_per_member, want_per_slot);
}

void check_sampled_need() {
    if (!SampledBank{true, 250, 1}.reference() || SampledBank{true, 251, 1}.reference() || SampledBank{true, 250, 2}.reference()) failed("SampledBank::reference");
    expect_need(250, 1, true, 0, 0, 0);  // (the default: pdmpc_sampled_kernel, nothing needed)
    expect_need(251, 1, true, 0, 0, 0);
    expect_need(16384, 1, false, 2067408, 0, 0);
    expect_need(250, 2, true, 0, 14, 7);
    expect_need(251, 2, true, 0, 14, 7);
    expect_need(251, 16, true, 0, 112, 7);
    expect_need(16384, 2, false, 4134816, 14, 7);
    expect_need(16384, 16, false, 33078528, 112, 7);
    // an empty bank needs nothing, wherever its trees would live
    SampledExtra hbm;
    hbm.node_cap = 16408;
    hbm.tree_in_lds = 0;
    const SampledNeed none = sampled_need(SampledBank{true, 16384, 16}, 0, hbm);
    if (none.tree != 0 || none.per_member != 0 || none.per_slot != 0) failed("sampled need of an empty bank");
}

void check_pending_seeds() {
    PendingSeeds P;
    std::vector<uint32_t> got{9u};
    if (P.take(got) || !got.empty()) failed("pending seeds: a take with nothing set is a sampled one");
    const uint32_t first[] = {1u, 2u, 3u}, second[] = {40u, 50u};
    P.assign(first, 3);
    if (!P.take(got) || got != std::vector<uint32_t>{1u, 2u, 3u}) failed("pending seeds: set then take does not yield the seeds");
    if (P.set || !P.seeds.empty()) failed("pending seeds: a take leaves something behind");
    if (P.take(got) || !got.empty()) failed("pending seeds: a second take is a sampled one");
    P.assign(first, 3);
    P.assign(second, 2);
    if (!P.take(got) || got != std::vector<uint32_t>{40u, 50u}) failed("pending seeds: set twice does not keep the last");
    P.assign(first, 0);  // (no vehicles, but set: the pack is a sampled one)
    if (!P.take(got) || !got.empty() || P.take(got)) failed("pending seeds: an empty set of seeds");
}

}  // namespace

int main() {
    check_reference_trees();
    check_reach_rects();
    check_reach_lists();
    check_choices();
    check_sampled_need();
    check_pending_seeds();
    puts("host-only checks ok");
    return 0;
}
