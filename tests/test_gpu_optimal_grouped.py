"""The unique prioritizations of several coupling graphs in one device call (pdmpc_unique_priorities_grouped,
csrc/priority_kernel.hip): every block is what the ungrouped device call returns for that graph alone and what the
host twin returns -- at the tile boundaries, with more groups than a wavefront has lanes, with vertices above bit 32 of the placed set --,
what does not fit is refused with every count reported and nothing written, and the handle goes on."""
import numpy as np
import pytest

from pdmpc.backend import CapacityError, Handle, unique_priorities_grouped_call
from pdmpc.config import Config, ScenarioType

from test_optimal_grouped import alone, assert_same_lists
from test_optimal_reference import complete, random_graph

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 4096  # PDMPC_PRIO_TILE: orientations per tile


@pytest.fixture(scope="module")
def h():
    handle = Handle(Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 12))
    yield handle
    handle.close()


def with_edges(rng, n, E, first=0, size=None):
    """a graph of `size` (default n) vertices with exactly E edges among the n vertices from `first` on"""
    size = n + first if size is None else size
    A = np.zeros((size, size), dtype=np.int64)
    pairs = [(r, c) for c in range(n) for r in range(c)]
    for q in rng.choice(len(pairs), size=E, replace=False):
        r, c = pairs[q]
        A[first + r, first + c] = A[first + c, first + r] = 1
    return A


def check(h, graphs, ctx):
    """the grouped device call == the ungrouped device call per graph == the grouped host twin; -> the counts"""
    want = alone(graphs, handle=h)
    counts = [len(m) for _, m in want]
    assert_same_lists(h.unique_priorities_grouped(graphs, counts), want, ctx + ": device, ungrouped")
    assert_same_lists(unique_priorities_grouped_call(graphs, counts), want, ctx + ": host twin")
    return counts


def test_one_group_of_each_reference_graph(h):
    rng = np.random.default_rng(17)
    graphs = [np.zeros((1, 1)), np.zeros((6, 6)), complete(3), complete(5)] + [random_graph(rng, int(rng.integers(2, 12)), 20) for _ in range(10)]
    for i, A in enumerate(graphs):
        check(h, [A], "graph %d alone" % i)
    counts = check(h, graphs, "all of them in one call")
    assert counts[:4] == [1, 1, 6, 120]


def test_tile_boundaries_in_one_call(h):
    rng = np.random.default_rng(19)
    # E = 12: exactly one full tile; E = 0: one tile that holds one mask; E = 13: two tiles; E = 11: half a tile; E = 4
    graphs = [with_edges(rng, 7, E) for E in (12, 0, 13, 11, 4)]
    assert [2 ** int(np.triu(A, 1).sum()) for A in graphs] == [TILE, 1, 2 * TILE, TILE // 2, 16]
    counts = check(h, graphs, "in this order")
    assert check(h, graphs[::-1], "reversed") == counts[::-1]
    # (more than 6 edges on 7 vertices close a cycle: those lists are compacted)
    assert counts[1] == 1 and all(1 < k < 2 ** int(np.triu(A, 1).sum()) for k, A in zip(counts, graphs) if np.triu(A, 1).sum() > 6)


def test_two_identical_graphs_next_to_each_other(h):
    rng = np.random.default_rng(23)
    A = with_edges(rng, 7, 13)
    got = h.unique_priorities_grouped([A, A, complete(3), complete(3)], 10000)
    assert_same_lists(got[:1], got[1:2], "the same graph twice")
    check(h, [A, A, complete(3), complete(3)], "twice")


@pytest.mark.parametrize("n_groups", [65, 130])
def test_many_tiny_groups(h, n_groups):
    """the depth of the group search, and more groups than a wavefront has lanes"""
    rng = np.random.default_rng(n_groups)
    graphs = [random_graph(rng, int(rng.integers(1, 6)), 6) for _ in range(n_groups)]
    assert any(A.shape[0] == 1 for A in graphs) and any(A.sum() > 4 for A in graphs)
    check(h, graphs, "%d groups" % n_groups)


def test_a_64_vertex_graph_between_two_small_groups(h):
    """12 edges among vertices 40-52: the placed set of the order pass above bit 32"""
    rng = np.random.default_rng(29)
    big = with_edges(rng, 13, 12, first=40, size=64)
    assert big.shape == (64, 64) and np.triu(big, 1).sum() == 12 and not big[:40].any() and not big[53:].any()
    counts = check(h, [complete(3), big, complete(4)], "64 vertices")
    assert counts[0] == 6 and counts[2] == 24 and counts[1] > 1
    (prio, _), = h.unique_priorities_grouped([big], counts[1])
    assert np.array_equal(np.sort(prio, axis=0), np.tile(np.arange(1, 65)[:, None], (1, counts[1])))


def test_one_group_over_its_max_out_is_refused_and_the_handle_goes_on(h):
    rng = np.random.default_rng(31)
    graphs = [complete(3), with_edges(rng, 7, 13), complete(4), np.zeros((5, 5))]
    counts = [len(m) for _, m in alone(graphs)]
    masks = np.full(sum(counts) + 8, 0xDEADBEEF, dtype=np.uint32)
    prio = np.full(sum(k * A.shape[0] for k, A in zip(counts, graphs)) + 8, -77, dtype=np.int32)
    caps = list(counts)
    caps[1] -= 1
    with pytest.raises(CapacityError) as e:
        h.unique_priorities_grouped(graphs, caps, masks_out=masks, priorities_out=prio)
    assert e.value.counts == counts and e.value.count == counts[1]
    assert (masks == 0xDEADBEEF).all() and (prio == -77).all()
    path = np.zeros((40, 40), dtype=np.int64)  # 33 edges
    for v in range(33):
        path[v, v + 1] = path[v + 1, v] = 1
    with pytest.raises(CapacityError) as e:
        h.unique_priorities_grouped([complete(3), path, np.zeros((65, 65)), complete(4)], 100, masks_out=masks, priorities_out=prio)
    assert e.value.counts == [6, -1, -1, 24]
    assert (masks == 0xDEADBEEF).all() and (prio == -77).all()
    assert_same_lists(h.unique_priorities_grouped(graphs, counts, masks_out=masks, priorities_out=prio), alone(graphs), "after the refusals")
    assert (masks[sum(counts):] == 0xDEADBEEF).all() and (prio[-8:] == -77).all()


def test_a_small_call_directly_after_a_large_one(h):
    large = [complete(7), complete(6)]  # E = 21: 512 tiles, 5040 masks
    got = h.unique_priorities_grouped(large, 6000)
    assert [len(m) for _, m in got] == [5040, 720]
    check(h, [complete(3), np.zeros((2, 2))], "after a large call")
    assert_same_lists(h.unique_priorities_grouped(large, 6000), got, "and the large one again")


def test_the_star_with_32_leaves_counts_2_to_the_32(h):
    """Every orientation of a tree is acyclic: int64 counting across 2^20 tiles (two sweeps per mask: well under a second)."""
    star = np.zeros((33, 33), dtype=np.int64)
    star[0, 1:] = star[1:, 0] = 1
    with pytest.raises(CapacityError) as e:
        h.unique_priorities_grouped([complete(3), star, complete(4)], 0)
    assert e.value.counts == [6, 1 << 32, 24]
