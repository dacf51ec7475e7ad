"""Where a group's records are after its launches (csrc/group_route.hpp behind pdmpc_group_route_host), without a
device: the route in C++ against a Python restatement built on pdmpc.distributed's partition twins.

A rank holds the records of its whole components in the order it planned them: a topological order of the coupling DAG — level order
(the caller's order within a level), or with expected work per vehicle priority order (the largest work among a vehicle and its
descendants, descending; ties by level, then by the caller's index).  The component planned by levels is held by rank 0 behind its
own records, in level order."""
import numpy as np
import pytest

from pdmpc import backend, distributed

from test_group import random_dag

MODES = [backend.SHARD_COMPONENTS, backend.SHARD_AUTO, backend.SHARD_LEVELS]


def levels_of(preds):
    """computation level per slot (1-based, longest path) of a DAG whose predecessors sit in lower slots"""
    lvl = []
    for ps in preds:
        lvl.append(1 + max((lvl[p] for p in ps), default=0))
    return lvl


def inherited_priority(preds, weights):
    """per slot the largest weight among the slot and its descendants (slots in a topological order)"""
    prio = [float(w) if w > 0 else 0.0 for w in weights]
    for s in reversed(range(len(preds))):
        for p in preds[s]:
            prio[p] = max(prio[p], prio[s])
    return prio


def route_restated(preds, world, mode, weights):
    """-> (rank, position) per slot, from the Python partition twins and the order stated in the module's docstring"""
    n = len(preds)
    if mode == backend.SHARD_LEVELS:
        parts, shared = [[] for _ in range(world)], list(range(n))
    elif mode == backend.SHARD_AUTO:
        parts, shared = distributed.hybrid_partition(preds, world, weights)
    else:
        parts, shared = distributed.partition_components(preds, world, weights), []
    lvl = levels_of(preds)
    prio = inherited_priority(preds, weights) if weights is not None else [0.0] * n
    rank, pos = [-1] * n, [-1] * n
    held = [0] * world
    for r, slots in enumerate(parts):
        for i, s in enumerate(sorted(slots, key=lambda v: (-prio[v], lvl[v], v))):
            rank[s], pos[s] = r, i
        held[r] = len(slots)
    for i, s in enumerate(sorted(shared, key=lambda v: (lvl[v], v))):
        rank[s], pos[s] = 0, held[0] + i
    return rank, pos


def assert_route(preds, world, mode, weights, ctx):
    rank, pos = backend.group_route(preds, world, mode, weights)
    want_rank, want_pos = route_restated(preds, world, mode, weights)
    assert rank.tolist() == want_rank, ctx
    assert pos.tolist() == want_pos, ctx
    # every record has one holder and one place: (rank, position) is a bijection onto 0 .. held[rank] - 1
    for r in range(world):
        assert sorted(pos[rank == r].tolist()) == list(range(int((rank == r).sum()))), ctx
    return rank, pos


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("world", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", MODES)
def test_route_matches_the_python_restatement(seed, world, mode):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(5, 61))
    preds = random_dag(rng, n, 0.15, int(rng.integers(1, 9)))
    weights = [float(w) for w in rng.integers(1, 2000, n)] if seed % 2 else None
    assert_route(preds, world, mode, weights, (seed, world, mode))


@pytest.mark.parametrize("mode", MODES)
def test_more_ranks_than_components_leave_ranks_empty(mode):
    rng = np.random.default_rng(3)
    preds = random_dag(rng, 14, 0.5, 2)
    n_components = len(set(distributed.weak_components(preds)))
    assert n_components < 8
    rank, _ = assert_route(preds, 8, mode, None, mode)
    assert len(set(rank.tolist())) <= n_components  # ... so some of the eight ranks hold no record


@pytest.mark.parametrize("world", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", MODES)
def test_a_step_that_is_one_component(world, mode):
    n = 17
    preds = [[] if s == 0 else [s - 1] + ([s - 3] if s >= 3 and s % 2 else []) for s in range(n)]  # one chain with chords
    assert len(set(distributed.weak_components(preds))) == 1
    rank, pos = assert_route(preds, world, mode, None, (world, mode))
    if mode == backend.SHARD_COMPONENTS or world == 1:
        assert (rank == 0).all() and pos.tolist() == list(range(n))  # the least loaded rank, ties to the lowest: rank 0 takes it whole
    else:
        # planned by levels over all ranks (2 * world <= 17 and it outweighs the mean load): rank 0 holds it, in level order
        assert (rank == 0).all() and pos.tolist() == list(range(n))


def test_the_empty_step_and_bad_arguments():
    rank, pos = backend.group_route([], 4)
    assert len(rank) == 0 and len(pos) == 0
    with pytest.raises(backend.BackendError):
        backend.group_route([[1], [0]], 2)  # a cycle
    with pytest.raises(backend.BackendError):
        backend.group_route([[]], 2, mode=7)
    with pytest.raises(backend.BackendError):
        backend.group_route([[]], 0)
