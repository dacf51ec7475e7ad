"""Closed-form counts of unique prioritizations (acyclic orientations, |chi_G(-1)|) for graphs too large for deletion-contraction:
the GPU tests of the priority enumeration at 29 to 32 edges take their expected counts from here.

A leaf edge is a bridge: its two orientations are independent of the rest, so stripping it halves the count.  What is left after
stripping every leaf is a disjoint union of cores; a cycle C_n has 2^n - 2 acyclic orientations, K_n has n!, a lone vertex one."""
import math

import numpy as np
import pytest

from test_optimal_reference import chromatic_at_minus_one, complete


def disjoint_union(*graphs):
    n = sum(A.shape[0] for A in graphs)
    U = np.zeros((n, n), dtype=np.int64)
    at = 0
    for A in graphs:
        m = A.shape[0]
        U[at : at + m, at : at + m] = A
        at += m
    return U


def cycle(n):
    A = np.zeros((n, n), dtype=np.int64)
    for v in range(n):
        A[v, (v + 1) % n] = A[(v + 1) % n, v] = 1
    return A


def tree_path(k):
    """A path of k edges."""
    A = np.zeros((k + 1, k + 1), dtype=np.int64)
    for v in range(k):
        A[v, v + 1] = A[v + 1, v] = 1
    return A


def star(k):
    """A star of k edges, centre 0."""
    A = np.zeros((k + 1, k + 1), dtype=np.int64)
    A[0, 1:] = A[1:, 0] = 1
    return A


def pendant(A, k, at=0):
    """A with k new vertices, each joined to vertex `at` by one edge."""
    n = A.shape[0]
    B = np.zeros((n + k, n + k), dtype=np.int64)
    B[:n, :n] = A
    B[at, n:] = B[n:, at] = 1
    return B


def closed_form_count(A):
    A = (np.asarray(A) != 0).astype(np.int64)
    np.fill_diagonal(A, 0)
    alive = np.ones(A.shape[0], dtype=bool)
    count = 1
    while True:  # strip leaves: a factor 2 each
        deg = A[:, alive][alive].sum(axis=1) if alive.any() else np.zeros(0)
        idx = np.flatnonzero(alive)
        leaves = idx[deg == 1]
        if len(leaves) == 0:
            break
        v = leaves[0]
        alive[v] = False
        count *= 2
    idx = np.flatnonzero(alive)
    seen = set()
    for s in idx:
        if s in seen:
            continue
        comp, stack = [], [s]
        seen.add(s)
        while stack:
            v = stack.pop()
            comp.append(v)
            for w in idx[A[v, idx] != 0]:
                if w not in seen:
                    seen.add(w)
                    stack.append(w)
        m = len(comp)
        e = int(A[np.ix_(comp, comp)].sum()) // 2
        if e == 0:
            continue
        if e == m * (m - 1) // 2:
            count *= math.factorial(m)
        elif e == m and all(A[v, comp].sum() == 2 for v in comp):
            count *= 2**m - 2
        else:
            raise ValueError("core of %d vertices and %d edges has no closed form here" % (m, e))
    return count


SMALL = [
    ("forest", lambda: disjoint_union(star(3), tree_path(4))),
    ("cycles", lambda: disjoint_union(cycle(3), cycle(5))),
    ("cycle and tree", lambda: disjoint_union(cycle(4), star(2), tree_path(1))),
    ("complete and cycle", lambda: disjoint_union(complete(4), cycle(5))),
    ("pendants on K_4", lambda: pendant(complete(4), 3)),
    ("pendants on C_5", lambda: pendant(cycle(5), 2, at=2)),
    ("path hanging off K_3", lambda: pendant(pendant(complete(3), 1), 1, at=3)),
    ("isolated vertices", lambda: disjoint_union(np.zeros((3, 3), dtype=np.int64), cycle(4), np.zeros((2, 2), dtype=np.int64))),
]


@pytest.mark.parametrize("name,make", SMALL, ids=[s[0] for s in SMALL])
def test_product_rule_equals_deletion_contraction(name, make):
    A = make()
    assert closed_form_count(A) == chromatic_at_minus_one(A)


def test_closed_forms_of_the_components():
    for k in range(0, 7):
        assert closed_form_count(star(k)) == 2**k == chromatic_at_minus_one(star(k))
    for n in range(3, 8):
        assert closed_form_count(cycle(n)) == 2**n - 2 == chromatic_at_minus_one(cycle(n))
    for n in range(1, 7):
        assert closed_form_count(complete(n)) == math.factorial(n) == chromatic_at_minus_one(complete(n))


def test_a_core_without_a_closed_form_is_refused():
    A = disjoint_union(cycle(4))
    A[0, 2] = A[2, 0] = 1  # C_4 with a chord
    with pytest.raises(ValueError):
        closed_form_count(A)


def test_large_counts_of_the_gpu_cases():
    """The expected counts the GPU tests use at 29 to 32 edges (test_gpu_kernel_matrix.py), by the rule above."""
    assert closed_form_count(disjoint_union(star(16), star(16))) == 1 << 32
    assert closed_form_count(pendant(complete(8), 4)) == math.factorial(8) * 16
    for A in (disjoint_union(star(16), star(16)), pendant(complete(8), 4)):
        assert int(np.triu(A, 1).sum()) == 32
    # permuting the vertices changes nothing
    A = disjoint_union(cycle(5), star(3), complete(4))
    p = np.random.default_rng(1).permutation(A.shape[0])
    assert closed_form_count(A[np.ix_(p, p)]) == closed_form_count(A) == chromatic_at_minus_one(A)
