"""What the tests of the reachable-set geometry share (tests/test_exact_reachable_geometry.py, tests/test_gpu_reachable_limits.py): the
check of one bounded set against the exact K ∩ L, the coupling decisions of a family, the gear cases, and the writer of
profiles/exact_geometry_errors.txt.  The reference itself is tests/exact_geometry.py."""
import os
from fractions import Fraction

import numpy as np

import exact_geometry as X
from pdmpc import reachability as R


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Decisions:
    """the coupling bits of a family against the exact decision"""

    def __init__(self):
        self.n = self.left_out = 0

    def check(self, bit, exact, tol, what):
        self.n += 1
        if X.decision_is_safe(exact, tol):
            assert bool(bit) == X.coupled(exact), what
        else:
            self.left_out += 1

    def assert_share(self):
        assert self.n > 0 and self.left_out <= 0.01 * self.n, "%d of %d pairs lie within the tolerance of the 1e-3 threshold" % (self.left_out, self.n)


class Pinches:
    """how many bounded sets of a family were held to the weak notion of simple because the exact K ∩ L is pinched"""

    def __init__(self):
        self.n = self.pinched = 0

    def add(self, pinched):
        self.n += 1
        self.pinched += bool(pinched)

    def assert_share(self, cap):
        """cap: the share of a family that may be pinched.  Whether a case is pinched follows from K and L alone, in exact arithmetic,
        so the share is a property of the generator, not of the code under test: 0 in general position and for the gears; on lattices
        of 4 to 9 units, which are there to make such coincidences, a reflex vertex of L lands on ∂K in 2 to 5 % of the cases (0.1)."""
        assert self.n > 0 and self.pinched <= cap * self.n, "%d of %d bounded sets are pinched: the strict check covers too few" % (self.pinched, self.n)


def _edge_part(a, b, K):
    """the parameters (t0, t1) of the part of the segment a -> b strictly inside the clockwise convex K, exactly; None if there is none
    (an edge along an edge of K has none)"""
    t0, t1 = Fraction(0), Fraction(1)
    for k in range(len(K)):
        p, q = K[k], K[(k + 1) % len(K)]
        ca, cb = X.cross(p, q, a), X.cross(p, q, b)
        if ca == cb:
            if ca >= 0:
                return None
        elif ca > cb:  # leaving the outside: an entry
            t0 = max(t0, Fraction(ca) / (ca - cb))
        else:
            t1 = min(t1, Fraction(ca) / (ca - cb))
    return (t0, t1) if t0 < t1 else None


def _parts(K, Ln):
    return [_edge_part(Ln[i], Ln[(i + 1) % len(Ln)], K) for i in range(len(Ln))]


def _chain_starts(parts):
    n = len(parts)
    if all(p is not None and p == (0, 1) for p in parts):
        return []
    return [i for i in range(n) if parts[i] is not None and not (parts[i][0] == 0 and parts[i - 1] is not None and parts[i - 1][1] == 1)]


def count_chains(K, Ln):
    """the number of maximal runs of L's boundary strictly inside K, from exact clipping of every L edge: an edge has a part inside iff
    its clip by K has positive length; two consecutive parts join iff the first reaches its edge's end and the second starts at its
    edge's start"""
    return len(_chain_starts(_parts(K, Ln)))


def chain_entries(K, Ln):
    """(L edge the chain starts on, exact entry point) of every chain"""
    parts = _parts(K, Ln)
    out = []
    for i in _chain_starts(parts):
        a, b, t = Ln[i], Ln[(i + 1) % len(Ln)], parts[i][0]
        out.append((i, (a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]))))
    return out


def pinch_vertices(K, Ln):
    """The vertices of L at which the exact K ∩ L is pinched, decided exactly: a reflex vertex of L on ∂K whose two edges both run on into
    K's interior.  The chain goes through it (both parts are inside), L's interior there is the outside of the angle between them, so
    inside K it is two sectors that touch in the vertex, and ∂K bounds both: the boundary of K ∩ L passes the vertex twice."""
    D, (k, l) = X._integers(K, Ln)
    n, m = len(l), len(k)
    out = []
    for i in range(n):
        u, v, w = l[i - 1], l[i], l[(i + 1) % n]
        if X.cross(u, v, w) <= 0:  # (clockwise: a right turn or straight on is not reflex)
            continue
        side = [X.cross(k[j], k[(j + 1) % m], v) for j in range(m)]
        if max(side) != 0:  # not on ∂K
            continue
        before, after = _edge_part(u, v, k), _edge_part(v, w, k)
        if before is not None and after is not None and before[1] == 1 and after[0] == 0:
            out.append(i)
    return out


def check_bounded_set(errors, family, twin, r, flag, K, Ln, lattice, what, triangles=None, thorough=True, pinches=None):
    """One bounded set r (closed (2, c) array) of the clockwise convex K and the clockwise lanelet polygon Ln against the exact K ∩ L,
    by its flag.  `triangles`: a triangulation of Ln (default: ear clipping).  thorough = False leaves out area(r ∩ K) and
    area(r ∩ L) and the check of the first chain, which cost minutes in exact arithmetic at the largest sizes.  `pinches`: a Pinches
    that counts the cases held to the weak notion of simple.  Returns the exact area of K ∩ L."""
    r = np.asarray(r)
    assert r.shape[1] >= 4 and r[0, 0] == r[0, -1] and r[1, 0] == r[1, -1], (family, what, "not closed")
    full = X.area_convex_simple(K, Ln)
    aK, aL = X.area(K), X.area(Ln)
    tol = X.tolerance(full, aK, aL)
    if flag & R.BOUND_RESTORED:
        assert flag == R.BOUND_RESTORED, (family, what, flag)
        assert np.array_equal(bits(r[:, :-1]), bits(X.arr(K))), (family, what, "restored, but not K")
        assert full == 0 if lattice else full <= tol, (family, what, float(full))
        return full
    P = X.poly(r)
    ar = X.area(P)
    assert ar > 0, (family, what, "not clockwise")
    assert all(P[i] != P[i - 1] for i in range(len(P))), (family, what, "a vertex twice in a row")  # (an entry or exit on a vertex of K is that vertex)
    # simple, by exact orientation tests — except where the exact K ∩ L is itself pinched (pinch_vertices): there r is its boundary, which
    # touches itself in the pinch vertex, and with the rounded entry and exit points next to it the edges cross by less than an ulp
    pinched = bool(pinch_vertices(K, Ln))
    if pinches is not None:
        pinches.add(pinched)
    if pinched:
        assert X.has_no_crossing(P, X.rounding_slack(K, Ln)), (family, what, "edges cross at a pinch")
    else:
        assert X.is_simple(P), (family, what, "not simple")
    unit = X.error_unit(K, Ln)
    if thorough:
        inK = X.area(X.clip_convex(P, K))
        inL = X.area_simple_simple(Ln, P, triangles)
        for name, part in (("r in K", inK), ("r in L", inL)):
            err = abs(part - ar)
            errors.add(family + ", " + name, twin, err, unit)
            assert err <= tol, (family, what, name, float(part), float(ar))
            if lattice:
                assert err <= 1e-12, (family, what, name, float(err))
    if flag & R.BOUND_MULTIPLE:
        assert flag == R.BOUND_MULTIPLE and ar < full - Fraction(tol), (family, what, float(ar), float(full))
        return full
    assert flag == 0, (family, what, flag)
    err = abs(ar - full)
    errors.add(family, twin, err, unit)
    assert err <= tol, (family, what, float(ar), float(full), float(err), tol)
    if lattice:
        assert err <= 1e-12, (family, what, float(err))
    # where it starts: K itself from its first vertex; L itself from its first vertex if every L edge runs through K's interior (L
    # inside K, no edge along an edge of K); otherwise at a point where L enters K
    if len(P) == len(K) and ar == aK:
        assert P == K, (family, what, "K, but not from its first vertex")
    elif all(X.cross(K[k], K[(k + 1) % len(K)], v) <= 0 for k in range(len(K)) for v in Ln) and not any(
        X.cross(K[k], K[(k + 1) % len(K)], Ln[i]) == 0 and X.cross(K[k], K[(k + 1) % len(K)], Ln[(i + 1) % len(Ln)]) == 0
        for k in range(len(K)) for i in range(len(Ln))
    ):
        assert P == Ln, (family, what, "L, but not from its first vertex")
    else:
        assert X.boundary_distance(P[0], K) <= 1e-9 and X.boundary_distance(P[0], Ln) <= 1e-9, (family, what, "does not start at an entry")
        if thorough:  # ... and of the region's chains (those whose exact entry point is a vertex of r) the one that starts on the smallest L edge
            slack = Fraction(X.rounding_slack(K, Ln))
            near = lambda p, q: abs(p[0] - q[0]) <= slack and abs(p[1] - q[1]) <= slack  # noqa: E731
            mine = [(e, q) for e, q in chain_entries(K, Ln) if any(near(q, v) for v in P)]
            assert mine and near(min(mine)[1], P[0]), (family, what, "does not start at the entry of the region's first chain")
    return full




def gear_case(T, M=None, drop=None, phase=0.0, cx=0.0, cy=0.0, bits=24):
    """(K, L): the T-tooth gear against the aligned M-gon (default M = T), vertex `drop` of the M-gon taken out"""
    K = X.ngon(T if M is None else M, 1.0, phase, cx, cy, bits)
    if drop is not None:
        K = K[:drop] + K[drop + 1 :]
        assert X.is_convex_clockwise(K)
    return K, X.gear(T, 0.9, 1.2, phase, cx, cy, bits)


def chains_case(chains, T=None, phase=0.0, cx=0.0, cy=0.0, bits=24):
    """(K, L) with exactly `chains` chains: the T-tooth gear with `chains` deep valleys (radius 0.9, the first ones) and the others
    shallow (radius 1.05: outside), against the aligned T-gon"""
    T = max(chains + 1, 8) if T is None else T
    return X.ngon(T, 1.0, phase, cx, cy, bits), X.gear(T, [0.9] * chains + [1.05] * (T - chains), 1.2, phase, cx, cy, bits)


def write_report(errors, section):
    """Writes the worst observed errors (a record, not a threshold) into the file PDMPC_EXACT_GEOMETRY_REPORT names, if it names one, as
    that file's section `section`; the sections other runs wrote stay (profiles/exact_geometry_errors.txt is two runs into one file: the
    CPU module's and the GPU module's)."""
    path = os.environ.get("PDMPC_EXACT_GEOMETRY_REPORT")
    if not path:
        return None
    sections = {}
    if os.path.exists(path):
        name = None
        for line in open(path).read().splitlines():
            if line.startswith("## "):
                name = line[3:]
                sections[name] = []
            elif name is not None and line:
                sections[name].append(line)
    sections[section] = errors.lines()
    with open(path, "w") as f:
        f.write(REPORT_HEADER)
        for name in sorted(sections):
            f.write("\n## %s\n%s\n" % (name, "\n".join(sections[name])))
    return path


REPORT_HEADER = """Worst observed error of the reachable-set geometry against exact arithmetic (tests/exact_geometry.py), per family and twin.
A record, not a threshold.  'in units': the error divided by eps * (m_a + m_b) * R^2, m the vertex counts, R the largest coordinate
magnitude.  Written by tests/test_exact_reachable_geometry.py (python, host) and tests/test_gpu_reachable_limits.py (device, one
MI355X), each run with PDMPC_EXACT_GEOMETRY_REPORT=<this file>; a run replaces its own section.
Bounding families: |area(r) - area(K n L)| of the sets flagged 0; 'r in K' / 'r in L': |area(r n K) - area(r)| and
|area(r n L) - area(r)| of every set not restored.  On lattices of up to 8 units every family also holds 1e-12 absolute (asserted).
Sections 'edge checks, ...': the search's collision primitives (InterX, intersect_sat, intersect_lanelet_boundary) against proper
crossings and the exact normalised gap, written by tests/test_exact_edge_checks.py (the oracle) and tests/test_gpu_edge_check_limits.py
(the device) in the same way.  Per family: cases, the ones with an exact verdict (judged), the ones double arithmetic could decide either
way (undecided, by 64 eps R^2 on an orientation value and 32 eps R on a gap) and the decided ones answered wrongly (asserted: 0).
'double gap' rows: |gap in double arithmetic - exact gap| of the SAT families, in units of eps * R; the bound behind the slack is 14.
"""
