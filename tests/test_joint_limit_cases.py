"""The cases of tests/joint_limit_cases.py are what they claim (no GPU): every reference search ends PDMPC_OK within the node cap and
reaches the code its case names -- the read-back's item counts, the second mask word, the step a rectangle lies in, the child
counts at the edges of a chunk, an open list beyond 256 entries, the pass of layout_joint --, so that the GPU half
(tests/test_gpu_joint_limits.py) cannot pass vacuously.  It also extends test_joint_reference.py's pin of the reference to the
oracle to Hp 16 and the two larger automata.  Run with -s for the table of node and pop counts per case.
"""
import dataclasses

import numpy as np
import pytest

from pdmpc import abi

import joint_limit_cases as jl
import joint_reference as jr
from test_joint_reference import assert_records_equal

CASES = jl.cases()
NAMES = list(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_reference_ends_ok_within_the_cap_and_reaches_what_the_case_names(name):
    c = CASES[name]
    recs, facts = jl.reference(name)
    N, Hp = len(c.problem), c.options.Hp
    print("\n%-22s N %d Hp %2d: %6d nodes, %5d pops, open list up to %5d, child counts %s" % (name, N, Hp, recs["n_expanded"][0], facts["n_popped"], facts["peak"], sorted(facts["children"])))
    assert (recs["status"] == abi.OK).all()
    assert recs["n_expanded"][0] <= jl.NODE_CAP
    claims = dict(c.claims)
    if "items" in claims:
        assert N * (Hp + 1) == claims.pop("items")
    if "children" in claims:
        assert claims.pop("children") <= facts["children"], sorted(facts["children"])
    if "backs_up" in claims:
        assert facts["n_popped"] > claims.pop("backs_up")
    if "n_words" in claims:
        assert (c.mpa.n_trims + 63) // 64 == claims.pop("n_words")
    if "n_trims" in claims:
        assert c.mpa.n_trims == claims.pop("n_trims")
    if claims.pop("trim_above_64", False):
        assert all(r["predicted_trims"][:Hp].max() > 64 for r in recs), "the winning path holds no trim of the second mask word"
    if claims.pop("crosses_words", False):
        jm = jr.JointMpa(c.mpa)
        lists = [jm.successors(t, e[0] + 1) for e in facts["expanded"] for t in e[1:]]
        assert any(s[0] <= 64 < s[-1] for s in lists), "no expanded node's successor list crosses the mask words"
    if "differs_from" in claims:
        other, _ = jl.reference(claims.pop("differs_from"))
        assert not np.array_equal(recs["y_predicted"], other["y_predicted"])
    if claims.pop("large_offset_only", False):
        # the boundary changes the plan, and it does so through the large-offset area of step Hp alone: with that area replaced
        # by the one without offset the search is the one without boundaries, record for record
        unbounded = [dataclasses.replace(it, predicted_lanelet_boundary=(None, None)) for it in c.problem]
        want = jr.search(c.options, jr.JointMpa(c.mpa), unbounded, jl.NODE_CAP)[0]
        assert not np.array_equal(recs["y_predicted"], want["y_predicted"]) and recs["n_expanded"][0] > want["n_expanded"][0]
        jm = jr.JointMpa(c.mpa)
        plain = jm.maneuver
        jm.maneuver = lambda t1, t2: dataclasses.replace(plain(t1, t2), area_large_offset=plain(t1, t2).area_without_offset)
        assert_records_equal(jr.search(c.options, jm, c.problem, jl.NODE_CAP)[0], want, name)
    if "other_records_than" in claims:  # (the plan may be the same one: the tree and the pops are not)
        other, _ = jl.reference(claims.pop("other_records_than"))
        assert recs.tobytes() != other.tobytes() and (recs["n_expanded"][0], recs["n_popped"][0]) != (other["n_expanded"][0], other["n_popped"][0])
    if "equals" in claims:
        assert_records_equal(recs, jl.reference(claims.pop("equals"))[0], name)
    if "peak_above" in claims:
        assert facts["peak"] > claims.pop("peak_above")
    if "layout" in claims:
        p, heap_lds = claims.pop("layout")
        R = claims.pop("rectangles")
        rc, plan = jl.joint_plan(c.options, c.mpa, jl.launch_soup_cap([c.problem], Hp))
        assert rc == 0 and plan["pass"] == p and plan["areas_in_lds"] == (1 if p in (0, 2) else 0)
        assert (plan["total"] > 64 * 1024) == (p >= 2)
        print("    %d rectangles: pass %d, heap_lds %d, %d bytes of LDS" % (R, p, plan["heap_lds"], plan["total"]))
        if heap_lds is not None:
            assert plan["heap_lds"] == heap_lds
            # ... and one rectangle more is the next pass's, or nothing's
            rc, more = jl.joint_plan(c.options, c.mpa, jl.launch_soup_cap([c.problem], Hp) + 5 * Hp)
            assert (rc == -4) if p == 3 else (rc == 0 and more["pass"] == p + 1)
        else:
            assert plan["heap_lds"] > 256
            rc, fewer = jl.joint_plan(c.options, c.mpa, jl.launch_soup_cap([c.problem], Hp) - 5 * Hp)
            assert rc == 0 and fewer["pass"] == p - 1 and fewer["heap_lds"] == 256
    assert not claims, "claims nobody checked: %s" % sorted(claims)


def test_step_rectangles_lie_where_the_case_says():
    """The `at` variant holds its rectangle in vehicle u's row at step k and nowhere else; `other` in vehicle 0's; `shifted` and
    `adjacent` in vehicle u's at another step.  All other polygons are the far ones."""
    u = jl.SOUP_VEHICLE
    for name, N, Hp, ks in jl.SOUP_SETS:
        for k in ks:
            for tag, veh, step in (("at", u, k), ("other", 0, k), ("shifted", u, jl.shifted_step(k, Hp)), ("adjacent", u, jl.adjacent_step(k, Hp))):
                if "%s_k%d_%s" % (name, k, tag) not in CASES:
                    assert (tag == "adjacent" and N == 3) or (tag == "shifted" and step is None)
                    continue
                c = CASES["%s_k%d_%s" % (name, k, tag)]
                near = [(v, s + 1) for v, it in enumerate(c.problem) for s, poly in enumerate(it.dynamic_obstacle_area[0]) if poly[0].max() < 30.0]
                assert near == [(veh, step)], (c.name, near)
                assert len({id(o) for it in c.problem for o in it.dynamic_obstacle_area[0]}) == N * Hp  # every vehicle a soup of its own
                assert jl.soup_columns(c.problem, Hp) == N * (Hp * 5 + 2)


def test_child_counts_meet_the_edges_of_a_chunk():
    seen = set().union(*(jl.reference(name)[1]["children"] for name in NAMES))
    print("\nchild counts over all cases: %s" % sorted(seen))
    assert {1, 63, 64, 72, 144, 192, 256} <= seen
    assert 64 in seen and any(c > 64 and c % 64 == 0 for c in seen)


@pytest.mark.parametrize("name", ["ss_1_16", "ts_1_16", "re_1_16_from_67"])
def test_single_vehicle_reference_equals_the_oracle_at_hp_16(name):
    from oracle import oracle

    c = CASES[name]
    assert len(c.problem) == 1 and c.options.Hp == 16
    _, want, _ = oracle.plan_batch(c.options, c.mpa, c.problem)
    got = jr.plan_joint(c.options, c.mpa, [c.problem], max_nodes=jr.arena_nodes(c.options))
    assert_records_equal(got, want, name)
    assert_records_equal(got, jl.reference(name)[0], name)


def test_arena_edge_cases_reach_one_side_each():
    """An even tree size fits its arena exactly, an odd one is one node short of the arena below (arenas are even)."""
    sides = set()
    for name in jl.ARENA_EDGE:
        c = CASES[name]
        n = int(jl.reference(name)[0]["n_expanded"][0])
        fits, short = jl.arena_edge_sizes(n)
        assert fits % 2 == 0 and short % 2 == 0 and short < n <= fits
        sides.add("exact" if fits == n else "one short")
        assert short == n - 1 or fits == n
        over = jr.plan_joint(c.options, c.mpa, [c.problem], max_nodes=short)
        assert (over["status"] == abi.ARENA_OVERFLOW).all() and over["n_expanded"][0] <= short
        assert_records_equal(jr.plan_joint(c.options, c.mpa, [c.problem], max_nodes=fits), jl.reference(name)[0], name)
    assert sides == {"exact", "one short"}


def test_soup_capacity_is_layout_joints_at_every_pass():
    """centralized_cases.joint_soup_capacity against pdmpc_launch_plan_host: the largest soup_cap of every pass is the plan's of
    that pass, one more column is the next one's (or does not fit).  The realistic automaton's 527 maneuvers' areas never fit:
    passes 0 and 2 are never taken; triple_speed's do not fit 64 KB beside its tables of Hp 16."""
    for name, passes in (("open_list_p0_last", [0, 1, 2, 3]), ("re_3_16", [1, 3]), ("ts_2_16", [1, 2, 3])):
        c = CASES[name]
        Hp = c.options.Hp
        caps = [jl.pass_capacity(c.mpa, Hp, p) for p in range(4)]
        taken = [p for p in range(4) if caps[p] > 0 and all(caps[q] < caps[p] for q in range(p))]
        assert taken == passes, caps
        for i, p in enumerate(taken):
            rc, plan = jl.joint_plan(c.options, c.mpa, caps[p])
            assert rc == 0 and plan["pass"] == p and plan["heap_lds"] == 256, (name, p, plan)
            rc, plan = jl.joint_plan(c.options, c.mpa, caps[p] + 1)
            assert (rc == -4) if p == 3 else (rc == 0 and plan["pass"] == taken[i + 1] and plan["heap_lds"] > 256), (name, p)
        # ... and the on-path problem itself, a few columns of soup, is the first pass's
        rc, plan = jl.joint_plan(c.options, c.mpa, jl.launch_soup_cap([c.problem], Hp) if "open_list" not in name else 6)
        assert rc == 0 and plan["pass"] == taken[0]
