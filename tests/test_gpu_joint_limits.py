"""The joint search (pdmpc_plan_joint, joint_kernel.hip) at its horizon, vehicle, automaton and layout limits against the CPU
reference (tests/joint_reference.py): records byte-identical, no tolerances.

The cases are tests/joint_limit_cases.py's; tests/test_joint_limit_cases.py shows on the CPU that each reaches the code it names
(Hp 15 and 16 with four vehicles, both larger automata and the second mask word, a rectangle in one vehicle's soup of one step,
child counts of 1, 63, 64, 72, 144, 192 and 256, open lists beyond the 256 entries of the smallest LDS part, either side of every
pass edge of layout_joint, an arena that fits exactly or is one node short).  A case's reference search is computed once (in an arena
of joint_limit_cases.NODE_CAP nodes); where the handle's arena holds the reference's tree -- asserted -- that is
jr.plan_joint(..., max_nodes=h.arena_nodes()[0]): the arena enters the search in its overflow test alone.
"""
import dataclasses

import pytest

from pdmpc import abi
from pdmpc.backend import BackendError, Handle

import joint_limit_cases as jl
import joint_reference as jr
from test_joint_reference import assert_records_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

CASES = jl.cases()
NAMES = list(CASES)


@pytest.fixture(scope="module")
def handles():
    """one handle per (automaton, Hp), with the automaton uploaded"""
    made = {}

    def get(case):
        key = (case.options.mpa_type, case.options.Hp)
        if key not in made:
            made[key] = Handle(case.options)
            made[key].upload_mpa(case.mpa)
        return made[key]

    yield get
    for h in made.values():
        h.close()


def device_soup_columns(h, first, N):
    """pdmpc_joint_soup_columns (csrc/pdmpc_device.h) from the offsets the last pack gave the problem's vehicles"""
    offs = [h.packed_offsets(first + v) for v in range(N)]
    need = 0
    for v, (lit, _, ll) in enumerate(offs):
        if not any(offs[u][0] == lit for u in range(v)):
            need += lit[-1] - lit[0]
        if not any(offs[u][2] == ll for u in range(v)):
            need += ll[1]
    return need


def check_layout(h, case, problems):
    """The launch's LDS bytes are those of the plan for the soup columns the packer counted, which are the ones the case computed."""
    Hp = case.options.Hp
    at, cols = 0, []
    for prob in problems:
        cols.append(device_soup_columns(h, at, len(prob)))
        at += len(prob)
    assert cols == [jl.soup_columns(prob, Hp) for prob in problems]
    rc, plan = jl.joint_plan(case.options, case.mpa, max(cols) + 2)
    assert rc == 0 and h.stats()["lds_bytes"] == plan["total"]
    return plan


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_reference(handles, name):
    c = CASES[name]
    want, _ = jl.reference(name)
    h = handles(c)
    got = h.plan_joint([c.problem])
    st = h.stats()
    assert st["kernel"] == 4
    assert h.arena_nodes()[0] >= int(want["n_expanded"][0])
    plan = check_layout(h, c, [c.problem])
    print("\n%-22s pass %d (areas in %s), heap_lds %d, %d bytes of LDS, arena %d" % (name, plan["pass"], "LDS" if plan["areas_in_lds"] else "L2", plan["heap_lds"], plan["total"], h.arena_nodes()[0]))
    assert_records_equal(got, want, name)
    if "layout" in c.claims:
        p, heap_lds = c.claims["layout"]
        assert plan["pass"] == p and plan["areas_in_lds"] == (1 if p in (0, 2) else 0) and (st["lds_bytes"] > 64 * 1024) == (p >= 2)
        assert plan["heap_lds"] == heap_lds if heap_lds is not None else plan["heap_lds"] > 256
    if c.mpa.n_trims > 64:
        assert plan["areas_in_lds"] == 0  # (527 maneuvers: the areas stay in L2)


@pytest.mark.parametrize("automaton", list(jl.HORIZON))
def test_horizon_cases_of_an_automaton_in_one_launch_equal_each_alone(handles, automaton):
    """The mixed-size launch at Hp 16: 4, 3, 1 and 2 vehicles of single_speed; 2 and 1 of triple_speed; 3 and 1 of realistic."""
    names = jl.HORIZON[automaton]
    cs = [CASES[n] for n in names]
    assert all(c.options.Hp == 16 and c.options.mpa_type == cs[0].options.mpa_type for c in cs)
    h = handles(cs[0])
    together = h.plan_joint([c.problem for c in cs])
    assert h.stats()["kernel"] == 4 and h.stats()["n_vehicles"] == sum(len(c.problem) for c in cs)
    check_layout(h, cs[0], [c.problem for c in cs])
    at = 0
    for c in cs:
        N = len(c.problem)
        want, _ = jl.reference(c.name)
        assert h.arena_nodes()[0] >= int(want["n_expanded"][0])
        assert_records_equal(together[at : at + N], want, "%s in the launch" % c.name)
        assert_records_equal(h.plan_joint([c.problem]), want, "%s alone" % c.name)
        at += N


def test_small_open_list_behind_other_problems_of_the_launch(handles):
    """first > 0: the problem whose open list has 256 entries of LDS, second and third in a launch behind a one-vehicle problem, reads
    and writes the far list of ITS first slot (slots 1 and 3)."""
    c = CASES["open_list_p3_last"]
    want, facts = jl.reference(c.name)
    assert facts["peak"] > 256
    small = jl.small_problem()
    h = handles(c)
    got = h.plan_joint([small, c.problem, c.problem])
    plan = check_layout(h, c, [small, c.problem, c.problem])
    assert h.stats()["kernel"] == 4 and plan["heap_lds"] == 256 and plan["pass"] == 3
    assert h.arena_nodes()[0] >= int(want["n_expanded"][0])
    assert_records_equal(got[1:3], want, "second in the launch")
    assert_records_equal(got[3:5], want, "third in the launch")
    assert_records_equal(got[0:1], jr.plan_joint(c.options, c.mpa, [small], max_nodes=h.arena_nodes()[0]), "the small problem")


@pytest.mark.parametrize("name", jl.ARENA_EDGE)
def test_arena_edge(name):
    """The smallest arena that holds the reference's tree: PDMPC_OK and the reference's records; the next smaller arena (arenas are
    even: two nodes fewer): PDMPC_ARENA_OVERFLOW and the reference's overflow record."""
    c = CASES[name]
    want, _ = jl.reference(name)
    fits, short = jl.arena_edge_sizes(int(want["n_expanded"][0]))
    for size in (fits, short):
        h = Handle(dataclasses.replace(c.options, max_nodes=size))
        h.upload_mpa(c.mpa)
        h.set_arena_limit(size)
        h.allow_overflow = True
        got = h.plan_joint([c.problem])
        assert h.stats()["kernel"] == 4 and h.arena_nodes() == (size, 0)
        if size == fits:
            assert (got["status"] == abi.OK).all()
            assert_records_equal(got, want, "%s in an arena of %d" % (name, size))
        else:
            assert (got["status"] == abi.ARENA_OVERFLOW).all()
            assert_records_equal(got, jr.plan_joint(c.options, c.mpa, [c.problem], max_nodes=size), "%s in an arena of %d" % (name, size))
            h.allow_overflow = False
            with pytest.raises(BackendError):
                h.plan_joint([c.problem])
        h.close()
