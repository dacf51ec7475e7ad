"""The sampled optimizer's expansion budget without a GPU: the restatement the GPU tests compare with (sampled_budget_reference.py)
against the oracle at the reference's budget, the properties a budget must have, the plan of a budgeted launch through its window
(pdmpc_sampled_plan_host) and the argument checks of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import problems
import sampled_budget_reference as sbr
from oracle import oracle
from pdmpc import abi, backend
from pdmpc.config import MpaType

INVALID, CAPACITY = -1, -4


@pytest.mark.parametrize("mpa_type", [MpaType.single_speed, MpaType.triple_speed], ids=["single", "triple"])
@pytest.mark.parametrize("Hp", [5, 8])
@pytest.mark.parametrize("mode", ["interx", "sat"])
def test_restatement_at_250_is_the_oracle_byte_for_byte(mode, Hp, mpa_type):
    options, mpa, iters = problems.problem_set(mode, 11 + Hp, 12, Hp=Hp, mpa_type=mpa_type, n_hdv=1 if mode == "interx" else 0)
    seeds = [3 + i for i in range(len(iters))]
    _, want = oracle.plan_batch_sampled(options, mpa, iters, seeds)
    got = sbr.plan_batch_sampled(options, mpa, iters, seeds, budget=250)
    assert got.tobytes() == want.tobytes()
    assert (want["status"] == 0).any()


BUDGETS = [1, 2, 7, 32, 100, 250, 251, 600, 1500, 3000]


@pytest.fixture(scope="module")
def ladder():
    """Records of the same problems and seeds at rising budgets (computed once)."""
    out = {}
    for mode in ("interx", "sat"):
        options, mpa, iters = problems.problem_set(mode, 5, 6, Hp=5)
        sm = sbr.SampledMpa(mpa)
        seeds = [9 + i for i in range(len(iters))]
        out[mode] = (options, {b: sbr.plan_batch_sampled(options, sm, iters, seeds, budget=b) for b in BUDGETS})
    return out


@pytest.mark.parametrize("mode", ["interx", "sat"])
def test_prefix_property_of_rising_budgets(ladder, mode):
    """The descents of a smaller budget are the first descents of a larger one (the same stream, consumed in the same order), so a
    plan found stays found and the best cost never rises; a budget that lets the tree run dry (fewer expansions than the budget:
    the search ended at the root) changes nothing from there on."""
    options, recs = ladder[mode]
    Hp = options.Hp
    dry_seen = 0
    for b1, b2 in zip(BUDGETS[:-1], BUDGETS[1:]):
        for v in range(len(recs[b1])):
            r1, r2 = recs[b1][v], recs[b2][v]
            assert int(r1["n_popped"]) <= Hp * b1  # (no index beyond the drawn numbers: the streams of b1 and b2 agree where b1 reads)
            assert int(r1["n_expanded"]) <= b1 + Hp - 1 and int(r2["n_expanded"]) <= b2 + Hp - 1
            if int(r1["status"]) == 0:
                assert int(r2["status"]) == 0
                assert float(r2["path_nodes"][Hp][4]) <= float(r1["path_nodes"][Hp][4])
            if int(r1["n_expanded"]) < b1:  # ran dry
                dry_seen += 1
                assert r1.tobytes() == r2.tobytes()
    assert dry_seen > 0


QUERY = dict(checker=abi.CHECK_INTERX, Hp=6, n_trims=12, n_man=40, n_cu=256, device_share=1, max_nodes=32768, kind=1, count=20, n_chained=0, soup_cap=400, ll_cap=80,
             cand_cap=300, safe=0)


def launch_plan(query):
    lib = backend.load_library()
    q, p = abi.LaunchQuery(**query), abi.LaunchPlan()
    rc = lib.pdmpc_launch_plan_host(None, C.byref(q), C.byref(p))
    plan = {f: getattr(p, f) for f, _ in abi.LaunchPlan._fields_}
    plan["kernel"] = plan["kernel"].decode() if plan["kernel"] else ""
    return rc, plan


@pytest.mark.parametrize("safe", [0, 1])
@pytest.mark.parametrize("checker", [abi.CHECK_INTERX, abi.CHECK_SAT])
def test_default_budget_is_todays_plan_field_for_field(checker, safe):
    query = dict(QUERY, checker=checker, safe=safe)
    rc0, want = launch_plan(query)
    rc1, got, extra = backend.sampled_plan_host(query, 250)
    assert rc0 == 0 and rc1 == 0
    assert got == want and got["kernel"] == "pdmpc_sampled_kernel"
    assert extra == {"node_cap": 288, "tree_in_lds": 1, "tree_hbm_bytes": 0, "rand_chunk": query["Hp"] * 250}


@pytest.mark.parametrize("Hp", [1, 6, 16])
@pytest.mark.parametrize("budget", [1, 7, 249, 251, 1000, 4096, 16384])
def test_other_budgets_plan_the_new_kernel_with_room_for_every_node(budget, Hp):
    query = dict(QUERY, Hp=Hp)
    rc, plan, extra = backend.sampled_plan_host(query, budget)
    assert rc == 0
    assert plan["kernel"].startswith("pdmpc_sampled_budget_kernel")
    assert extra["node_cap"] >= 1 + budget + Hp
    assert extra["node_cap"] - 1 <= 0xFFFF  # node ids are 16-bit
    assert extra["rand_chunk"] == 312
    row_bytes = 36
    if extra["tree_in_lds"]:
        assert plan["kernel"] == "pdmpc_sampled_budget_kernel" and extra["tree_hbm_bytes"] == 0
        assert plan["total"] >= plan["tree16"] + extra["node_cap"] * row_bytes and plan["total"] <= 160 * 1024
    else:
        assert plan["kernel"] == "pdmpc_sampled_budget_kernel_hbm"
        assert extra["tree_hbm_bytes"] == extra["node_cap"] * row_bytes and extra["tree_hbm_bytes"] <= 600 * 1024
        assert plan["total"] <= 160 * 1024
    # the generator's state has a region of its own behind the rest, in front of the tree
    assert plan["rand"] + 624 * 4 <= plan["tree16"] <= plan["total"]
    assert plan["n_waves"] == 1


def test_the_tree_leaves_lds_at_one_budget_and_stays_out():
    """80 KB first, then 160 KB, then HBM: tree_in_lds falls once over the budgets, the LDS total never exceeds the CU's."""
    edge = None
    prev_in_lds = 1
    for budget in list(range(1, 6000, 37)) + [16384]:
        if budget == 250:
            continue
        rc, plan, extra = backend.sampled_plan_host(QUERY, budget)
        assert rc == 0 and plan["total"] <= 160 * 1024
        assert extra["tree_in_lds"] <= prev_in_lds
        if prev_in_lds and not extra["tree_in_lds"]:
            edge = budget
        prev_in_lds = extra["tree_in_lds"]
    assert edge is not None and edge > 1000


def test_argument_checks():
    lib = backend.load_library()
    n = C.c_int32(0)
    assert lib.pdmpc_set_sampled_budget(None, 64) == INVALID
    assert lib.pdmpc_get_sampled_budget(None, C.byref(n)) == INVALID
    assert lib.pdmpc_last_sampled_kernel(None) == b""
    assert lib.pdmpc_debug_random_stream(None, 1, None, 1, None) == INVALID
    q, p = abi.LaunchQuery(**QUERY), abi.LaunchPlan()
    x = (C.c_int64 * 4)()
    assert lib.pdmpc_sampled_plan_host(None, None, 64, C.byref(p), x) == INVALID
    assert lib.pdmpc_sampled_plan_host(None, C.byref(q), 64, None, x) == INVALID
    assert lib.pdmpc_sampled_plan_host(None, C.byref(q), 64, C.byref(p), None) == INVALID
    for bad in (0, -1, 16385, 1 << 30):
        assert lib.pdmpc_sampled_plan_host(None, C.byref(q), bad, C.byref(p), x) == INVALID
        assert b"budget" in lib.pdmpc_last_error()
    assert lib.pdmpc_sampled_plan_host(b"no_such_key=1", C.byref(q), 64, C.byref(p), x) == INVALID
    for ok in (1, 16384):
        assert lib.pdmpc_sampled_plan_host(None, C.byref(q), ok, C.byref(p), x) == 0
    huge = abi.LaunchQuery(**dict(QUERY, soup_cap=20000))
    assert lib.pdmpc_sampled_plan_host(None, C.byref(huge), 64, C.byref(p), x) == CAPACITY
    assert backend.SAMPLED_BUDGET_DEFAULT == 250 and backend.SAMPLED_BUDGET_MAX == 16384


def test_config_carries_the_budget():
    from pdmpc.config import Config

    assert Config().n_expansions_max == 250
    assert Config(n_expansions_max=64).n_expansions_max == 64
