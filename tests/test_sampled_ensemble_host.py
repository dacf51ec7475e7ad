"""Seed ensembles of the sampled optimizer without a GPU (pdmpc_set_sampled_ensemble): the header's seed rule against
the twin's, the plan of an ensemble launch through its window (pdmpc_sampled_ensemble_plan_host), the twin the GPU tests compare with
(sampled_ensemble_reference.py), the argument checks of the new entry points and the new kernel's resources."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sampled_ensemble_cases as sec
import sampled_ensemble_reference as ser
import sampled_step_reference as ssr
from pdmpc import abi, backend

INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
RECORD_BYTES = abi.VEHICLE_OUT_DTYPE.itemsize

QUERY = dict(checker=abi.CHECK_INTERX, Hp=6, n_trims=12, n_man=40, n_cu=256, device_share=1, max_nodes=32768, kind=1, count=20, n_chained=0, soup_cap=400, ll_cap=80,
             cand_cap=300, safe=0)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1])
def test_the_headers_seed_rule_is_the_twins(seed):
    header = open(os.path.join(ROOT, "include", "pdmpc.h")).read()
    assert re.search(r"#define PDMPC_SAMPLED_ENSEMBLE_STRIDE 1000003u\b", header) and re.search(r"#define PDMPC_SAMPLED_ENSEMBLE_MAX 16\b", header)
    assert backend.SAMPLED_ENSEMBLE_STRIDE == ser.STRIDE == 1000003 and backend.SAMPLED_ENSEMBLE_MAX == ser.MEMBERS_MAX == 16
    for e in range(16):
        got = backend.sampled_member_seed(seed, e)  # (PDMPC_SAMPLED_MEMBER_SEED, evaluated by the library)
        assert got == ser.member_seed(seed, e) == (seed + e * 1000003) % 2 ** 32
    assert backend.sampled_member_seed(seed, 0) == seed  # member 0 is the reference's stream


def hbm_budget(query):
    """The smallest budget of a coarse ladder whose tree the plan puts in HBM."""
    for budget in range(1000, 16385, 500):
        rc, _, extra = backend.sampled_plan_host(query, budget)
        assert rc == 0
        if not extra["tree_in_lds"]:
            return budget
    raise AssertionError("no budget puts the tree in HBM")


@pytest.mark.parametrize("safe", [0, 1])
@pytest.mark.parametrize("budget", [250, 40, "hbm"])
def test_one_member_is_the_budgets_plan_field_for_field(budget, safe):
    query = dict(QUERY, safe=safe)
    if budget == "hbm":
        budget = hbm_budget(query)
    rc0, want, want_extra = backend.sampled_plan_host(query, budget)
    rc1, got, extra = backend.sampled_ensemble_plan_host(query, budget, 1)
    assert rc0 == 0 and rc1 == 0
    assert got == want
    assert {k: extra[k] for k in want_extra} == want_extra
    assert extra["member_bytes"] == 0 and extra["ensemble_tree_bytes"] == 0 and extra["n_members"] == 1
    assert extra["grid"] == min(got["slice"], query["count"])


@pytest.mark.parametrize("n_members", [2, 16])
@pytest.mark.parametrize("budget", [250, 40, "hbm"])
def test_an_ensemble_plans_its_kernel_its_grid_and_its_bytes(budget, n_members):
    in_hbm = budget == "hbm"
    if in_hbm:
        budget = hbm_budget(QUERY)
    rc, plan, extra = backend.sampled_ensemble_plan_host(QUERY, budget, n_members)
    assert rc == 0
    assert plan["kernel"] == ("pdmpc_sampled_ensemble_kernel_hbm" if in_hbm else "pdmpc_sampled_ensemble_kernel")
    assert plan["slice"] == QUERY["count"] and extra["grid"] == QUERY["count"] * n_members and extra["n_members"] == n_members
    assert extra["member_bytes"] == n_members * RECORD_BYTES
    assert extra["tree_in_lds"] == (0 if in_hbm else 1)
    assert extra["ensemble_tree_bytes"] == n_members * extra["tree_hbm_bytes"] and (extra["ensemble_tree_bytes"] > 0) == in_hbm
    # the layout is the budget kernel's at every budget, the default included: the generator's state, then the tree
    if budget != 250:
        _, single, single_extra = backend.sampled_plan_host(QUERY, budget)
        for field in ("total", "rand", "tree16", "soup", "areas_in_lds", "spin_limit", "reverse_dispatch"):
            assert plan[field] == single[field], field
        assert extra["node_cap"] == single_extra["node_cap"]
    assert extra["rand_chunk"] == 312 and extra["node_cap"] >= 1 + budget + QUERY["Hp"]
    assert plan["rand"] + 624 * 4 <= plan["tree16"] <= plan["total"] <= 160 * 1024
    # the safe mode's slices count slots that are resident with all their members
    rc, safe_plan, safe_extra = backend.sampled_ensemble_plan_host(dict(QUERY, safe=1, count=600), budget, n_members)
    assert rc == 0
    per_cu = 2 if safe_plan["total"] <= 80 * 1024 else 1
    assert safe_plan["slice"] == per_cu * QUERY["n_cu"] // n_members
    assert safe_extra["grid"] == min(safe_plan["slice"], 600) * n_members <= per_cu * QUERY["n_cu"]


def test_argument_checks():
    lib = backend.load_library()
    q, p = abi.LaunchQuery(**QUERY), abi.LaunchPlan()
    x = (C.c_int64 * 8)()
    for bad in (0, 17, -1, 1 << 20):
        assert lib.pdmpc_sampled_ensemble_plan_host(None, C.byref(q), 250, bad, C.byref(p), x) == INVALID
        assert b"ensemble" in lib.pdmpc_last_error()
    for bad_budget in (0, 16385):
        assert lib.pdmpc_sampled_ensemble_plan_host(None, C.byref(q), bad_budget, 4, C.byref(p), x) == INVALID
    assert lib.pdmpc_sampled_ensemble_plan_host(None, None, 250, 4, C.byref(p), x) == INVALID
    assert lib.pdmpc_sampled_ensemble_plan_host(None, C.byref(q), 250, 4, None, x) == INVALID
    assert lib.pdmpc_sampled_ensemble_plan_host(None, C.byref(q), 250, 4, C.byref(p), None) == INVALID
    assert lib.pdmpc_sampled_ensemble_plan_host(b"no_such_key=1", C.byref(q), 250, 4, C.byref(p), x) == INVALID
    n = C.c_int32(0)
    assert lib.pdmpc_set_sampled_ensemble(None, 4) == INVALID and lib.pdmpc_get_sampled_ensemble(None, C.byref(n)) == INVALID
    assert lib.pdmpc_sampled_ensemble_result(None, 0, None, None, None) == INVALID
    assert lib.pdmpc_group_set_sampled_ensemble(None, 4) == INVALID


def test_config_carries_the_ensemble_size():
    from pdmpc.config import Config

    assert Config().n_members == 1 and Config(n_members=4).n_members == 4


@pytest.mark.parametrize("name", ["circle", "road"])
def test_the_twin_with_one_member_is_the_step_reference(name):
    options, mpa, prob, seeds = sec.case(name)
    recs, winners, costs = sec.twin(name, 1, 250)
    want = ssr.plan_step_sampled(options, mpa, prob, seeds)
    assert recs.tobytes() == np.asarray(want).tobytes()
    assert winners.tolist() == [0] * len(seeds) and costs.shape == (1, len(seeds))


@pytest.mark.parametrize("budget", [250, 12])
@pytest.mark.parametrize("n_members", [2, 3, 16])
@pytest.mark.parametrize("name", ["circle", "road"])
def test_the_twins_winner_is_never_worse_than_member_0_and_a_winner_is_handed_over(name, n_members, budget):
    options, mpa, prob, seeds = sec.case(name)
    Hp = options.Hp
    recs, winners, costs = sec.twin(name, n_members, budget)
    single = sec.twin(name, 1, budget)[0]
    for s in range(len(seeds)):
        w = int(winners[s])
        if np.isfinite(costs[:, s]).any():
            assert int(recs[s]["status"]) == 0 and float(recs[s]["path_nodes"][Hp][4]) == costs[w, s] == costs[:, s].min()
            assert w == int(np.argmin(costs[:, s]))  # (argmin returns the first minimum: the lowest index wins a tie)
        else:
            assert w == 0 and int(recs[s]["status"]) == 1
        if not prob["preds"][s]:
            # no predecessors: member 0 plans the single-stream step's problem, and the winner is at least as cheap
            assert costs[0, s] == (float(single[s]["path_nodes"][Hp][4]) if int(single[s]["status"]) == 0 else np.inf)
            assert costs[w, s] <= costs[0, s]
    # what the GPU parity test relies on: the areas of a member other than 0 are handed to a successor
    assert len(prob["level_sizes"]) >= 3
    assert sec.has_handed_over_winner(prob, recs, winners), (winners.tolist(), recs["status"].tolist())


@pytest.mark.timeout(300)
def test_ensemble_kernels_use_no_scratch_memory_and_spill_no_vector_register():
    """`make` builds sampled_ensemble_kernel.hip and `make resources` lists it with the other kernels; its kernels -- the trees in LDS and
    in HBM -- use no scratch memory and spill no vector register, and a wavefront's registers leave room for four per SIMD."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    with open(os.path.join(CSRC, "Makefile")) as f:
        lines = f.read().splitlines()
    for var in ("SRCS", "RESOURCE_SRCS"):
        listed = [line for line in lines if line.startswith(var)]
        assert listed and "sampled_ensemble_kernel.hip" in listed[0], "%s does not cover sampled_ensemble_kernel.hip" % var
    assert any(line.startswith("HDRS") and "sampled_ensemble.h" in line for line in lines)
    out = subprocess.run(["make", "-s", "-C", CSRC, "resources", "RESOURCE_SRCS=sampled_ensemble_kernel.hip"], capture_output=True, text=True, check=True).stdout
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("vgprs", r" VGPRs: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    for kernel in ("pdmpc_sampled_ensemble_kernel", "pdmpc_sampled_ensemble_kernel_hbm"):
        assert kernel in seen, seen.keys()
        assert seen[kernel]["scratch"] == 0 and seen[kernel]["vgpr_spill"] == 0, (kernel, seen[kernel])
        assert seen[kernel]["vgprs"] <= 128 and seen[kernel]["lds"] == 0, (kernel, seen[kernel])
