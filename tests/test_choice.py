"""The choice among the plans of a batch as data (pdmpc_choice, pdmpc_choose_host) and the explorative step of a sweep
(pdmpc_sweep_explore_build / _problem / _apply) without a GPU: the host twin against the Python restatements of both choices on
closed-loop steps planned by the oracle, crafted costs at the edges of the rounding and of the order of addition, every refusal, and
a sweep of handle-less controllers that leaves every member where its own explorative steps leave it."""
import os

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.backend import BackendError, Choice, choose_host_call
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.distributed import weak_components
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeSweep

from test_native_controller import assert_same_problem
from test_sweep import ERR_CAPACITY, ERR_INVALID, HP, _bits, assert_same_state, distance_members, reachable_members, road

OK, EXHAUSTED, ARENA_OVERFLOW, ERR_HIP = 0, 1, 2, -3
THREADS = min(os.cpu_count() or 1, 8)


# ---- the two choices as data, restated from the batch (the library builds its own in csrc/step_controller.cpp)


def explorative_choice(batch, picks=()):
    """Graph = weakly connected sub-graph (by smallest vehicle), candidates = instances, cell (g, p) = the slots of instance p whose
    vehicles belong to g, ascending."""
    adj = batch["graph_coupling"]
    n = adj.shape[0]
    labels = weak_components([[j for j in range(n) if adj[i, j] or adj[j, i]] for i in range(n)])
    graphs = sorted(set(labels))
    K = batch["n_instances"]
    cells = [[s for s, (q, v) in enumerate(zip(batch["instance"], batch["vehicle"])) if q == p and labels[v] == g] for g in graphs for p in range(K)]
    return Choice(cells, [K] * len(graphs), picks), labels, graphs


def optimal_choice(batch, picks=()):
    """Graph = vehicle, candidates = instances, cell (v, p) = v's slot of instance p, then the others' by ascending vehicle."""
    K = batch["n_instances"]
    n = len(batch["vehicle"]) // K
    slot = {(p, v): s for s, (p, v) in enumerate(zip(batch["instance"], batch["vehicle"]))}
    cells = [[slot[(p, v)]] + [slot[(p, j)] for j in range(n) if j != v] for v in range(n) for p in range(K)]
    return Choice(cells, [K] * n, picks)


def lean(records, Hp):
    return np.asarray(records["status"], dtype=np.int32), np.ascontiguousarray(records["path_nodes"][:, Hp, 4])


def status_of(call):
    with pytest.raises(BackendError) as e:
        call()
    return e.value.status


# ---- 1. the host twin against the Python restatements


def test_host_twin_is_the_explorative_choice_on_closed_loop_steps():
    from oracle import oracle
    from pdmpc.explorative import choose_solution, explore_step
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=12, Hp=HP, max_nodes=1 << 30)
    sc = commonroad_scenario(options, seed=5)
    mpa = get_mpa(options)
    K = 4
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    seen = {"graphs": 0, "other": 0}

    def plan_batch(batch):
        recs, _ = oracle.plan_step(options, mpa, batch, n_threads=THREADS)
        want, cost = choose_solution(batch, recs, options.Hp)
        choice, labels, graphs = explorative_choice(batch)
        chosen, cell_cost = choose_host_call(*lean(recs, options.Hp), choice)
        assert chosen.tolist() == [want[g] for g in graphs]
        assert np.array_equal(_bits(cell_cost.reshape(len(graphs), K).T), _bits(cost))
        seen["graphs"] += len(graphs)
        seen["other"] += sum(1 for c in chosen if c != 0)
        return recs

    for _ in range(4):
        explore_step(py, plan_batch, K)
    assert seen["graphs"] > 4 and seen["other"] > 0


@pytest.mark.parametrize("scenario", ["circle", "road"])
def test_host_twin_is_the_optimal_priority_choice_on_closed_loop_steps(scenario):
    from oracle import oracle
    from pdmpc.optimal import choose_from_costs, optimal_step
    from pdmpc.road_network import boundary_provider, commonroad_scenario
    from pdmpc.scenario import circle_scenario

    if scenario == "circle":
        options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=HP, max_nodes=1 << 30)
        sc, coupling, boundary = circle_scenario(options), "full", None
    else:
        options = Config(scenario_type=ScenarioType.commonroad, amount=6, Hp=HP, max_nodes=1 << 30)
        sc = commonroad_scenario(options, seed=1)
        coupling, boundary = "distance", boundary_provider(sc)
    mpa = get_mpa(options)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling=coupling, boundary_provider=boundary)
    n = options.amount

    def plan_batch(batch):
        recs, _ = oracle.plan_step(options, mpa, batch, n_threads=THREADS)
        K = batch["n_instances"]
        st, fc = lean(recs, options.Hp)
        val = np.zeros((K, n))
        for s, (p, v) in enumerate(zip(batch["instance"], batch["vehicle"])):
            val[p, v] = fc[s] if st[s] == OK else np.inf
        want, cost = choose_from_costs(val)
        chosen, cell_cost = choose_host_call(st, fc, optimal_choice(batch))
        assert chosen.tolist() == want
        assert np.array_equal(_bits(cell_cost.reshape(n, K)), _bits(cost))
        return recs

    for _ in range(2):
        optimal_step(py, plan_batch, 1000)


# ---- 2. crafted inputs


def half_way_sum():
    """Two addends whose double sum v makes v * 1e8 a double exactly half-way between two integers, the lower one even, and two more
    with the lower one odd: round-half-even goes down for the first pair and up for the second."""
    rng = np.random.default_rng(11)
    found = {}
    for _ in range(200000):
        k = int(rng.integers(1, 1 << 20))
        v = (k + 0.5) / 1e8
        if v * 1e8 != k + 0.5:
            continue
        a = float(rng.uniform(0, v))
        b = v - a
        if a + b == v and k % 2 not in found:
            found[k % 2] = (a, b, k)
        if len(found) == 2:
            return found
    pytest.fail("no sum found whose multiple of 1e8 lies half-way between two integers")


def test_sums_that_differ_below_the_rounding_keep_the_first_candidate():
    cost = [1.0, 1.0 - 1e-9, 0.5, 0.5 - 2e-9]  # the second candidate is the smaller one before the rounding
    assert cost[1] + cost[3] < cost[0] + cost[2]
    chosen, cell_cost = choose_host_call([OK] * 4, cost, Choice([[0, 2], [1, 3]], [2]))
    assert chosen.tolist() == [0] and cell_cost.tolist() == [1.5, 1.5]
    # ... and the second one wins as soon as it is smaller by more than the rounding
    chosen, _ = choose_host_call([OK] * 4, [1.0, 1.0 - 2e-8, 0.5, 0.5], Choice([[0, 2], [1, 3]], [2]))
    assert chosen.tolist() == [1]


def test_a_sum_half_way_between_two_multiples_rounds_to_the_even_one():
    found = half_way_sum()
    for parity, (a, b, k) in found.items():
        _, cell_cost = choose_host_call([OK, OK], [a, b], Choice([[0, 1]], [1]))
        even = k if parity == 0 else k + 1
        assert cell_cost[0] == even / 1e8, (a, b, k)
        assert _bits(cell_cost)[0] == _bits([np.rint((a + b) * 1e8) / 1e8])[0]


def test_exhausted_plans_cost_infinity_and_all_infinite_candidates_give_the_first():
    chosen, cell_cost = choose_host_call([OK, EXHAUSTED, OK, OK], [1.0, 0.25, 3.0, 4.0], Choice([[0, 1], [2], [3]], [3]))
    assert chosen.tolist() == [1] and np.isinf(cell_cost[0]) and cell_cost[1:].tolist() == [3.0, 4.0]
    chosen, cell_cost = choose_host_call([EXHAUSTED] * 3, [1.0, 2.0, 3.0], Choice([[0], [1], [2]], [3]))
    assert chosen.tolist() == [0] and np.isinf(cell_cost).all()
    # the minimum at the last candidate; a graph of one candidate; an empty cell costs 0
    chosen, cell_cost = choose_host_call([OK] * 4, [4.0, 3.0, 2.0, 1.0], Choice([[0], [1], [2], [3], [0, 3], []], [4, 1, 1]))
    assert chosen.tolist() == [3, 0, 0] and cell_cost.tolist() == [4.0, 3.0, 2.0, 1.0, 5.0, 0.0]


def test_the_order_of_a_cells_list_is_the_order_of_addition():
    cost = [1e16, 1.0, -1e16, 1.0]
    forward, backward = [0, 1, 2, 3], [3, 2, 1, 0]
    _, c = choose_host_call([OK] * 4, cost, Choice([forward, backward], [2]))
    assert c[0] == np.rint(((((0.0 + 1e16) + 1.0) - 1e16) + 1.0) * 1e8) / 1e8 == 1.0
    assert c[1] == np.rint(((((0.0 + 1.0) - 1e16) + 1.0) + 1e16) * 1e8) / 1e8 == 0.0
    assert _bits(c)[0] != _bits(c)[1], "the reversed list adds to the same bits: the test would not notice a sorted or reversed addition"


def test_an_error_status_is_refused_also_where_no_cell_lists_it():
    choice = Choice([[0], [1]], [2])
    for bad in (ARENA_OVERFLOW, ERR_HIP, -7):
        assert status_of(lambda: choose_host_call([OK, OK, bad], [1.0, 2.0, 3.0], choice)) == ERR_HIP
        assert status_of(lambda: choose_host_call([bad, OK, OK], [1.0, 2.0, 3.0], choice)) == ERR_HIP


def test_every_validation_refusal():
    st, fc = [OK] * 4, [1.0, 2.0, 3.0, 4.0]

    def refused(choice, **patch):
        for key, value in patch.items():
            setattr(choice, key, np.ascontiguousarray(value, dtype=np.int32))
        return status_of(lambda: choose_host_call(st, fc, choice)) == ERR_INVALID

    good = lambda: Choice([[0, 1], [2], [3]], [2, 1], [(0, [0, 2]), (-1, [3]), (1, [1])])  # noqa: E731
    chosen, _ = choose_host_call(st, fc, good())
    assert chosen.tolist() == [0, 0]
    assert refused(good(), cell_offset=[0, 2, 1, 4])       # cell offsets that decrease
    assert refused(good(), cell_offset=[-1, 2, 3, 4])      # ... that start below 0
    assert refused(good(), cell_slot=[0, 1, 2, 4, 0])      # a slot beyond the batch
    assert refused(good(), cell_slot=[0, -1, 2, 3, 0])     # a negative slot
    assert refused(good(), graph_offset=[0, 3, 2])         # graph offsets that decrease
    assert refused(good(), graph_offset=[0, 2, 4])         # candidates beyond the cells
    assert refused(good(), pick_graph=[0, -2, 1, 0])       # pick_graph below -1
    assert refused(good(), pick_graph=[0, -1, 2, 0])       # pick_graph beyond the graphs
    assert refused(good(), pick_offset=[0, 2, 1, 4])       # pick offsets that decrease
    assert refused(good(), pick_offset=[0, 1, 3, 4])       # a pick with fewer slots than its graph has candidates
    assert refused(good(), pick_graph=[1, -1, 1, 0])       # ... with more
    assert refused(good(), pick_graph=[-1, -1, 1, 0])      # a follow-own pick with two slots
    assert refused(good(), pick_slot=[0, 2, 4, 1, 0])      # a picked slot beyond the batch
    assert refused(Choice([[0], [1]], [2, 0], [(1, [])]))  # a pick of a graph without candidates
    bad = good()
    bad.n_cells = -1
    assert refused(bad)
    with pytest.raises(BackendError):
        choose_host_call(st[:2], fc[:2], good())           # the same lists on a smaller batch: slots 2 and 3 lie outside


# ---- 3. the explorative step of a sweep against solo members, on the host


def exhaust(member, k, problem, records):
    """The vehicle whose search the member's scenario lets run empty at step k does so in the instances 0 and 2 of the batch."""
    v = member.force(k)
    if v is not None:
        for s, (p, veh) in enumerate(zip(problem["instance"], problem["vehicle"])):
            if veh == v and p % 2 == 0:
                records[s]["status"] = EXHAUSTED


def solo_explorative_step(member, c, k, n_perm, follow_own=False):
    """One explorative step of a controller without a handle, planned by the oracle -> (its batch, its records, chosen, cost table)."""
    from oracle import oracle

    c.explore_build(n_perm, seed=k)
    p = c.explore_problem()
    recs, _ = oracle.plan_step(member.options, member.mpa, p, n_threads=THREADS)
    exhaust(member, k, p, recs)
    chosen, cost = c.explore_choose(recs)
    slot = {(q, v): s for s, (q, v) in enumerate(zip(p["instance"], p["vehicle"]))}
    c.apply(recs[[slot[(0 if follow_own else int(chosen[v]), v)] for v in c.problem()["order"]]])
    return p, recs, chosen, cost


def assert_concatenated_batch(sp, problems, ctx):
    """The sweep's batch is the members' batches one after the other, predecessor slots shifted by the member's first slot."""
    want = {"iters": [], "preds": [], "fallback": [], "member": [], "instance": [], "vehicle": [], "levels": []}
    for m, p in enumerate(problems):
        first = len(want["iters"])
        want["iters"] += p["iters"]
        want["fallback"] += p["fallback"]
        want["preds"] += [[first + q for q in pr] for pr in p["preds"]]
        want["member"] += [m] * len(p["iters"])
        for key in ("instance", "vehicle", "levels"):
            want[key] += p[key]
    for key in ("member", "instance", "vehicle", "levels"):
        assert sp[key] == want[key], (ctx, key)
    same = {"order": [], "level_sizes": []}
    assert_same_problem(dict(want, **same), dict(sp, **same), ctx)


def assert_same_choice(a, b, ctx):
    (chosen_a, cost_a), (chosen_b, cost_b) = a, b
    assert chosen_a.tolist() == chosen_b.tolist(), ctx
    assert cost_a.shape == cost_b.shape and np.array_equal(_bits(cost_a), _bits(cost_b)), ctx


def explorative_sweep_against_solo(members, n_perm, n_steps, follow_own=None):
    """follow_own: index of a member that applies the plans of its own prioritization; its state twin is a PLAIN controller."""
    from oracle import oracle

    solo = [m.make() for m in members]
    swept = [m.make() for m in members]
    plain = members[follow_own].make() if follow_own is not None else None
    if follow_own is not None:
        swept[follow_own].explore_follow_own(True)
    sweep = NativeSweep(swept)
    other = 0
    try:
        for k in range(1, n_steps + 1):
            steps = [solo_explorative_step(m, c, k, n_perm, i == follow_own) for i, (m, c) in enumerate(zip(members, solo))]
            if plain is not None:
                plain.build_step()
                recs, _ = oracle.plan_step(members[follow_own].options, members[follow_own].mpa, plain.problem())
                plain.apply(recs)
            sweep.explore_build(n_perm)
            assert_concatenated_batch(sweep.explore_problem(), [s[0] for s in steps], "step %d" % k)
            for c, s in zip(swept, steps):  # ... and every member's own batch is the one its own build leaves
                q = c.explore_problem()
                assert_same_problem(q, s[0], "step %d, a member's own batch" % k)
                assert q["instance"] == s[0]["instance"] and q["vehicle"] == s[0]["vehicle"]
            sweep.explore_apply(np.concatenate([s[1] for s in steps]))
            for i, (a, b, s) in enumerate(zip(solo, swept, steps)):
                ctx = "step %d member %d" % (k, i)
                assert_same_state(a.state(), b.state(), ctx)
                assert a.seeds() == b.seeds(), ctx
                assert_same_choice(b.explore_result(), s[2:], ctx)
                other += int((s[2] != 0).sum())
            if plain is not None:
                assert_same_state(plain.state(), swept[follow_own].state(), "step %d, follow-own against the plain step" % k)
        assert other > 0, "no member ever preferred another prioritization"
        # a member alone after the sweep goes on like its twin, explorative and plain
        sweep.close()
        for k in range(n_steps + 1, n_steps + 3):
            for i, (m, a, b) in enumerate(zip(members, solo, swept)):
                ctx = "alone after the sweep, step %d member %d" % (k, i)
                sa, sb = solo_explorative_step(m, a, k, n_perm, i == follow_own), solo_explorative_step(m, b, k, n_perm, i == follow_own)
                assert_same_problem(sa[0], sb[0], ctx)
                assert_same_choice(sa[2:], sb[2:], ctx)
                assert_same_state(a.state(), b.state(), ctx)
    finally:
        sweep.close()
        for c in solo + swept + ([plain] if plain is not None else []):
            c.close()


def test_explorative_sweep_leaves_the_members_where_their_own_steps_do():
    explorative_sweep_against_solo(distance_members(), 3, 8)


def test_explorative_sweep_with_reachable_set_coupling_and_a_member_that_follows_its_own_prioritization():
    members = reachable_members()
    explorative_sweep_against_solo(members, 3, 8, follow_own=len(members) - 1)


def test_a_sweep_alternates_plain_and_explorative_steps():
    from oracle import oracle

    members = [road(8, 1, "distance"), road(6, 2, "distance", priority_strategy="coloring", max_num_CLs=2)]
    solo = [m.make() for m in members]
    swept = [m.make() for m in members]
    sweep = NativeSweep(swept)
    try:
        for k in range(1, 5):
            if k % 2:
                steps = [solo_explorative_step(m, c, k, 4) for m, c in zip(members, solo)]
                sweep.explore_build(4)
                sweep.explore_apply(np.concatenate([s[1] for s in steps]))
            else:
                recs = []
                for m, c in zip(members, solo):
                    c.build_step()
                    recs.append(oracle.plan_step(m.options, m.mpa, c.problem())[0])
                    c.apply(recs[-1])
                sweep.build()
                sweep.apply(np.concatenate(recs))
            for a, b in zip(solo, swept):
                assert_same_state(a.state(), b.state(), "step %d" % k)
                assert a.seeds() == b.seeds()
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()


def test_seeds_are_those_of_whichever_was_built_last_the_step_or_the_batch():
    """The step and the batch of prioritizations each carry their own seeds; seeds() hands out those of the problem built last: one entry
    per slot of that problem, time_step + vehicle + 1 (1-based vehicle index), whether a step follows a batch or a batch a step."""
    from pdmpc.native_controller import NativeController
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=3, Hp=HP, max_nodes=1 << 30)
    nat = NativeController(options, circle_scenario(options), get_mpa(options), None, coupling="full", optimizer="sampled")
    try:
        def assert_seeds(vehicle_of_slot, n_slots, what):
            k = nat.state()["k"]
            assert len(vehicle_of_slot) == n_slots, what
            assert nat.seeds() == [k + v + 1 for v in vehicle_of_slot], what

        nat.build_step()
        assert_seeds(nat.problem()["order"], 3, "first step")
        nat.explore_build(2, 7)
        batch = nat.explore_problem()
        assert max(batch["levels"]) > 1
        assert_seeds(batch["vehicle"], 2 * 3, "explorative batch")
        nat.build_step()
        assert_seeds(nat.problem()["order"], 3, "step behind a batch")
        K = nat.optimal_build(100)
        assert K > 1
        assert_seeds(nat.optimal_problem()["vehicle"], K * 3, "optimal-priority batch")
    finally:
        nat.close()


def test_every_refusal_of_the_explorative_sweep_leaves_the_members_untouched():
    from oracle import oracle

    members = [road(6, 1, "distance"), road(5, 2, "distance")]
    cs = [m.make() for m in members]
    sweep = NativeSweep(cs)

    def status(call):
        with pytest.raises(BackendError) as e:
            call()
        return e.value.status

    try:
        before = [c.state() for c in cs]
        assert status(lambda: sweep.explore_build(0)) == ERR_INVALID             # n_perm < 1
        assert status(lambda: sweep.explore_build(-3)) == ERR_INVALID
        assert status(lambda: sweep.explore_step(3)) == ERR_INVALID              # no handle
        assert status(lambda: sweep.explore_run(3, 2)) == ERR_INVALID
        assert status(lambda: sweep.explore_problem()) == ERR_INVALID            # nothing built
        assert status(lambda: sweep._check(sweep.L.pdmpc_sweep_explore_apply(sweep.s, None), "pdmpc_sweep_explore_apply")) == ERR_INVALID  # no records
        for m in cs:
            m.n_perm = 3
        assert status(lambda: sweep.explore_apply(abi.out_array(33))) == ERR_INVALID  # apply before build
        for c, b in zip(cs, before):
            assert_same_state(c.state(), b, "after the refusals")
            assert c.state()["k"] == 0
        # a sweep that broke refuses the explorative calls as well: records with an error status break it in explore_apply
        sweep.explore_build(3)
        p = sweep.explore_problem()
        recs = np.concatenate([oracle.plan_step(m.options, m.mpa, c.explore_problem(), n_threads=THREADS)[0] for m, c in zip(members, cs)])
        assert len(recs) == len(p["member"]) == 33
        recs[len(recs) - 1]["status"] = ARENA_OVERFLOW
        assert status(lambda: sweep.explore_apply(recs)) == ERR_HIP
        state = [c.state() for c in cs]
        assert status(lambda: sweep.explore_build(3)) == ERR_INVALID
        assert status(lambda: sweep.explore_apply(recs)) == ERR_INVALID
        assert status(lambda: sweep.build()) == ERR_INVALID
        for c, b in zip(cs, state):
            assert_same_state(c.state(), b, "a broken sweep")
    finally:
        sweep.close()
        for c in cs:
            c.close()
    assert ERR_CAPACITY == -4  # (the capacity refusal needs a handle: tests/test_gpu_choice.py)


# ---- 9. what the compiler made of the kernels (hipcc cross-compiles: no GPU needed)


def test_choice_kernels_use_no_scratch_memory_and_spill_nothing():
    import re
    import shutil
    import subprocess

    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "p-dmpc_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "resources", "RESOURCE_SRCS=choice_kernel.hip"], capture_output=True, text=True, check=True).stdout
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    for kernel in ("pdmpc_choice_cells_kernel", "pdmpc_choice_gather_kernel"):
        assert kernel in seen, sorted(seen)
        assert seen[kernel] == {"scratch": 0, "vgpr_spill": 0, "sgpr_spill": 0}, (kernel, seen[kernel])
