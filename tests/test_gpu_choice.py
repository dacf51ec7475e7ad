"""The choice among the plans of a batch on the MI355X (csrc/choice_kernel.hip: pdmpc_choose_resident, pdmpc_plan_step_chosen,
pdmpc_controller_set_device_choice, pdmpc_sweep_explore_step): the device choice against its host twin on synthetic
records at every size where the kernels take another path, pdmpc_plan_step_chosen against pdmpc_plan_step plus the twin (also across
an arena regrow), closed loops with the choice on the device against the same loops with the choice on the host, members of an
explorative sweep against members stepped alone, and a sweep's kept records against the oracle's."""
import copy
import os

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.backend import BackendError, Choice, Handle, choose_host_call
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeSweep

from test_choice import ERR_HIP, EXHAUSTED, OK, ARENA_OVERFLOW, assert_same_choice, explorative_choice, half_way_sum, lean
from test_gpu_parity import assert_records_equal
from test_gpu_sweep import shared_handle
from test_sweep import ERR_CAPACITY, ERR_INVALID, HP, _bits, assert_same_state, circle, distance_members, reachable_members, road

pytestmark = pytest.mark.gpu

N_SYNTH = 600  # records of the synthetic batch: more than two workgroups' worth of CUs are picked from it


# ---- 4. pdmpc_choose_resident on synthetic records


@pytest.fixture(scope="module")
def synth():
    options = Config(scenario_type=ScenarioType.commonroad, Hp=HP, max_vehicles=N_SYNTH + 8, max_nodes=1 << 10)
    h = Handle(options)
    yield h
    h.close()


def records(rng, n=N_SYNTH):
    """n records of distinct payload bytes, every status OK and a final cost that is a multiple of 2^-20 (sums of them are exact)."""
    recs = abi.out_array(n)
    raw = recs.view(np.uint8).reshape(n, -1)
    raw[:] = rng.integers(0, 256, raw.shape, dtype=np.uint8)
    raw[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)  # (no two records alike)
    recs["status"] = OK
    recs["path_nodes"][:, HP, 4] = rng.integers(1 << 20, 1 << 24, n) / float(1 << 20)
    return recs


def on_device(h, recs, choice, n=None):
    """The records made resident through a torch device tensor, then the choice on the device."""
    import torch

    n = len(recs) if n is None else n
    t = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    h.import_results(0, len(recs), t.data_ptr())
    return h.choose_resident(n, choice)


def assert_device_is_host(h, recs, choice, ctx):
    chosen, cost, picks = on_device(h, recs, choice)
    want_chosen, want_cost = choose_host_call(*lean(recs, HP), choice)
    assert chosen.tolist() == want_chosen.tolist(), ctx
    assert np.array_equal(_bits(cost), _bits(want_cost)), ctx
    go = choice.graph_offset
    for i in range(choice.n_picks):
        g = int(choice.pick_graph[i])
        slot = int(choice.pick_slot[choice.pick_offset[i] + (0 if g < 0 else want_chosen[g])])
        assert picks[i].tobytes() == recs[slot].tobytes(), (ctx, i)
    assert len(picks) == choice.n_picks and len(go) == choice.n_graphs + 1
    return chosen, cost, picks


@pytest.mark.parametrize("cands", [1, 2, 63, 64, 65, 130])
def test_one_graph_at_every_candidate_count(synth, cands):
    rng = np.random.default_rng(cands)
    recs = records(rng)
    slots = rng.permutation(N_SYNTH)
    cells = [[int(slots[c])] for c in range(cands)]
    pick = (0, [int(s) for s in slots[200 : 200 + cands]])
    for n_picks in (0, 1, 300):  # none, one, more picks than the device has CUs
        assert_device_is_host(synth, recs, Choice(cells, [cands], [pick] * n_picks), "%d candidates, %d picks" % (cands, n_picks))
    # the minimum at the last candidate
    recs["path_nodes"][slots[cands - 1], HP, 4] = 0.5
    chosen, _, _ = assert_device_is_host(synth, recs, Choice(cells, [cands], [pick]), "minimum at the last of %d" % cands)
    assert chosen.tolist() == [cands - 1]
    # every candidate infinitely expensive: the first
    recs["status"][slots[:cands]] = EXHAUSTED
    chosen, cost, _ = assert_device_is_host(synth, recs, Choice(cells, [cands], [pick]), "all of %d infinite" % cands)
    assert chosen.tolist() == [0] and np.isinf(cost).all()
    assert synth.choice_kernel_ms() > 0.0


def test_many_graphs_long_cells_and_cells_of_no_graph(synth):
    rng = np.random.default_rng(7)
    recs = records(rng)
    sizes = [1, 2, 63, 64, 65, 130, 1, 64]
    cells, picks = [], []
    for g, size in enumerate(sizes):
        for c in range(size):
            addends = 1 if (g + c) % 3 else int(rng.integers(65, 140))  # one addend, or more than a wavefront has lanes
            cells.append([int(s) for s in rng.integers(0, N_SYNTH, addends)])
        for _ in range(40):
            picks.append((g, [int(s) for s in rng.integers(0, N_SYNTH, size)]))
        picks.append((-1, [int(rng.integers(0, N_SYNTH))]))  # follow-own: the single listed slot
    assert len(picks) > 256
    cells += [[5, 6, 7], [], [599]]  # behind the last graph: cells that are summed but belong to no graph
    recs["status"][rng.integers(0, N_SYNTH, 25)] = EXHAUSTED
    assert_device_is_host(synth, recs, Choice(cells, sizes, picks), "graphs of every size")
    # ... and with cells in front of the first graph as well
    offset = np.concatenate([[3], 3 + np.cumsum(sizes)])
    front = [[1], [2, 3], [4]] + cells
    moved = [(g, sl) for g, sl in picks]
    assert_device_is_host(synth, recs, Choice(front, graph_offset=offset, picks=moved), "cells in front of the graphs")


@pytest.mark.parametrize("first,second,cands", [(3, 67, 130), (64, 65, 130), (0, 64, 65), (63, 127, 128)])
def test_equal_minima_give_the_smaller_index_also_across_the_stride(synth, first, second, cands):
    rng = np.random.default_rng(first)
    recs = records(rng)
    cells = [[c] for c in range(cands)]
    recs["path_nodes"][[first, second], HP, 4] = 0.25
    chosen, cost, _ = assert_device_is_host(synth, recs, Choice(cells, [cands], [(0, list(range(100, 100 + cands)))]), "tie")
    assert chosen.tolist() == [first] and cost[first] == cost[second] == 0.25


def test_rounding_on_the_device_is_the_hosts(synth):
    rng = np.random.default_rng(3)
    recs = records(rng)
    found = half_way_sum()
    for parity, (a, b, k) in found.items():
        recs["path_nodes"][[10, 11], HP, 4] = (a, b)
        # candidates: the half-way sum, the even neighbour it must round to, the odd one it must not
        even = k if parity == 0 else k + 1
        recs["path_nodes"][[12, 13], HP, 4] = (even / 1e8, (2 * k + 1 - even) / 1e8)
        _, cost, _ = assert_device_is_host(synth, recs, Choice([[10, 11], [12], [13]], [3]), "half-way, parity %d" % parity)
        assert cost[0] == even / 1e8
    # sums that differ below the rounding: the first candidate; an order of addition that matters
    recs["path_nodes"][[20, 21, 22, 23], HP, 4] = (1.0, 1.0 - 1e-9, 0.5, 0.5 - 2e-9)
    chosen, _, _ = assert_device_is_host(synth, recs, Choice([[20, 22], [21, 23]], [2]), "below the rounding")
    assert chosen.tolist() == [0]
    recs["path_nodes"][[30, 31, 32, 33], HP, 4] = (1e16, 1.0, -1e16, 1.0)
    _, cost, _ = assert_device_is_host(synth, recs, Choice([[30, 31, 32, 33], [33, 32, 31, 30]], [2]), "order of addition")
    assert cost.tolist() == [1.0, 0.0]


def test_a_status_that_is_no_planning_result_is_counted_wherever_it_is(synth):
    rng = np.random.default_rng(5)
    choice = Choice([[0], [1]], [2], [(0, [0, 1])])
    for bad in (ARENA_OVERFLOW, ERR_HIP, -7):
        for where in (599, 2, 64, 0):  # in records that no cell lists (the last of the batch, ...) and in one that a cell lists
            recs = records(rng)
            recs["status"][where] = bad
            with pytest.raises(BackendError) as e:
                on_device(synth, recs, choice)
            assert e.value.status == ERR_HIP, (bad, where)
    # outside the n records the call is about it does not count; and the handle goes on
    recs = records(rng)
    recs["status"][300] = ARENA_OVERFLOW
    chosen, _, picks = on_device(synth, recs, choice, n=300)
    assert chosen.tolist() == [int(np.argmin(recs["path_nodes"][:2, HP, 4]))] and picks[0].tobytes() == recs[chosen[0]].tobytes()
    # refusals come before anything is launched
    with pytest.raises(BackendError) as e:
        on_device(synth, recs, Choice([[0], [N_SYNTH + 8]], [2]))
    assert e.value.status == ERR_INVALID


# ---- 5. pdmpc_plan_step_chosen against pdmpc_plan_step plus the host twin


def explorative_batch(optimizer, max_nodes):
    """A real explorative batch (12 vehicles x 3 prioritizations) after three closed-loop steps, with picks of every vehicle."""
    from pdmpc.explorative import build_exploration_batch
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=12, Hp=HP, max_vehicles=36, max_nodes=1 << 17)
    mpa = get_mpa(options)
    sc = commonroad_scenario(options, seed=2)
    big = Handle(options)
    big.upload_mpa(mpa)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    for _ in range(3):
        ctl.step(plan_step=lambda prob: _infos(big.plan_step(prob["iters"], prob["preds"], [f or [] for f in prob["fallback"]]), options.Hp))
    batch = build_exploration_batch(ctl, 3, seed=ctl.k + 1)
    seeds = [ctl.k + v + 1 for v in batch["vehicle"]] if optimizer == "sampled" else None  # time step + vehicle index
    small_options = copy.copy(options)
    small_options.max_nodes = max_nodes
    return options, mpa, batch, seeds, big, small_options


def _infos(recs, Hp):
    from pdmpc.iteration_data import info_from_record

    return [info_from_record(recs[i], Hp) for i in range(len(recs))]


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
def test_plan_step_chosen_is_plan_step_and_the_twin(optimizer):
    options, mpa, batch, seeds, h, small_options = explorative_batch(optimizer, 64)
    small = None
    try:
        fb = [f or [] for f in batch["fallback"]]
        slot = {(p, v): s for s, (p, v) in enumerate(zip(batch["instance"], batch["vehicle"]))}
        _, labels, graphs = explorative_choice(batch)
        picks = [(graphs.index(labels[v]), [slot[(p, v)] for p in range(3)]) for v in range(12)] + [(-1, [slot[(0, 5)]])]
        choice, _, _ = explorative_choice(batch, picks)

        def plan(handle, call):
            if seeds is not None:
                handle.set_step_seeds(seeds)
            return call(handle)

        recs = plan(h, lambda q: q.plan_step(batch["iters"], batch["preds"], fb))
        want_chosen, want_cost = choose_host_call(*lean(recs, options.Hp), choice)
        handles = [h]
        if optimizer == "graph_search":  # (the sampled optimizer has no arenas to outgrow)
            small = Handle(small_options)
            small.upload_mpa(mpa)
            handles.append(small)
        for q in handles:
            chosen, cost, kept = plan(q, lambda q: q.plan_step_chosen(batch["iters"], batch["preds"], fb, choice))
            assert chosen.tolist() == want_chosen.tolist() and np.array_equal(_bits(cost), _bits(want_cost))
            for i, (g, slots) in enumerate(picks):
                assert kept[i].tobytes() == recs[slots[0 if g < 0 else want_chosen[g]]].tobytes(), i
            assert q.choice_kernel_ms() > 0.0
        if small is not None:
            nodes, regrows = small.arena_nodes()
            assert regrows >= 1 and nodes > 64, "the small handle's first launch did not overflow: the regrow path was not taken"
        # a bad description is refused before the pack: the resident batch is still the one planned last
        with pytest.raises(BackendError) as e:
            h.plan_step_chosen(batch["iters"], batch["preds"], fb, Choice([[0], [36]], [2]))
        assert e.value.status == ERR_INVALID
        chosen, cost, _ = h.choose_resident(36, choice)
        assert chosen.tolist() == want_chosen.tolist() and np.array_equal(_bits(cost), _bits(want_cost))
    finally:
        h.close()
        if small is not None:
            small.close()


# ---- 6. solo closed loops with the choice on the device


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
@pytest.mark.parametrize("follow_own", [False, True], ids=["chosen", "follow_own"])
def test_explorative_closed_loop_with_the_choice_on_the_device(optimizer, follow_own):
    m = road(12, 2, "distance", max_vehicles=64, max_nodes=1 << 17)
    h, mpa, _ = shared_handle(64)
    host, dev = (m.make(h, mpa, optimizer=optimizer) for _ in range(2))
    dev.set_device_choice(True)
    other = 0
    try:
        for c in (host, dev):
            c.explore_follow_own(follow_own)
        for k in range(8):
            host.explore_run(3, 1)
            dev.explore_run(3, 1)
            assert dev.last_timing()["wait_and_read_back"] > 0
            assert_same_state(host.state(), dev.state(), "step %d" % (k + 1))
            assert_same_choice(host.explore_result(), dev.explore_result(), "step %d" % (k + 1))
            assert host.records().tobytes() == dev.records().tobytes(), k
            assert host.seeds() == dev.seeds()
            other += int((dev.explore_result()[0] != 0).sum())
        assert other > 0
        assert h.choice_kernel_ms() > 0.0
    finally:
        host.close()
        dev.close()
        h.close()


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
def test_optimal_priority_closed_loop_with_the_choice_on_the_device(optimizer):
    m = circle("full", max_vehicles=96, max_nodes=1 << 17)
    h, mpa, _ = shared_handle(96)
    host, dev = (m.make(h, mpa, optimizer=optimizer) for _ in range(2))
    dev.set_device_choice(True)
    try:
        for k in range(8):
            host.optimal_run(24, 1)
            dev.optimal_run(24, 1)
            assert_same_state(host.state(), dev.state(), "step %d" % (k + 1))
            assert_same_choice(host.optimal_result(), dev.optimal_result(), "step %d" % (k + 1))
            assert host.optimal_result()[1].shape == (4, 24)
            assert host.records().tobytes() == dev.records().tobytes(), k
    finally:
        host.close()
        dev.close()
        h.close()


# ---- 7. the sweep property on the device


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
@pytest.mark.parametrize("members", [distance_members, reachable_members], ids=["distance", "reachable_sets"])
def test_members_of_an_explorative_sweep_end_every_step_where_they_end_it_alone(members, optimizer):
    members = members(max_vehicles=256, max_nodes=1 << 17)
    h, mpa, _ = shared_handle(256)
    solo = [m.make(h, mpa, optimizer=optimizer) for m in members]
    swept = [m.make(h, mpa, optimizer=optimizer) for m in members]
    for c in (solo[-1], swept[-1]):  # the last member applies the plans of its own prioritization
        c.explore_follow_own(True)
    sweep = NativeSweep(swept, h)
    other = 0
    try:
        for k in range(1, 9):
            for c in solo:
                c.explore_step(3)
            together = sweep.explore_step(3)
            for i, (a, b) in enumerate(zip(solo, swept)):
                ctx = "step %d member %d" % (k, i)
                assert a.records().tobytes() == together[i].tobytes() == b.records().tobytes(), ctx
                assert_same_state(a.state(), b.state(), ctx)
                assert_same_choice(a.explore_result(), b.explore_result(), ctx)
                assert a.seeds() == b.seeds(), ctx
                other += int((b.explore_result()[0] != 0).sum())
        assert other > 0
        assert h.choice_kernel_ms() > 0.0
        t = sweep.last_timing()
        assert t["build"] > 0 and t["wait_and_read_back"] > 0
        # plain and explorative steps alternate; then a member taken out of the sweep goes on alone like its twin
        plain = sweep.step()
        for i, c in enumerate(solo):
            assert c.step().tobytes() == plain[i].tobytes(), i
        sweep.close()
        for i, (a, b) in enumerate(zip(solo, swept)):
            a.explore_step(3)
            b.explore_step(3)
            assert a.records().tobytes() == b.records().tobytes(), i
            assert_same_state(a.state(), b.state(), "alone after the sweep, member %d" % i)
            assert_same_choice(a.explore_result(), b.explore_result(), "alone after the sweep, member %d" % i)
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
        h.close()


def test_explorative_sweep_refuses_more_plans_than_the_handle_holds():
    members = [road(6, 1, "distance", max_vehicles=24), road(5, 2, "distance", max_vehicles=24)]
    h, mpa, _ = shared_handle(24, max_nodes=1 << 12)
    cs = [m.make(h, mpa) for m in members]
    sweep = NativeSweep(cs, h)
    try:
        for call in (lambda: sweep.explore_step(3), lambda: sweep.explore_build(3), lambda: sweep.explore_run(3, 2)):  # 33 plans > 24
            with pytest.raises(BackendError) as e:
                call()
            assert e.value.status == ERR_CAPACITY
        with pytest.raises(BackendError) as e:
            sweep.explore_step(0)
        assert e.value.status == ERR_INVALID
        assert all(c.state()["k"] == 0 for c in cs)
        sweep.explore_step(2)  # 22 plans fit, and the sweep was not broken by the refusals
        assert all(c.state()["k"] == 1 for c in cs)
    finally:
        sweep.close()
        for c in cs:
            c.close()
        h.close()


# ---- 8. the oracle


def test_kept_records_of_an_explorative_sweep_are_the_oracles_for_the_concatenated_batch():
    from oracle import oracle

    members = [road(20, 1, "distance", max_vehicles=96, max_nodes=1 << 17), road(12, 2, "distance", priority_strategy="coloring", max_num_CLs=2, max_vehicles=96, max_nodes=1 << 17)]
    h, mpa, options = shared_handle(96)
    swept = [m.make(h, mpa) for m in members]
    sweep = NativeSweep(swept, h)
    unbounded = copy.copy(options)
    unbounded.max_nodes = 1 << 30
    try:
        for k in range(1, 3):
            kept = sweep.explore_step(3)
            sweep_batch = sweep.explore_problem()  # (of the step just planned)
            # the oracle plans level by level: the batch's slots sorted by computation level
            level = sweep_batch["levels"]
            order = sorted(range(len(level)), key=lambda s: level[s])
            place = {s: q for q, s in enumerate(order)}
            prob = {
                "iters": [sweep_batch["iters"][s] for s in order],
                "fallback": [sweep_batch["fallback"][s] for s in order],
                "preds": [[place[p] for p in sweep_batch["preds"][s]] for s in order],
                "level_sizes": [sum(1 for lv in level if lv == l) for l in range(1, max(level) + 1)],
            }
            ref, _ = oracle.plan_step(unbounded, mpa, prob, n_threads=min(os.cpu_count() or 1, 16))
            ref = ref[[place[s] for s in range(len(level))]]  # back in the batch's slot order
            first = 0
            for i, c in enumerate(swept):
                n_slots = c.n * 3
                mine = ref[first : first + n_slots]
                chosen, cost = c.explore_result()
                want_chosen, want_cost = c.explore_choose(mine)  # (the member's own host choice on the oracle's records)
                assert_same_choice((chosen, cost), (want_chosen, want_cost), "step %d member %d" % (k, i))
                inst, veh = sweep_batch["instance"][first : first + n_slots], sweep_batch["vehicle"][first : first + n_slots]
                slot = {(p, v): s for s, (p, v) in enumerate(zip(inst, veh))}
                want = mine[[slot[(int(chosen[v]), v)] for v in c.problem()["order"]]]
                assert_records_equal(kept[i], want, "step %d member %d" % (k, i))
                first += n_slots
    finally:
        sweep.close()
        for c in swept:
            c.close()
        h.close()
