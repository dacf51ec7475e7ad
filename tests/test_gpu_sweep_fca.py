"""Sweeps with FCA members on the MI355X (pdmpc_sweep_step / pdmpc_sweep_explore_step with pdmpc_fca_collisions_grouped as the fourth
step-preparation call): members stepped by a sweep end every step byte for byte where members stepped alone on the
same handle end it, with ONE collision assessment per lock-step whatever the number of FCA members, and the sweep's records are the
oracle's for its concatenated problem."""
import copy
import os

import numpy as np
import pytest

from pdmpc.native_controller import NativeSweep

from test_choice import assert_same_choice
from test_fca_grouped import assert_same_priorities, fca_members
from test_gpu_parity import assert_records_equal
from test_gpu_sweep import shared_handle
from test_sweep import assert_same_state, assert_sweep_problem

pytestmark = pytest.mark.gpu


def is_fca(members):
    return [m.kw.get("priority_strategy") == "fca" for m in members]


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
def test_fca_members_of_a_sweep_end_every_step_where_they_end_it_alone(optimizer):
    """three FCA members of 8, 6 and 4 vehicles (the circle with a scenario obstacle of its own) and a colouring member"""
    members = fca_members(max_vehicles=32, max_nodes=1 << 17)
    fca = is_fca(members)
    h, mpa, _ = shared_handle(32)
    solo = [m.make(h, mpa, optimizer=optimizer) for m in members]
    swept = [m.make(h, mpa, optimizer=optimizer) for m in members]
    sweep = NativeSweep(swept, h)
    hits, reordered = 0, 0
    try:
        for k in range(1, 7):
            alone = [c.step() for c in solo]
            together = sweep.step()
            assert sweep.prep_calls() == [0, 0, 0, 1], k
            for i, (a, b) in enumerate(zip(alone, together)):
                ctx = "step %d member %d" % (k, i)
                assert_records_equal(b, a, ctx)
                assert a.tobytes() == b.tobytes(), ctx
                assert_same_state(solo[i].state(), swept[i].state(), ctx)
                assert solo[i].seeds() == swept[i].seeds(), ctx
                hits += assert_same_priorities(solo[i], swept[i], ctx, fca[i])
                reordered += fca[i] and swept[i].priorities()[0] != list(range(1, swept[i].n + 1))
            assert_sweep_problem(sweep.problem(), [c.problem() for c in solo], "step %d" % k)
        assert hits > 0 and reordered > 0
        assert h.fca_kernel_ms() > 0.0
        # a member taken out of the sweep goes on alone like its twin
        sweep.close()
        for i, (a, b) in enumerate(zip(solo, swept)):
            assert a.step().tobytes() == b.step().tobytes(), i
            assert_same_state(a.state(), b.state(), "alone after the sweep, member %d" % i)
            assert_same_priorities(a, b, "alone after the sweep, member %d" % i, fca[i])
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
        h.close()


def test_fca_members_of_an_explorative_sweep_end_every_step_where_they_end_it_alone():
    members = fca_members(max_vehicles=128, max_nodes=1 << 17)
    fca = is_fca(members)
    h, mpa, _ = shared_handle(128)
    solo = [m.make(h, mpa) for m in members]
    swept = [m.make(h, mpa) for m in members]
    sweep = NativeSweep(swept, h)
    hits = 0
    try:
        for k in range(1, 7):
            for c in solo:
                c.explore_step(3)
            together = sweep.explore_step(3)
            assert sweep.prep_calls() == [0, 0, 0, 1], k
            for i, (a, b) in enumerate(zip(solo, swept)):
                ctx = "step %d member %d" % (k, i)
                assert a.records().tobytes() == together[i].tobytes() == b.records().tobytes(), ctx
                assert_same_state(a.state(), b.state(), ctx)
                assert_same_choice(a.explore_result(), b.explore_result(), ctx)
                assert a.seeds() == b.seeds(), ctx
                hits += assert_same_priorities(a, b, ctx, fca[i])
        assert hits > 0
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()
        h.close()


def test_records_of_a_sweep_with_fca_members_are_the_oracles_for_the_concatenated_problem():
    from oracle import oracle

    members = fca_members(max_vehicles=32, max_nodes=1 << 17)
    h, mpa, options = shared_handle(32)
    swept = [m.make(h, mpa) for m in members]
    sweep = NativeSweep(swept, h)
    unbounded = copy.copy(options)
    unbounded.max_nodes = 1 << 30
    try:
        for k in range(1, 5):
            gpu = np.concatenate(sweep.step())
            assert sweep.prep_calls()[3] == 1
            sp = sweep.problem()
            # the oracle plans level by level: the sweep's slots sorted by their member's computation level
            level = [lv for c in swept for lv in c.problem()["levels"]]
            order = sorted(range(sweep.n), key=lambda s: level[s])
            place = {s: q for q, s in enumerate(order)}
            prob = {
                "iters": [sp["iters"][s] for s in order],
                "fallback": [sp["fallback"][s] for s in order],
                "preds": [[place[p] for p in sp["preds"][s]] for s in order],
                "level_sizes": [sum(1 for lv in level if lv == l) for l in range(1, max(level) + 1)],
            }
            ref, _ = oracle.plan_step(unbounded, mpa, prob, n_threads=min(os.cpu_count() or 1, 16))
            assert_records_equal(gpu[order], ref, "sweep step %d" % k)
    finally:
        sweep.close()
        for c in swept:
            c.close()
        h.close()
