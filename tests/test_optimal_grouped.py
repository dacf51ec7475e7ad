"""The unique prioritizations of several coupling graphs in one call and the optimal-priority step of a sweep, without a GPU
(pdmpc_unique_priorities_grouped_host, pdmpc_sweep_optimal_build / _problem / _apply): every block of the
grouped twin is the ungrouped twin on that graph alone, what does not fit is refused with every count reported and nothing written,
and a handle-less sweep leaves every member where its never-swept twin's own optimal-priority steps leave it."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pdmpc.backend import BackendError, CapacityError, unique_priorities_call, unique_priorities_grouped_call
from pdmpc.config import Config, ScenarioType
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController, NativeSweep

from test_native_controller import assert_same_problem
from test_optimal_reference import complete, random_graph
from test_sweep import ERR_CAPACITY, ERR_INVALID, assert_same_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def count_of(A):
    with pytest.raises(CapacityError) as e:
        unique_priorities_call(A, 0)
    return e.value.count


def alone(graphs, handle=None):
    """every graph through the ungrouped call -> [(priorities, masks)]"""
    return [unique_priorities_call(A, count_of(A), handle=handle) for A in graphs]


def assert_same_lists(got, want, ctx=""):
    assert len(got) == len(want), ctx
    for g, ((p, m), (p1, m1)) in enumerate(zip(got, want)):
        assert m.tolist() == m1.tolist() and p.shape == p1.shape and np.array_equal(p, p1), (ctx, g)


def reference_graphs():
    rng = np.random.default_rng(11)
    return [complete(4), complete(6), np.zeros((3, 3)), np.zeros((1, 1))] + [random_graph(rng, int(rng.integers(2, 10)), 16) for _ in range(14)]


def test_grouped_host_twin_returns_the_ungrouped_lists_group_by_group():
    graphs = reference_graphs()
    want = alone(graphs)
    counts = [len(m) for _, m in want]
    assert_same_lists(unique_priorities_grouped_call(graphs, counts), want, "exact room")
    assert_same_lists(unique_priorities_grouped_call(graphs, max(counts) + 3), want, "spare room")
    assert_same_lists(unique_priorities_grouped_call(graphs[::-1], counts[::-1]), want[::-1], "reversed")
    assert_same_lists(unique_priorities_grouped_call(graphs[:1], counts[:1]), want[:1], "one group")
    assert_same_lists(unique_priorities_grouped_call([graphs[1], graphs[1]], 720), [want[1], want[1]], "the same graph twice")


def _path(n_vertices, n_edges):
    A = np.zeros((n_vertices, n_vertices), dtype=np.int64)
    for v in range(n_edges):
        A[v, v + 1] = A[v + 1, v] = 1
    return A


def test_capacity_rule_reports_every_count_and_writes_nothing():
    graphs = [complete(3), complete(4), np.zeros((5, 5)), complete(3)]
    masks = np.full(64, 0xDEADBEEF, dtype=np.uint32)
    prio = np.full(64 * 5, -77, dtype=np.int32)
    with pytest.raises(CapacityError) as e:
        unique_priorities_grouped_call(graphs, [6, 23, 1, 6], masks_out=masks, priorities_out=prio)  # K_4 has 24
    assert e.value.counts == [6, 24, 1, 6] and e.value.count == 24
    assert (masks == 0xDEADBEEF).all() and (prio == -77).all()
    # a graph outside the limits among graphs inside them: -1 for it, the true counts for the others, nothing written
    for outside in (_path(40, 33), np.zeros((65, 65))):
        with pytest.raises(CapacityError) as e:
            unique_priorities_grouped_call([complete(3), outside, complete(4)], 100, masks_out=masks, priorities_out=prio)
        assert e.value.counts == [6, -1, 24] and e.value.count == -1
        assert (masks == 0xDEADBEEF).all() and (prio == -77).all()
    with pytest.raises(CapacityError) as e:
        unique_priorities_grouped_call([np.zeros((64, 64))], 0)  # K = 1 > max_out = 0, without output arrays to speak of
    assert e.value.counts == [1]
    # ... and the same buffers take a call that fits
    got = unique_priorities_grouped_call(graphs, [6, 24, 1, 6], masks_out=masks, priorities_out=prio)
    assert_same_lists(got, alone(graphs), "after the refusals")
    assert masks[:37].tolist() == [int(m) for _, ms in got for m in ms] and (masks[37:] == 0xDEADBEEF).all()


def test_every_invalid_argument_of_the_grouped_twin_is_refused():
    import ctypes as C

    from pdmpc import abi
    from pdmpc.backend import load_library

    L = load_library()
    A = np.ascontiguousarray(complete(3), dtype=np.uint8)
    n = np.array([3], dtype=np.int32)
    cap = np.array([6], dtype=np.int64)
    K = np.zeros(1, dtype=np.int64)
    masks = np.zeros(6, dtype=np.uint32)
    prio = np.zeros(18, dtype=np.int32)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    ptrs = (abi.c_uint8_p * 1)(abi.u8p(A))
    null = (abi.c_uint8_p * 1)()
    call = L.pdmpc_unique_priorities_grouped_host
    good = [1, abi.i32p(n), ptrs, i64(cap), i64(K), abi.u32p(masks), abi.i32p(prio)]
    assert call(*good) == 0 and K[0] == 6
    for at, bad in ((0, 0), (0, -1), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (2, null)):
        args = list(good)
        args[at] = bad
        assert call(*args) == ERR_INVALID, (at, bad)
    assert call(1, abi.i32p(np.array([0], dtype=np.int32)), ptrs, i64(cap), i64(K), abi.u32p(masks), abi.i32p(prio)) == ERR_INVALID
    assert call(1, abi.i32p(n), ptrs, i64(np.array([-1], dtype=np.int64)), i64(K), abi.u32p(masks), abi.i32p(prio)) == ERR_INVALID
    # no output arrays are needed where nothing may be written
    assert call(1, abi.i32p(n), ptrs, i64(np.array([0], dtype=np.int64)), i64(K), None, None) == ERR_CAPACITY and K[0] == 6


# ---- the optimal-priority step of a handle-less sweep


def circle_member(amount):
    from pdmpc.scenario import circle_scenario

    options = Config(scenario_type=ScenarioType.circle, amount=amount, Hp=5, max_nodes=1 << 30)
    return options, circle_scenario(options)


def plan_concatenated(options, mpa, sp):
    """The oracle's records for a sweep's concatenated batch, in the batch's slot order (the oracle plans level by level: the slots
    sorted by their member's computation level)."""
    from oracle import oracle

    level = sp["levels"]
    order = sorted(range(len(level)), key=lambda s: level[s])
    place = {s: q for q, s in enumerate(order)}
    prob = {"iters": [sp["iters"][s] for s in order], "fallback": [sp["fallback"][s] for s in order], "preds": [[place[p] for p in sp["preds"][s]] for s in order],
            "level_sizes": [sum(1 for lv in level if lv == l) for l in range(1, max(level) + 1)]}
    ref, _ = oracle.plan_step(options, mpa, prob, n_threads=min(os.cpu_count() or 1, 16))
    recs = np.empty_like(ref)
    recs[order] = ref
    return recs


def member_part(sp, m):
    """member m's slots of a sweep's concatenated batch as that member's own batch (predecessor slots counted from its first slot)"""
    slots = [s for s, who in enumerate(sp["member"]) if who == m]
    first = slots[0]
    assert slots == list(range(first, first + len(slots)))
    levels = [sp["levels"][s] for s in slots]
    return first, {"order": [sp["vehicle"][s] for s in slots], "iters": [sp["iters"][s] for s in slots], "fallback": [sp["fallback"][s] for s in slots],
                   "preds": [[p - first for p in sp["preds"][s]] for s in slots], "levels": levels, "instance": [sp["instance"][s] for s in slots],
                   "level_sizes": [levels.count(l) for l in range(1, max(levels) + 1)]}


def twin_step(twin, recs, max_instances):
    """a never-swept twin's optimal-priority step on the records `recs` of its batch -> (chosen, cost table, its batch)"""
    K = twin.optimal_build(max_instances)
    q = twin.optimal_problem()
    chosen, cost = twin.optimal_choose(recs)
    slot = {(p, v): s for s, (p, v) in enumerate(zip(q["instance"], q["vehicle"]))}
    twin.apply(recs[[slot[(int(chosen[v]), v)] for v in twin.problem()["order"]]])
    return K, chosen, cost, q


def test_a_sweep_without_a_handle_leaves_its_members_where_their_own_optimal_steps_leave_them():
    made = [circle_member(a) for a in (2, 3, 4)]
    options = made[0][0]
    mpa = get_mpa(options)
    twins = [NativeController(o, sc, mpa, None, coupling="full") for o, sc in made]
    swept = [NativeController(o, sc, mpa, None, coupling="full") for o, sc in made]
    sweep = NativeSweep(swept)
    try:
        for k in range(1, 5):
            assert sweep.optimal_build(30) == [2, 6, 24], k
            assert sweep.optimal_calls() == [1, 0], k
            sp = sweep.optimal_problem()
            assert len(sp["iters"]) == 2 * 2 + 6 * 3 + 24 * 4
            recs = plan_concatenated(options, mpa, sp)
            sweep.optimal_apply(recs)
            for m, (a, b) in enumerate(zip(twins, swept)):
                ctx = "step %d member %d" % (k, m)
                first, part = member_part(sp, m)
                K, chosen, cost, q = twin_step(a, recs[first : first + len(part["iters"])], 30)
                assert_same_problem(part, q, ctx)
                assert part["instance"] == q["instance"], ctx
                got_chosen, got_cost = b.optimal_result()
                assert got_chosen.tolist() == chosen.tolist() and got_cost.shape == (a.n, K), ctx
                assert np.array_equal(got_cost.view(np.uint64), np.ascontiguousarray(cost).view(np.uint64)), ctx
                assert_same_state(a.state(), b.state(), ctx)
                assert a.seeds() == b.seeds(), ctx
                assert_same_problem(a.problem(), b.problem(), ctx + ", the member's own problem")
        # a member taken out of the sweep goes on alone like its twin
        sweep.close()
        for m, (a, b) in enumerate(zip(twins, swept)):
            for k in range(2):
                K = a.optimal_build(30)
                assert b.optimal_build(30) == K
                q = a.optimal_problem()
                assert_same_problem(q, b.optimal_problem(), "alone after the sweep, member %d" % m)
                from oracle import oracle

                recs, _ = oracle.plan_step(options, mpa, q)
                for c in (a, b):
                    chosen, _ = c.optimal_choose(recs)
                    slot = {(p, v): s for s, (p, v) in enumerate(zip(q["instance"], q["vehicle"]))}
                    c.apply(recs[[slot[(int(chosen[v]), v)] for v in c.problem()["order"]]])
                assert_same_state(a.state(), b.state(), "alone after the sweep, member %d" % m)
    finally:
        sweep.close()
        for c in twins + swept:
            c.close()


def test_every_refusal_of_the_sweeps_optimal_step():
    made = [circle_member(a) for a in (2, 3)]
    mpa = get_mpa(made[0][0])
    cs = [NativeController(o, sc, mpa, None, coupling="full") for o, sc in made]
    sweep = NativeSweep(cs)

    def status(call, *args):
        with pytest.raises(BackendError) as e:
            call(*args)
        return e.value.status

    try:
        assert status(sweep.optimal_build, 0) == ERR_INVALID
        assert status(sweep.optimal_step, 10) == ERR_INVALID  # no handle
        assert status(sweep.optimal_run, 10, 1) == ERR_INVALID
        assert status(sweep.optimal_problem) == ERR_INVALID  # nothing built
        assert all(c.state()["k"] == 0 for c in cs)  # nothing advanced
        assert sweep.optimal_build(6) == [2, 6]
        # K = 6 > max_instances: known only after the couplings exist; the sweep refuses every step afterwards
        assert status(sweep.optimal_build, 5) == ERR_CAPACITY
        assert sweep.optimal_calls() == [1, 0]
        assert status(sweep.optimal_build, 6) == ERR_INVALID
        assert status(sweep.build) == ERR_INVALID
    finally:
        sweep.close()
        for c in cs:
            c.close()


def test_grouped_priority_kernels_use_no_scratch_and_spill_nothing():
    """`make resources` on csrc/priority_kernel.hip: every pass, ungrouped and grouped, without scratch memory and without spills."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resources", "RESOURCE_SRCS=priority_kernel.hip"], capture_output=True, text=True, check=True).stdout
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    grouped = ["pdmpc_priority_count_grouped_kernel", "pdmpc_priority_write_grouped_kernel", "pdmpc_priority_order_grouped_kernel", "pdmpc_priority_group_offsets_kernel"]
    ungrouped = ["pdmpc_priority_count_kernel", "pdmpc_priority_scan_kernel", "pdmpc_priority_write_kernel", "pdmpc_priority_order_kernel"]
    for kernel in grouped + ungrouped:
        assert seen.get(kernel) == {"scratch": 0, "vgpr_spill": 0, "sgpr_spill": 0}, (kernel, seen.get(kernel))
