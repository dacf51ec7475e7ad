"""Seed ensembles of the sampled optimizer on the GPU (pdmpc_set_sampled_ensemble, csrc/sampled_ensemble_kernel.hip):
records, winners and member costs byte for byte against the twin (sampled_ensemble_reference.py) on the smallest steps at which the
protocol can go wrong -- chains of levels whose handed-over areas are a member's other than 0, re-launches of a resident bank,
exhausted and partly exhausted slots, a tie, trees in HBM, a group of logical ranks and the native controller's closed loop."""
import copy

import numpy as np
import pytest

import sampled_ensemble_cases as sec
import sampled_ensemble_reference as ser
from pdmpc import abi, backend
from pdmpc.backend import BackendError, Group, Handle
from pdmpc.native_controller import NativeController
from test_gpu_parity import assert_records_equal
from test_gpu_sampled_budget import boxed_in_problem

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ENSEMBLE, ENSEMBLE_HBM = "pdmpc_sampled_ensemble_kernel", "pdmpc_sampled_ensemble_kernel_hbm"
MODES = {"components": backend.SHARD_COMPONENTS, "levels": backend.SHARD_LEVELS, "auto": backend.SHARD_AUTO}


def handle_for(options, mpa, n_members=None, budget=None, max_vehicles=8):
    opt = copy.copy(options)
    opt.max_vehicles = max_vehicles
    h = Handle(opt)
    h.upload_mpa(mpa)
    if budget is not None:
        h.set_sampled_budget(budget)
    if n_members is not None:
        h.set_sampled_ensemble(n_members)
    return h


def plan_step_gpu(h, prob, seeds):
    return h.plan_step_sampled(prob["iters"], prob["preds"], sec.fallback_args(prob), seeds)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_ensemble_equal(h, got, want, ctx):
    """Records, winners and member costs of the handle's last launch against the twin's (records, winners, costs (E, n))."""
    recs, winners, costs = want
    assert_records_equal(got, recs, ctx)
    assert np.ascontiguousarray(got).tobytes() == recs.tobytes(), ctx
    w, status, cost = h.sampled_ensemble_result(len(recs), n_members=costs.shape[0])
    assert w.tolist() == winners.tolist(), ctx
    assert np.array_equal(bits(cost), bits(costs.T)), ctx
    assert np.array_equal(status == 0, np.isfinite(costs.T)), ctx


@pytest.mark.parametrize("budget", [250, 12])
@pytest.mark.parametrize("n_members", [2, 3, 16])
@pytest.mark.parametrize("name", ["circle", "road"])
def test_parity_with_the_twin(name, n_members, budget):
    options, mpa, prob, seeds = sec.case(name)
    want = sec.twin(name, n_members, budget)
    # (first, on the CPU with the twin alone: a member other than 0 solved a slot that has successors)
    assert sec.has_handed_over_winner(prob, want[0], want[1]) and len(prob["level_sizes"]) >= 3
    h = handle_for(options, mpa, n_members, budget)
    try:
        assert h.get_sampled_ensemble() == n_members
        got = plan_step_gpu(h, prob, seeds)
        st = h.stats()
        assert st["kernel"] == 3 and st["n_launches"] == 1 and st["safe_replans"] == 0
        assert h.last_sampled_kernel() == ENSEMBLE
        assert_ensemble_equal(h, got, want, "%s E %d budget %d" % (name, n_members, budget))
    finally:
        h.close()


@pytest.mark.parametrize("name", ["circle", "road"])
def test_one_member_is_the_parent(name):
    options, mpa, prob, seeds = sec.case(name)
    h = handle_for(options, mpa)
    try:
        assert h.get_sampled_ensemble() == 1
        plain = plan_step_gpu(h, prob, seeds)
        assert h.last_sampled_kernel() == "pdmpc_sampled_kernel"
        h.set_sampled_ensemble(4)
        other = plan_step_gpu(h, prob, seeds)
        assert h.last_sampled_kernel() == ENSEMBLE
        h.set_sampled_ensemble(1)
        again = plan_step_gpu(h, prob, seeds)
        assert h.last_sampled_kernel() == "pdmpc_sampled_kernel"
        assert again.tobytes() == plain.tobytes() and other.tobytes() != plain.tobytes()
        assert plain.tobytes() == sec.twin(name, 1, 250)[0].tobytes()
        with pytest.raises(BackendError):  # (the bank in place was not packed as an ensemble)
            h.sampled_ensemble_result(len(seeds))
        h.set_sampled_budget(12)
        low = plan_step_gpu(h, prob, seeds)
        assert h.last_sampled_kernel() == "pdmpc_sampled_budget_kernel"
        assert low.tobytes() == sec.twin(name, 1, 12)[0].tobytes()
        # the setter's range, with a live handle: a refused value leaves the size as it was
        for bad in (0, -3, 17):
            with pytest.raises(BackendError):
                h.set_sampled_ensemble(bad)
        assert h.get_sampled_ensemble() == 1 and h.L.pdmpc_get_sampled_ensemble(h.h, None) == -1
        for ok in (16, 1):
            h.set_sampled_ensemble(ok)
            assert h.get_sampled_ensemble() == ok
    finally:
        h.close()


def test_a_resident_bank_launched_again_and_again():
    """Three launches of a resident ensemble bank, then the same bank after a graph-search bank was packed and planned in between: the
    tickets start at zero every time, the bank keeps the size it was packed with."""
    name, E, budget = "road", 3, 12
    options, mpa, prob, seeds = sec.case(name)
    want = sec.twin(name, E, budget)
    n = len(seeds)
    h = handle_for(options, mpa, E, budget)
    try:
        h.set_step_seeds(seeds)
        h.pack_step(prob["iters"], prob["preds"], sec.fallback_args(prob))
        h.set_sampled_ensemble(1)  # (the handle's size from now on; the bank keeps its own)
        with pytest.raises(BackendError):  # (packed as an ensemble, but not launched yet)
            h.sampled_ensemble_result(n, n_members=E)
        for i in range(3):
            h.launch()
            assert h.last_sampled_kernel() == ENSEMBLE
            assert_ensemble_equal(h, h.fetch(n), want, "resident launch %d" % i)
        h.select_bank(1)
        searched = h.plan_step(prob["iters"], prob["preds"], sec.fallback_args(prob))
        assert len(searched) == n
        with pytest.raises(BackendError):  # (bank 1 is a graph-search bank)
            h.sampled_ensemble_result(n, n_members=E)
        h.select_bank(0)
        h.launch()
        assert h.last_sampled_kernel() == ENSEMBLE
        assert_ensemble_equal(h, h.fetch(n), want, "after a graph-search bank")
    finally:
        h.close()


def test_a_boxed_in_vehicle_publishes_its_fallback_areas_to_its_successor():
    options, mpa, prob, seeds, rect = boxed_in_problem()
    E = 4
    want = ser.plan_step_ensemble(options, mpa, prob, seeds, E)
    assert int(want[0][0]["status"]) == 1 and not np.isfinite(want[2][:, 0]).any() and prob["preds"][1]  # every member of slot 0 is exhausted
    h = handle_for(options, mpa, E)
    try:
        got = plan_step_gpu(h, prob, seeds)
        assert_ensemble_equal(h, got, want, "boxed in")
        assert int(got[0]["status"]) == 1 and h.sampled_ensemble_result(len(seeds))[0][0] == 0
        assert list(got[0]["shape_cols"][: options.Hp]) == [rect.shape[1]] * options.Hp  # its successors got its fallback areas
    finally:
        h.close()


def test_a_partly_exhausted_slot_is_won_by_a_member_that_is_not():
    name, E, budget = "road", 16, 2
    options, mpa, prob, seeds = sec.case(name)
    want = sec.twin(name, E, budget)
    costs = want[2]
    mixed = [s for s in range(len(seeds)) if np.isfinite(costs[:, s]).any() and not np.isfinite(costs[:, s]).all()]
    assert mixed and any(not np.isfinite(costs[0, s]) for s in mixed)  # (also a slot whose member 0 is exhausted)
    h = handle_for(options, mpa, E, budget)
    try:
        got = plan_step_gpu(h, prob, seeds)
        assert_ensemble_equal(h, got, want, "partly exhausted")
        winners = h.sampled_ensemble_result(len(seeds))[0]
        for s in mixed:
            assert int(got[s]["status"]) == 0 and np.isfinite(costs[winners[s], s])
    finally:
        h.close()


def standstill_problem():
    """One vehicle of the circle at standstill with a wall right in front of it: the only collision-free successor at every step is the
    equilibrium trim (speed 0), so every member finds the same plan at the same cost."""
    options, mpa, prob, seeds = sec.case("circle")
    it = copy.copy(prob["iters"][0])
    assert int(it.trim_index) == 1 and float(mpa.trims[0].speed) == 0.0
    x, y, yaw = (float(v) for v in it.x0[:3])
    assert yaw == 0.0
    wall = np.array([[x + 0.125, x + 0.6, x + 0.6, x + 0.125, x + 0.125], [y - 0.5, y - 0.5, y + 0.5, y + 0.5, y - 0.5]])
    it.obstacles = list(it.obstacles) + [wall]
    one = {"order": [prob["order"][0]], "iters": [it], "preds": [[]], "fallback": [None], "level_sizes": [1]}
    return options, mpa, one, [seeds[0]]


def test_a_tie_goes_to_member_0():
    options, mpa, prob, seeds = standstill_problem()
    E = 16
    want = ser.plan_step_ensemble(options, mpa, prob, seeds, E)
    recs, winners, costs = want
    assert int(recs[0]["status"]) == 0 and list(recs[0]["predicted_trims"][: options.Hp]) == [1] * options.Hp
    assert np.isfinite(costs).all() and len(set(bits(costs[:, 0]).tolist())) == 1 and winners.tolist() == [0]
    h = handle_for(options, mpa, E)
    try:
        got = plan_step_gpu(h, prob, seeds)
        assert_ensemble_equal(h, got, want, "tie")
    finally:
        h.close()


def test_trees_in_hbm():
    """The smallest budget at which the plan of THIS bank puts the trees in HBM (read from the window), two members per vehicle."""
    options, mpa, prob, seeds = standstill_problem()
    E = 2
    h = handle_for(options, mpa, E, 7)
    try:
        plan_step_gpu(h, prob, seeds)  # (packs the bank the window then plans for)
        lo, hi = 7, 16384
        assert h.sampled_plan_bank(lo)[1]["tree_in_lds"] == 1 and h.sampled_plan_bank(hi)[1]["tree_in_lds"] == 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if h.sampled_plan_bank(mid)[1]["tree_in_lds"]:
                lo = mid
            else:
                hi = mid
        plan, extra = h.sampled_plan_bank(hi)
        assert plan["kernel"] == ENSEMBLE_HBM and extra["tree_in_lds"] == 0
        h.set_sampled_budget(hi)
        got = plan_step_gpu(h, prob, seeds)
        assert h.last_sampled_kernel() == ENSEMBLE_HBM
        assert_ensemble_equal(h, got, ser.plan_step_ensemble(options, mpa, prob, seeds, E, hi), "trees in HBM, budget %d" % hi)
        # ... and a chain at that budget: the members of different slots have trees of their own
        options, mpa, prob, seeds = sec.case("circle")
        got = plan_step_gpu(h, prob, seeds)
        assert h.last_sampled_kernel() == ENSEMBLE_HBM
        assert_ensemble_equal(h, got, sec.twin("circle", E, hi), "a chain with trees in HBM")
    finally:
        h.close()


def test_two_logical_ranks_plan_the_single_handles_records_in_every_sharding_mode():
    name, E = "road", 4
    options, mpa, prob, seeds = sec.case(name)
    want = sec.twin(name, E, 250)[0]
    args = (prob["iters"], prob["preds"], sec.fallback_args(prob))
    h = handle_for(options, mpa, E)
    try:
        single = plan_step_gpu(h, prob, seeds)
    finally:
        h.close()
    assert single.tobytes() == want.tobytes()
    g = Group(options, n_devices=2, devices=[0, 0], collective=backend.COLLECTIVE_COPY)
    try:
        g.upload_mpa(mpa)
        g.set_sampled_ensemble(E)
        for mode_name, mode in MODES.items():
            g.set_step_seeds(seeds)
            got = g.plan_step(*args, mode=mode)
            assert_records_equal(got, single, "two ranks, mode %s" % mode_name)
        # ranks with different sizes: the pack is refused
        h1 = backend.C.c_void_p()
        assert g.L.pdmpc_group_handle(g.g, 1, backend.C.byref(h1)) == 0
        assert g.L.pdmpc_set_sampled_ensemble(h1, 3) == 0
        g.set_step_seeds(seeds)
        with pytest.raises(BackendError) as e:
            g.plan_step(*args)
        assert e.value.status == -1
        for bad in (0, 17):
            with pytest.raises(BackendError):
                g.set_sampled_ensemble(bad)
        g.set_sampled_ensemble(E)
        g.set_step_seeds(seeds)
        assert_records_equal(g.plan_step(*args), single, "two ranks, after the sizes were made equal again")
    finally:
        g.close()


def test_the_native_closed_loop_follows_the_handles_ensemble_size():
    """Five closed-loop steps of the native controller on the circle, E = 4, against a handle-less controller that applies the twin's
    records: the same records and the same state after every step."""
    from pdmpc.scenario import circle_scenario

    E = 4
    options, mpa, _, _ = sec.case("circle")
    sc = circle_scenario(options)
    h = handle_for(options, mpa, E)
    nat = NativeController(options, sc, mpa, h, coupling="full", optimizer="sampled")
    ref = NativeController(options, sc, mpa, None, coupling="full", optimizer="sampled")
    try:
        for k in range(5):
            got = nat.step()
            assert h.last_sampled_kernel() == ENSEMBLE
            ref.build_step()
            prob, seeds = ref.problem(), ref.seeds()
            assert seeds == nat.seeds()
            want = ser.plan_step_ensemble(options, mpa, prob, seeds, E)
            ref.apply(want[0])
            assert_records_equal(got, want[0], "closed loop, step %d" % (k + 1))
            a, b = nat.state(), ref.state()
            for key in ("x", "y", "yaw"):
                assert np.array_equal(bits(a[key]), bits(b[key])), (k, key)
            assert a["needs_fallback"].tolist() == b["needs_fallback"].tolist()
    finally:
        nat.close()
        ref.close()
        h.close()
