"""The sampled optimizer's expansion budget above the handle (pdmpc_set_sampled_budget, pdmpc_group_set_sampled_budget):
the native controller's closed loop and an explorative step, a group of logical ranks in every sharding mode, and a sweep, each
planning with the budget of the handle it plans on -- records byte for byte against the restatement (sampled_budget_reference.py)."""
import numpy as np
import pytest

import sampled_budget_reference as sbr
from pdmpc import backend
from pdmpc.backend import BackendError, Group, Handle
from pdmpc.config import Config, ScenarioType
from pdmpc.controller import PrioritizedSequentialController
from pdmpc.iteration_data import info_from_record
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeController, NativeSweep
from test_gpu_parity import assert_records_equal
from test_gpu_sampled_budget import NEW_KERNEL, road_step, step_reference
from test_sweep import road

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MODES = {"components": backend.SHARD_COMPONENTS, "levels": backend.SHARD_LEVELS, "auto": backend.SHARD_AUTO}


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def assert_same_poses(nat, py, ctx):
    st = nat.state()
    assert np.array_equal(bits(st["x"]), bits([m.x for m in py.meas])) and np.array_equal(bits(st["y"]), bits([m.y for m in py.meas])), ctx
    assert np.array_equal(bits(st["yaw"]), bits([m.yaw for m in py.meas])), ctx
    assert st["needs_fallback"].tolist() == [bool(i.needs_fallback) for i in py.infos], ctx


def test_native_closed_loop_and_an_explorative_step_follow_the_handles_budget():
    from pdmpc.explorative import explore_step
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    budget = 32
    options = Config(scenario_type=ScenarioType.commonroad, amount=12, Hp=6, max_vehicles=64)
    sc = commonroad_scenario(options, seed=1)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    h.set_sampled_budget(budget)
    py = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    nat = NativeController(options, sc, mpa, h, coupling="distance", optimizer="sampled")
    try:
        for k in range(6):
            got = nat.step()
            assert h.last_sampled_kernel() == NEW_KERNEL and h.stats()["kernel"] == 3
            seeds = nat.seeds()
            kept = {}

            def plan_step(prob):
                assert seeds == [int(py.k) + int(v) + 1 for v in prob["order"]]
                kept["want"] = step_reference(options, mpa, prob, seeds, budget)
                return [info_from_record(kept["want"][i], options.Hp) for i in range(len(kept["want"]))]

            py.step(plan_step=plan_step)
            assert_records_equal(got, kept["want"], "native step %d" % (k + 1))
            assert_same_poses(nat, py, "native step %d" % (k + 1))
        # one explorative step, four prioritizations in ONE launch: every instance plans with the budget
        K = 4
        got, chosen = nat.explore_step(K)
        assert h.last_sampled_kernel() == NEW_KERNEL
        kept = {}

        def plan_batch(batch):
            seeds = [int(py.k) + int(v) + 1 for v in batch["order"]]
            kept["want"] = step_reference(options, mpa, batch, seeds, budget)
            return kept["want"]

        _, _, chosen_py = explore_step(py, plan_batch, K)
        assert_records_equal(got, kept["want"], "explorative step")
        assert chosen.tolist() == chosen_py
        assert_same_poses(nat, py, "explorative step")
    finally:
        nat.close()
        h.close()


@pytest.fixture(scope="module")
def step32():
    """The 20-vehicle road-network step and its records at budget 32."""
    options, mpa, prob, seeds = road_step()
    options.max_nodes = 1 << 14
    return options, mpa, prob, seeds, step_reference(options, mpa, prob, seeds, 32)


@pytest.mark.parametrize("world", [2, 4])
def test_a_group_of_logical_ranks_plans_with_its_budget_in_every_sharding_mode(step32, world):
    options, mpa, prob, seeds, want = step32
    args = (prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])
    g = Group(options, n_devices=world, devices=[0] * world, collective=backend.COLLECTIVE_COPY)
    try:
        g.upload_mpa(mpa)
        g.set_sampled_budget(32)
        for name, mode in MODES.items():
            g.set_step_seeds(seeds)
            assert_records_equal(g.plan_step(*args, mode=mode), want, "world %d mode %s" % (world, name))
        # ranks with different budgets: the pack is refused, and consumes the seeds
        h1 = backend.C.c_void_p()
        assert g.L.pdmpc_group_handle(g.g, 1, backend.C.byref(h1)) == 0
        assert g.L.pdmpc_set_sampled_budget(h1, 33) == 0
        g.set_step_seeds(seeds)
        with pytest.raises(BackendError) as e:
            g.plan_step(*args)
        assert e.value.status == -1
        for bad in (0, 16385):
            with pytest.raises(BackendError):
                g.set_sampled_budget(bad)
        assert g.L.pdmpc_group_set_sampled_budget(None, 32) == -1
        g.set_sampled_budget(32)
        g.set_step_seeds(seeds)
        assert_records_equal(g.plan_step(*args), want, "world %d after the budgets were made equal again" % world)
    finally:
        g.close()


def test_a_sweep_plans_every_member_with_the_handles_budget():
    budget = 600
    members = [road(3, 3, "distance", max_vehicles=16, max_nodes=1 << 14), road(5, 1, "distance", max_vehicles=16, max_nodes=1 << 14)]
    options = Config(scenario_type=ScenarioType.commonroad, Hp=members[0].options.Hp, max_vehicles=16, max_nodes=1 << 14)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    h.set_sampled_budget(budget)
    swept = [m.make(h, mpa, optimizer="sampled") for m in members]
    sweep = NativeSweep(swept, h)
    sm = sbr.SampledMpa(mpa)
    try:
        for k in range(1, 3):
            together = sweep.step()
            assert h.last_sampled_kernel() == NEW_KERNEL and h.stats()["n_launches"] == 1
            for i, (c, got) in enumerate(zip(swept, together)):
                prob, seeds = c.problem(), c.seeds()
                want = sbr.plan_step_sampled(c.options, mpa, prob, seeds, lambda iters, sd: sbr.plan_batch_sampled(c.options, sm, iters, sd, budget=budget))
                assert_records_equal(got, want, "lock-step %d member %d" % (k, i))
    finally:
        sweep.close()
        for c in swept:
            c.close()
        h.close()
