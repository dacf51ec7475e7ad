"""The native controller and the sweep on a multi-GPU group (pdmpc_controller_set_group, pdmpc_sweep_set_group; the sampled optimizer,
the lean read-back and the choice over the ranks: pdmpc_group_set_step_seeds, _plan_step_lean, _fetch_records_at, _plan_step_chosen;
DESIGN.md §6.1), on logical ranks that share the one GPU (PDMPC_COLLECTIVE_COPY, the device listed `world` times).

Every case holds a controller that plans over a group to the same controller on a plain handle, byte for byte after every step: state,
records, seeds, chosen instances and cost table.  The plain handle's runs are computed once per scenario and shared."""
import numpy as np
import pytest

from pdmpc import abi, backend
from pdmpc.backend import BackendError, Choice, Group, Handle, choose_host_call
from pdmpc.config import Config, ScenarioType
from pdmpc.mpa import get_mpa
from pdmpc.native_controller import NativeSweep

from test_choice import ARENA_OVERFLOW, assert_same_choice, explorative_choice, lean
from test_gpu_parity import assert_records_equal
from test_sweep import ERR_INVALID, HP, _bits, assert_same_state, circle, road

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MAX_VEHICLES, MAX_NODES = 1024, 1 << 14
REC = abi.VEHICLE_OUT_DTYPE.itemsize
ENTRY = 16
MODES = {"components": backend.SHARD_COMPONENTS, "levels": backend.SHARD_LEVELS, "auto": backend.SHARD_AUTO}
WORLDS = [1, 2, 4]


class Rig:
    """One plain handle and one group per world size for the whole module, the members' scenarios, and the plain handle's runs."""

    def __init__(self):
        self.options = Config(scenario_type=ScenarioType.commonroad, Hp=HP, max_vehicles=MAX_VEHICLES, max_nodes=MAX_NODES)
        self.mpa = get_mpa(self.options)
        self.plain = Handle(self.options)
        self.plain.upload_mpa(self.mpa)
        self.groups, self.members, self.runs = {}, {}, {}

    def group(self, world):
        if world not in self.groups:
            g = Group(self.options, n_devices=world, devices=[0] * world, collective=backend.COLLECTIVE_COPY)
            assert g.collective == "copy"
            g.upload_mpa(self.mpa)
            self.groups[world] = g
        return self.groups[world]

    def member(self, name):
        if name not in self.members:
            kw = dict(max_vehicles=MAX_VEHICLES, max_nodes=MAX_NODES)
            self.members[name] = {
                "road20": lambda: road(20, 1, "distance", **kw),  # several components, several levels
                "road12": lambda: road(12, 2, "distance", **kw),
                "road5": lambda: road(5, 1, "distance", **kw),
                "road3": lambda: road(3, 3, "distance", **kw),
                "road8": lambda: road(8, 1, "distance", **kw),
                "circle4": lambda: circle("full", **kw),
            }[name]()
        return self.members[name]

    def make(self, name, handle, optimizer):
        return self.member(name).make(handle, self.mpa, optimizer=optimizer)

    def close(self):
        for g in self.groups.values():
            g.close()
        self.plain.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def snapshot(c, result=None):
    s = {"state": c.state(), "records": c.records().tobytes(), "seeds": c.seeds()}
    if result is not None:
        s["result"] = getattr(c, result)()
    return s


def assert_same_snapshot(a, b, ctx):
    assert_same_state(a["state"], b["state"], ctx)
    assert a["records"] == b["records"], ctx
    assert a["seeds"] == b["seeds"], ctx
    if "result" in a:
        assert_same_choice(a["result"], b["result"], ctx)


# how a controller is driven one step, and which result it leaves
DRIVES = {
    "plain": (lambda c: c.step(), None),
    "explore_records": (lambda c: c.explore_step(4), "explore_result"),  # every record comes back, the choice on the host
    "explore_lean": (lambda c: c.explore_run(4, 1), "explore_result"),  # status + cost of every plan, the chosen records afterwards
    "optimal_lean": (lambda c: c.optimal_run(64, 1), "optimal_result"),
}


def solo_run(rig, name, drive, optimizer, n_steps, follow_own=False):
    """the member's closed loop on the plain handle, once per module: a snapshot per step"""
    key = (name, drive, optimizer, n_steps, follow_own)
    if key not in rig.runs:
        c = rig.make(name, rig.plain, optimizer)
        c.explore_follow_own(follow_own)
        step, result = DRIVES[drive]
        try:
            rig.runs[key] = []
            for _ in range(n_steps):
                step(c)
                rig.runs[key].append(snapshot(c, result))
        finally:
            c.close()
    return rig.runs[key]


def group_run(rig, name, drive, optimizer, n_steps, world, mode, follow_own=False, device_choice=False):
    want = solo_run(rig, name, drive, optimizer, n_steps, follow_own)
    g = rig.group(world)
    c = rig.make(name, g.rank0(), optimizer)
    c.explore_follow_own(follow_own)
    c.set_device_choice(device_choice)
    c.set_group(g, mode)
    step, result = DRIVES[drive]
    try:
        for k in range(n_steps):
            step(c)
            assert_same_snapshot(want[k], snapshot(c, result), "%s %s world %d mode %d step %d" % (name, drive, world, mode, k + 1))
        t = c.last_timing()
        assert t["wait_and_read_back"] > 0
    finally:
        c.close()
    return g


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("world", WORLDS)
def test_plain_closed_loop_on_a_group(rig, world, mode, optimizer):
    g = group_run(rig, "road20", "plain", optimizer, 4, world, MODES[mode])
    x = g.last_exchange()
    assert x["host_waits"] >= 1 and x["host_bytes"] >= 20 * REC  # pdmpc_group_plan_step: whole records to the host


@pytest.mark.parametrize("follow_own", [False, True], ids=["chosen", "follow_own"])
@pytest.mark.parametrize("choice", ["host", "device"])
@pytest.mark.parametrize("world", WORLDS)
def test_explorative_step_on_a_group(rig, world, choice, follow_own):
    """4 prioritizations of 12 vehicles: instances are components of their batch and are dealt out over the ranks."""
    g = group_run(rig, "road12", "explore_lean", "graph_search", 3, world, backend.SHARD_COMPONENTS, follow_own, choice == "device")
    x = g.last_exchange()
    if choice == "device":
        # pdmpc_group_plan_step_chosen: one wait per attempt, and only the 12 kept records and the small arrays reach the host
        assert x["host_waits"] == 1 + x["replans"]
        assert 12 * REC <= x["host_bytes"] // (1 + x["replans"]) < 13 * REC + 8 * 48 + 64
    else:
        assert x == {"collective_bytes": 0, "host_bytes": 12 * REC, "host_waits": 1, "replans": 0}  # pdmpc_group_fetch_records_at


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
@pytest.mark.parametrize("mode", ["levels", "auto"])
def test_explorative_step_in_the_other_modes_and_with_every_record(rig, mode, optimizer):
    group_run(rig, "road12", "explore_lean", optimizer, 3, 2, MODES[mode], device_choice=True)
    group_run(rig, "road12", "explore_lean", optimizer, 3, 4, MODES[mode])
    group_run(rig, "road12", "explore_records", optimizer, 3, 2, MODES[mode])


@pytest.mark.parametrize("choice", ["host", "device"])
@pytest.mark.parametrize("world", WORLDS)
def test_optimal_priority_step_on_a_group(rig, world, choice):
    """5 vehicles, every unique prioritization of their coupling graph in one batch."""
    group_run(rig, "road5", "optimal_lean", "graph_search", 3, world, backend.SHARD_AUTO, device_choice=choice == "device")
    if world == 2:
        group_run(rig, "circle4", "optimal_lean", "sampled", 2, world, backend.SHARD_COMPONENTS, device_choice=choice == "device")


SWEEP_DRIVES = {
    "plain": (lambda s: s.step(), lambda c: c.step(), None),
    "explorative": (lambda s: s.explore_step(4), lambda c: c.explore_step(4), "explore_result"),
    "optimal": (lambda s: s.optimal_step(100), lambda c: c.optimal_step(100), "optimal_result"),  # (8 vehicles: 48 unique prioritizations)
}


@pytest.mark.parametrize("drive", list(SWEEP_DRIVES))
def test_sweep_of_three_members_on_four_ranks(rig, drive):
    """Members of 3, 5 and 8 vehicles on 4 ranks (more ranks than heavy members): each ends every lock-step where the same member
    stepped alone on a plain handle ends it."""
    names = ["road3", "road5", "road8"]
    g = rig.group(4)
    step_sweep, step_solo, result = SWEEP_DRIVES[drive]
    solo = [rig.make(n, rig.plain, "graph_search") for n in names]
    swept = [rig.make(n, g.rank0(), "graph_search") for n in names]
    sweep = NativeSweep(swept, g.rank0())
    sweep.set_group(g, backend.SHARD_AUTO)
    try:
        for k in range(3):
            for c in solo:
                step_solo(c)
            together = step_sweep(sweep)
            for i, (a, b) in enumerate(zip(solo, swept)):
                assert together[i].tobytes() == b.records().tobytes(), (k, i)
                assert_same_snapshot(snapshot(a, result), snapshot(b, result), "%s lock-step %d member %d" % (drive, k + 1, i))
        assert sweep.last_timing()["wait_and_read_back"] > 0
        # back on the handle in mid-run: the members go on as their twins do
        sweep.set_group(None)
        for c in solo:
            step_solo(c)
        step_sweep(sweep)
        for i, (a, b) in enumerate(zip(solo, swept)):
            assert_same_snapshot(snapshot(a, result), snapshot(b, result), "%s back on the handle, member %d" % (drive, i))
    finally:
        sweep.close()
        for c in solo + swept:
            c.close()


def test_set_group_null_returns_a_controller_to_its_handle_in_mid_run(rig):
    want = solo_run(rig, "road20", "plain", "graph_search", 4)
    g = rig.group(2)
    c = rig.make("road20", g.rank0(), "graph_search")
    try:
        c.set_group(g, backend.SHARD_AUTO)
        for k in range(2):
            c.step()
            assert_same_snapshot(want[k], snapshot(c), "on the group, step %d" % (k + 1))
        c.set_group(None)
        for k in range(2, 4):
            c.step()
            assert_same_snapshot(want[k], snapshot(c), "back on the handle, step %d" % (k + 1))
    finally:
        c.close()


def test_set_group_refusals(rig):
    g2, g4 = rig.group(2), rig.group(4)
    on_plain = rig.make("road5", rig.plain, "graph_search")
    on_g2 = rig.make("road5", g2.rank0(), "graph_search")
    plain_sweep = NativeSweep([on_plain], rig.plain)
    try:
        for call in (
            lambda: on_plain.set_group(g2, backend.SHARD_AUTO),  # a member on another handle
            lambda: on_g2.set_group(g4, backend.SHARD_AUTO),  # ... also another group's
            lambda: on_g2.set_group(g2, 7),  # an unknown mode
            lambda: plain_sweep.set_group(g2, backend.SHARD_AUTO),  # a sweep whose member is on a plain handle
            lambda: plain_sweep.set_group(g2, -1),
        ):
            with pytest.raises(BackendError) as e:
                call()
            assert e.value.status == ERR_INVALID
        on_g2.set_group(g2, backend.SHARD_LEVELS)  # ... and the refusals left the controller usable
        on_g2.step()
        on_plain.step()
        assert on_g2.records().tobytes() == on_plain.records().tobytes()
    finally:
        plain_sweep.close()
        on_plain.close()
        on_g2.close()


# ---- the group's own entry points on an explorative batch: seeds, the lean read-back, the choice, arenas that overflow


@pytest.fixture(scope="module")
def batch(rig):
    """A real explorative batch (12 vehicles x 3 prioritizations) after three closed-loop steps, with picks of every vehicle; its
    records by the graph search and by the sampled optimizer on the plain handle."""
    from pdmpc.controller import PrioritizedSequentialController
    from pdmpc.explorative import build_exploration_batch
    from pdmpc.iteration_data import info_from_record
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    options = Config(scenario_type=ScenarioType.commonroad, amount=12, Hp=HP, max_vehicles=MAX_VEHICLES, max_nodes=MAX_NODES)
    sc = commonroad_scenario(options, seed=2)
    ctl = PrioritizedSequentialController(options, sc, rig.mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))

    def plan(prob):
        recs = rig.plain.plan_step(prob["iters"], prob["preds"], [f or [] for f in prob["fallback"]])
        return [info_from_record(recs[i], options.Hp) for i in range(len(recs))]

    for _ in range(3):
        ctl.step(plan_step=plan)
    b = build_exploration_batch(ctl, 3, seed=ctl.k + 1)
    b["fb"] = [f or [] for f in b["fallback"]]
    b["seeds"] = [ctl.k + v + 1 for v in b["vehicle"]]
    slot = {(p, v): s for s, (p, v) in enumerate(zip(b["instance"], b["vehicle"]))}
    _, labels, graphs = explorative_choice(b)
    b["picks"] = [(graphs.index(labels[v]), [slot[(p, v)] for p in range(3)]) for v in range(12)] + [(-1, [slot[(0, 5)]])]
    b["choice"], _, _ = explorative_choice(b, b["picks"])
    b["ref"] = {"graph_search": rig.plain.plan_step(b["iters"], b["preds"], b["fb"]).copy()}
    b["ref"]["sampled"] = rig.plain.plan_step_sampled(b["iters"], b["preds"], b["fb"], b["seeds"]).copy()
    assert b["ref"]["sampled"].tobytes() != b["ref"]["graph_search"].tobytes()
    return b


def assert_chosen(got, batch, ref, ctx):
    chosen, cost, kept = got
    want_chosen, want_cost = choose_host_call(*lean(ref, HP), batch["choice"])
    assert chosen.tolist() == want_chosen.tolist() and np.array_equal(_bits(cost), _bits(want_cost)), ctx
    for i, (g, slots) in enumerate(batch["picks"]):
        assert kept[i].tobytes() == ref[slots[0 if g < 0 else want_chosen[g]]].tobytes(), (ctx, i)


@pytest.mark.parametrize("optimizer", ["graph_search", "sampled"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("world", [2, 4])
def test_group_entry_points_on_an_explorative_batch(rig, batch, world, mode, optimizer):
    g, ref, n = rig.group(world), batch["ref"][optimizer], 36
    args = (batch["iters"], batch["preds"], batch["fb"])
    ctx = "world %d mode %s %s" % (world, mode, optimizer)

    def seeded():
        if optimizer == "sampled":
            g.set_step_seeds(batch["seeds"])

    # every record: the seeds are routed with the sub-problems in every sharding mode
    seeded()
    assert_records_equal(g.plan_step(*args, mode=MODES[mode]), ref, ctx)
    # lean: statuses and costs in the caller's order, 16 bytes per record and per rank's header to the host, then records from their holders
    seeded()
    status, cost = g.plan_step_lean(*args, mode=MODES[mode])
    want_status, want_cost = lean(ref, HP)
    assert status.tolist() == want_status.tolist() and np.array_equal(_bits(cost), _bits(want_cost)), ctx
    x = g.last_exchange()
    assert x["host_bytes"] == ENTRY * (n + world) and x["host_waits"] == 1 and x["replans"] == 0, (ctx, x)
    if mode == "components":
        assert x["collective_bytes"] == 0, (ctx, x)  # no record has left the device that planned it
    want = [35, 0, 17, 17, 8]
    got = g.fetch_records_at(want)
    assert got.tobytes() == ref[want].tobytes(), ctx
    assert g.last_exchange() == {"collective_bytes": 0, "host_bytes": 5 * REC, "host_waits": 1, "replans": 0}
    # ... the lean launch left no gathered records behind: the whole-record fetch is refused, the choice on the resident bank is not
    with pytest.raises(BackendError) as e:
        g.fetch(0, n)
    assert e.value.status == ERR_INVALID
    assert_chosen(g.choose_resident(0, n, batch["choice"]), batch, ref, ctx + " resident")
    # chosen
    seeded()
    assert_chosen(g.plan_step_chosen(*args, batch["choice"], mode=MODES[mode]), batch, ref, ctx + " chosen")
    x = g.last_exchange()
    assert x["host_waits"] == 1 and x["replans"] == 0, (ctx, x)
    assert x["host_bytes"] == 16 + (4 * batch["choice"].n_graphs + 7) // 8 * 8 + 8 * batch["choice"].n_cells + 13 * REC, (ctx, x)
    # seeds are consumed by the pack they were set for, and a count other than the step's is refused before anything is launched
    if optimizer == "sampled":
        assert_records_equal(g.plan_step(*args, mode=MODES[mode]), batch["ref"]["graph_search"], ctx + " after the seeds")
        g.set_step_seeds(batch["seeds"][:-1])
        with pytest.raises(BackendError) as e:
            g.plan_step_lean(*args, mode=MODES[mode])
        assert e.value.status == ERR_INVALID
        with pytest.raises(BackendError) as e:
            g.fetch_records_at([0])  # the failed pack emptied the bank
        assert e.value.status == ERR_INVALID


@pytest.mark.parametrize("world", [2, 4])
def test_a_step_that_overflows_small_arenas_is_planned_again(rig, batch, world):
    """Arenas of 64 nodes: the first attempt overflows, the arenas are doubled on every rank until the step fits, and the step ends with
    the records of the unlimited run -- through _lean + _fetch_records_at and through _chosen."""
    import copy

    ref, n = batch["ref"]["graph_search"], 36
    assert int(ref["n_expanded"].max()) > 64
    small = copy.copy(rig.options)
    small.max_nodes = 64
    args = (batch["iters"], batch["preds"], batch["fb"])
    for path in ("lean", "chosen"):
        g = Group(small, n_devices=world, devices=[0] * world, collective=backend.COLLECTIVE_COPY)
        try:
            g.upload_mpa(rig.mpa)
            if path == "lean":
                status, cost = g.plan_step_lean(*args, mode=backend.SHARD_COMPONENTS)
                x = g.last_exchange()
                assert (status != ARENA_OVERFLOW).all() and status.tolist() == ref["status"].tolist()
                assert g.fetch_records_at(list(range(n))).tobytes() == ref.tobytes()
                assert x["host_bytes"] == (1 + x["replans"]) * ENTRY * (n + world)
            else:
                assert_chosen(g.plan_step_chosen(*args, batch["choice"], mode=backend.SHARD_COMPONENTS), batch, ref, "chosen after overflow")
                x = g.last_exchange()
            assert x["replans"] >= 1 and x["host_waits"] == 1 + x["replans"], (path, x)
        finally:
            g.close()
