"""The graph search's reach lists (include/pdmpc_reach.h) on the device: small step problems whose obstacle
segments lie just inside and just outside a step's reach, whose predecessors' areas move into and out of reach when they arrive, and
whose lists are built in more than one trip or are empty -- records byte for byte the oracle's, through the product, the generic and
the compact instantiation and with the wide kernel's automaton."""
import copy
import math
import re

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.config import MpaType
from pdmpc.iteration_data import VehicleIter

import problems
from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu

# variant -> (automaton, horizons, PDMPC_TUNING, kernel the layout line must name)
VARIANTS = {
    "product": (MpaType.single_speed, (2, 8), "compact=0", "pdmpc_bulk_kernel"),
    "generic": (MpaType.single_speed, (8,), "compact=0,generic=1", "pdmpc_bulk_kernel_any"),
    "compact": (MpaType.single_speed, (8,), "compact=1", "pdmpc_bulk_kernel_compact"),
    "wide": (MpaType.realistic, (5,), "", "pdmpc_bulk_kernel_wide"),
}
CASES = [(v, Hp) for v, (_, hps, _, _) in VARIANTS.items() for Hp in hps]
# Where a vehicle in front of the follower stands and how far in front of it its own obstacle is, per automaton, so that it brakes inside
# what the follower plans to cover (the realistic automaton's vehicles start in its slowest trim: 0.13 m/s against 0.8 m/s)
AHEAD = {MpaType.single_speed: (0.5, 0.5), MpaType.realistic: (0.3, 0.3)}


def reach(mpa):
    """(Dmax, Amax) of the automaton, as pdmpc_upload_mpa computes them."""
    dmax = amax = 0.0
    for row in mpa.maneuvers:
        for m in row:
            if m is None:
                continue
            dmax = max(dmax, math.hypot(m.dx, m.dy))
            for a in (m.area, m.area_without_offset, m.area_large_offset):
                amax = max(amax, float(np.max(np.hypot(a[0], a[1]))))
    return dmax, amax


def rho(dmax, amax, k, x, y):
    R = (k - 1) * dmax + amax
    R = R + R * 2.0 ** -50
    return R + 2.0 ** -20 * (1.0 + abs(x) + abs(y) + R)


def blocked_ahead(options, mpa):
    x, gap = AHEAD[options.mpa_type]
    return vehicle(options, mpa, x=x, obstacles=[bar(x + gap, half=0.6)])


def vehicle(options, mpa, x=0.0, y=0.0, obstacles=(), dyn=(), boundary=True, lane_y=None):
    """A vehicle at (x, y) heading along +x on a straight corridor around y = lane_y."""
    lane_y = y if lane_y is None else lane_y
    xs = np.linspace(x - 1.0, x + 60.0, 400)
    centre = np.column_stack([xs, np.full_like(xs, lane_y)])
    trim = [i + 1 for i, t in enumerate(mpa.trims) if t.steering == 0 and t.speed > 0][0]
    speed = float(max(mpa.get_straight_speeds_of_mpa()))
    path, _, v_ref, _ = problems.get_reference_trajectory(mpa, centre, speed, x, y, trim, options.dt_seconds)
    left = np.vstack([xs[::8], np.full_like(xs[::8], lane_y + 0.3)])
    right = np.vstack([xs[::8], np.full_like(xs[::8], lane_y - 0.3)])
    return VehicleIter(hdv_reachable_sets=[], x0=np.array([x, y, 0.0, mpa.trims[trim - 1].speed]), trim_index=trim, reference_trajectory_points=path, v_ref=v_ref,
                       predicted_lanelet_boundary=(left, right) if boundary else (None, None), obstacles=list(obstacles), dynamic_obstacle_area=list(dyn))


def bar(x, y=0.0, half=0.2):
    """One obstacle segment across the lane at x (a two-column polygon)."""
    return np.array([[x, x], [y - half, y + half]])


def boxes(x, y, Hp, step=0.0):
    return [problems.rect(x + step * k, y, 0.0, 0.24, 0.12) for k in range(Hp)]


def setup(variant, Hp, monkeypatch, tuning=""):
    mpa_type, _, base, _ = VARIANTS[variant]
    monkeypatch.setenv("PDMPC_TUNING", ",".join(e for e in (base, tuning, "debug_lds=1") if e))
    options = problems.make_options("interx", Hp=Hp, mpa_type=mpa_type)
    options.max_vehicles = 16
    options.max_nodes = 1 << 16
    return options, problems.get_mpa(options)


def plan(options, mpa, prob, label):
    """The step on the device and through the oracle: the same bytes.  Returns the device's records and its statistics."""
    from oracle import oracle
    from pdmpc.optimizer import GraphSearchHip

    opt = GraphSearchHip(options)
    try:
        opt._ensure_mpa(mpa)
        gpu = opt.handle.plan_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])
        stats = opt.handle.stats()
    finally:
        opt.handle.close()
    unbounded = copy.copy(options)
    unbounded.max_nodes = 1 << 30
    ref, _ = oracle.plan_step(unbounded, mpa, prob)
    assert_records_equal(gpu, ref, label)
    assert stats["kernel"] == 2 and stats["safe_replans"] == 0, stats
    return gpu, stats


def step_problem(iters, preds, fallback=None):
    return {"iters": iters, "preds": preds, "fallback": fallback if fallback is not None else [None] * len(iters), "level_sizes": level_sizes(preds)}


def level_sizes(preds):
    level = []
    for p in preds:
        level.append(1 + max([level[q] for q in p], default=-1))
    assert level == sorted(level)
    return [level.count(l) for l in range(max(level) + 1)]


def assert_kernel(capfd, variant, strict=True):
    """Which instantiation ran (strict=False: a soup that moves the maneuver areas to L2 may select the generic twin)."""
    names = re.findall(r"pdmpc LDS layout[^\n]* kernel (\w+)", capfd.readouterr().err)
    want = VARIANTS[variant][3]
    assert names and set(names) <= ({want} if strict else {want, want + "_any"}), (variant, names)


@pytest.mark.parametrize("variant,Hp", CASES)
def test_obstacle_segment_at_the_edge_of_a_steps_reach(variant, Hp, monkeypatch, capfd):
    """One static segment across the lane, first reached at step k (beyond the reach of step k - 1) for k = 1, 2, Hp; and just outside
    the reach of the last step: then the plan is the obstacle-free plan."""
    options, mpa = setup(variant, Hp, monkeypatch)
    dmax, amax = reach(mpa)
    free, _ = plan(options, mpa, step_problem([vehicle(options, mpa)], [[]]), "no obstacle")
    for k in sorted({1, 2, Hp}):
        at = 0.5 * amax if k == 1 else 0.5 * (rho(dmax, amax, k - 1, 0.0, 0.0) + rho(dmax, amax, k, 0.0, 0.0))
        assert (k == 1 or at > rho(dmax, amax, k - 1, 0.0, 0.0)) and at < rho(dmax, amax, k, 0.0, 0.0)
        plan(options, mpa, step_problem([vehicle(options, mpa, obstacles=[bar(at)])], [[]]), "segment first reached at step %d" % k)
    out = math.nextafter(rho(dmax, amax, Hp, 0.0, 0.0), math.inf) + 1e-9
    far, _ = plan(options, mpa, step_problem([vehicle(options, mpa, obstacles=[bar(out)])], [[]]), "segment beyond the last step's reach")
    assert far.tobytes() == free.tobytes()
    assert_kernel(capfd, variant)


@pytest.mark.parametrize("variant,Hp", CASES)
def test_predecessor_areas_move_into_and_out_of_reach(variant, Hp, monkeypatch, capfd):
    options, mpa = setup(variant, Hp, monkeypatch)
    follower = vehicle(options, mpa)
    ahead = blocked_ahead(options, mpa)  # in the follower's lane, just in front of it, and blocked: it brakes
    away = vehicle(options, mpa, x=0.0, y=40.0)    # drives where the follower never gets
    alone, _ = plan(options, mpa, step_problem([follower], [[]]), "follower alone")
    # expected areas far out of reach, the solved plan in the follower's lane: the list goes from empty to non-empty at the arrival
    gpu, _ = plan(options, mpa, step_problem([ahead, follower], [[], [0]], [boxes(0.0, 80.0, Hp), None]), "expected far, solved near")
    if Hp > 2:  # (two steps are over before the follower gets anywhere near)
        assert gpu[1:].tobytes() != alone.tobytes(), "the follower does not yield: the case tests nothing"
    # the reverse: expected areas in the lane, the solved plan far away: parked nodes come back, nothing is due for a re-check
    gpu2, _ = plan(options, mpa, step_problem([away, follower], [[], [0]], [boxes(0.5, 0.0, Hp, 0.05), None]), "expected near, solved far")
    assert gpu2[1:].tobytes() == alone.tobytes()
    # a predecessor that publishes exactly what it was expected to
    solved = [np.array(gpu[0]["shapes"][k][:, : int(gpu[0]["shape_cols"][k])]) for k in range(Hp)]
    gpu3, _ = plan(options, mpa, step_problem([ahead, follower], [[], [0]], [solved, None]), "expected == solved")
    assert gpu3.tobytes() == gpu.tobytes()
    # a predecessor without expectation (NaN-only slot until it arrives)
    plan(options, mpa, step_problem([ahead, follower], [[], [0]], [None, None]), "no expectation")
    # an exhausted predecessor (a segment through its own footprint: status 1) publishes its fallback areas, which lie in the follower's lane
    wall = [bar(0.45 + 0.05, half=0.6)]
    stuck = vehicle(options, mpa, x=0.45, obstacles=wall)
    gpu4, _ = plan(options, mpa, step_problem([stuck, follower], [[], [0]], [boxes(0.5, 0.0, Hp), None]), "exhausted predecessor")
    assert int(gpu4[0]["status"]) == 1
    assert_kernel(capfd, variant)


@pytest.mark.parametrize("variant,Hp", CASES)
def test_lists_built_in_two_trips_and_steps_without_any_segment(variant, Hp, monkeypatch, capfd):
    """Ten predecessors (80 slot columns per step: the vehicle-obstacle list of a step takes two 64-segment trips), one of them in the
    follower's lane; and a follower without boundary whose only obstacle is beyond the reach of its first steps: those steps have no
    segment at all, the later ones do."""
    options, mpa = setup(variant, Hp, monkeypatch)
    dmax, amax = reach(mpa)
    others = [vehicle(options, mpa, x=0.0, y=30.0 + 5.0 * i) for i in range(9)]
    ahead = blocked_ahead(options, mpa)
    follower = vehicle(options, mpa)
    n = len(others) + 1
    fallback = [boxes(0.6, 0.0, Hp) if i % 2 else None for i in range(n)] + [None]
    plan(options, mpa, step_problem(others + [ahead, follower], [[] for _ in range(n)] + [list(range(n))], fallback), "ten predecessors")
    k = min(3, Hp)
    at = 0.5 * (rho(dmax, amax, k - 1, 0.0, 0.0) + rho(dmax, amax, k, 0.0, 0.0))
    bare = vehicle(options, mpa, obstacles=[bar(at)], boundary=False)
    plan(options, mpa, step_problem([bare], [[]]), "no segment in reach before step %d" % k)
    plan(options, mpa, step_problem([vehicle(options, mpa, boundary=False)], [[]]), "no segment at all")
    assert_kernel(capfd, variant, strict=False)


def standing(options, mpa, x, y):
    """A vehicle that stands at (x, y) and is to stay there: a search of a few dozen nodes."""
    v = vehicle(options, mpa, x=x, y=y)
    trim = [i + 1 for i, t in enumerate(mpa.trims) if t.speed == 0][0]
    xs = np.linspace(x - 1.0, x + 60.0, 400)
    path, _, v_ref, _ = problems.get_reference_trajectory(mpa, np.column_stack([xs, np.full_like(xs, y)]), 0.0, x, y, trim, options.dt_seconds)
    v.trim_index, v.x0, v.reference_trajectory_points, v.v_ref = trim, np.array([x, y, 0.0, 0.0]), path, v_ref
    return v


def helper_scenario(options, mpa):
    """(predecessor, follower): a follower whose search is long (its lane blocked a few steps ahead, no boundary: it looks for a way
    round, 20 000 nodes) and shares its rounds, and a predecessor that stands beside the far end of that obstacle, where the
    follower's way round leads at its steps 4 to 8: a search of under a hundred nodes, so it arrives in the follower's first rounds,
    and the nodes that meet its areas are expanded, and checked by owner and helpers from their lists, long after the arrival."""
    dmax, amax = reach(mpa)
    at3 = 0.5 * (rho(dmax, amax, 2, 0.0, 0.0) + rho(dmax, amax, 3, 0.0, 0.0))
    return standing(options, mpa, 0.6, 0.25), vehicle(options, mpa, obstacles=[bar(at3)], boundary=False)


@pytest.mark.parametrize("variant", ["product", "generic"])
def test_helpers_rebuild_their_lists_on_an_arrival(variant, monkeypatch, capfd):
    """A search that shares its rounds with seated helper workgroups while a predecessor arrives whose EXPECTED areas lie far out of
    reach and whose solved areas lie where the follower searches: before the arrival the lists of owner and helpers hold none of that
    predecessor's slot segments, after it they must.  A helper (or an owner) that went on with the lists it had would miss those
    segments, find edges free that cross the predecessor's areas, and return another plan than the oracle.  That the arrival met the
    running, sharing search is read from the search's own diagnostics (debug_tail: the round at which the last arrival met it
    running, its rounds in all)."""
    from pdmpc.optimizer import GraphSearchHip

    Hp = VARIANTS[variant][1][-1]
    tuning = "share_min=16,tile=16,round0=64"
    options, mpa = setup(variant, Hp, monkeypatch, tuning)
    pred, heavy = helper_scenario(options, mpa)
    alone, _ = plan(options, mpa, step_problem([heavy], [[]]), "the follower alone")
    prob = step_problem([pred, heavy], [[], [0]], [boxes(0.0, 80.0, Hp), None])
    gpu, stats = plan(options, mpa, prob, "shared rounds with an arrival")
    assert gpu[1:].tobytes() != alone.tobytes(), "the predecessor's solved areas do not change the follower's plan: a stale list would go unnoticed"
    assert int(gpu[1]["n_expanded"]) > 10 * int(gpu[0]["n_expanded"])  # (the predecessor's search is by far the shorter one)
    assert stats["shared_rounds"] >= 2 and stats["helper_checked"] > 0 and stats["speculation_arrivals"] >= 1, stats
    assert_kernel(capfd, variant)
    # the same step once more with the search's diagnostics in the unused last rows of path_nodes (this selects the generic instantiation)
    monkeypatch.setenv("PDMPC_TUNING", ",".join(e for e in (VARIANTS[variant][2], tuning, "debug_tail=1") if e))
    opt = GraphSearchHip(options)
    try:
        opt._ensure_mpa(mpa)
        dbg = opt.handle.plan_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])
        dstats = opt.handle.stats()
    finally:
        opt.handle.close()
    rounds, at_arrival = int(dbg[1]["path_nodes"][abi.HP_MAX][0]), int(dbg[1]["path_nodes"][abi.HP_MAX - 2][6])
    print("rounds %d, round at the arrival %d, shared rounds %d" % (rounds, at_arrival, dstats["shared_rounds"]))
    assert 0 < at_arrival < rounds, (at_arrival, rounds)  # the arrival met the running search, and rounds followed it
    assert dstats["shared_rounds"] >= 2 and dstats["helper_checked"] > 0, dstats
