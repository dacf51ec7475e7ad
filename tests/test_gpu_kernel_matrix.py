"""Every compiled variant of the graph search (bulk_search.hpp) under the features that change its code path, at its LDS layout limits
and at the horizon limits, against the oracle: records byte-identical (and pop sequence and tree where check_batch asks for them).

The search is built four ways and the launch picks a layout at run time (compute_lds_bulk, csrc/launch_plan.hpp):

    bulk     InterX, one successor-mask word (bulk_kernel.hip, NW=1)          single_speed automaton (12 trims)
    wide     InterX, more than 64 trims (bulk_kernel_wide.hip, NW=0)          realistic automaton (71 trims, 2 mask words)
    sat1     separating-axis checker (bulk_kernel_sat.hip), one mask word     single_speed
    sat2     separating-axis checker, two mask words                          realistic
    compact  InterX, one mask word, 8 wavefronts in half the LDS              single_speed, PDMPC_TUNING compact=1

Every test here proves which one ran: it adds debug_lds=1 to PDMPC_TUNING and reads the "pdmpc LDS layout" lines that
compute_lds_bulk prints on fd 2 -- the "(compact)" tag, the wavefront count and where the maneuver areas live (areas 1: LDS,
areas 0: L2) -- and the automaton's trim count gives the mask words.  Without that a change of the selection rule would quietly move
a test onto another kernel.

Also here: the priority enumeration (priority_kernel.hip) at its limits of 32 edges and 64 vertices, against closed-form counts.
"""
import copy
import math
import os
import re

import numpy as np
import pytest

from pdmpc import abi
from pdmpc.backend import ERR_CAPACITY, BackendError, CapacityError, Handle, unique_priorities_call
from pdmpc.config import Config, MpaType, ScenarioType
from pdmpc.iteration_data import info_from_record

import problems
from test_gpu_parity import assert_records_equal, check_batch
from test_optimal_reference import complete
from test_optimal_reference_counts import closed_form_count, cycle, disjoint_union, pendant, star, tree_path

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
N_CU = 256  # MI355X: compute_lds_bulk takes twelve wavefronts for launches of more than two searches per CU

# variant -> (checker mode, automaton, Hp of its problems, seed of its problem set, extra tuning)
VARIANTS = {
    "bulk": ("interx", MpaType.single_speed, 6, 3, "compact=0"),  # (a launch of more than two searches per CU goes compact by default)
    "wide": ("interx", MpaType.realistic, 5, 42, ""),
    "sat1": ("sat", MpaType.single_speed, 6, 6, ""),
    "sat2": ("sat", MpaType.realistic, 5, 7, ""),
    "compact": ("interx", MpaType.single_speed, 6, 3, "compact=1"),
}
NAMES = list(VARIANTS)


def _oracle():
    from oracle import oracle

    return oracle


def set_tuning(monkeypatch, variant, tuning=""):
    """PDMPC_TUNING for `variant` plus `tuning`, with the layout printed (read at pdmpc_create: set it before making a handle)."""
    entries = [e for e in (VARIANTS[variant][4] if variant else "", tuning, "debug_lds=1") if e]
    monkeypatch.setenv("PDMPC_TUNING", ",".join(entries))


LAYOUT_LINE = re.compile(r"pdmpc LDS layout( \(compact\))?: launch (\d+) waves (\d+)(?: areas (\d))?")


def layouts(capfd):
    """The layouts compute_lds_bulk chose since the last call: [{compact, launch, waves, areas}] (the compact layout keeps the
    maneuver areas in L2: areas 0)."""
    err = capfd.readouterr().err
    out = []
    for m in LAYOUT_LINE.finditer(err):
        out.append({"compact": m.group(1) is not None, "launch": int(m.group(2)), "waves": int(m.group(3)), "areas": int(m.group(4) or 0)})
    return out


def tuned_waves(tuning):
    m = re.search(r"(?:^|,)waves=(\d+)", tuning)
    return int(m.group(1)) if m else None


def assert_variant(lines, variant, mpa, tuning="", areas=None):
    """Every launch since the last read ran `variant`'s kernel and layout."""
    mode, mpa_type, _, _, _ = VARIANTS[variant]
    assert lines, "no LDS layout line: the search kernel did not run"
    assert (mpa.n_trims > 64) == (mpa_type == MpaType.realistic)  # two successor-mask words: the NW=0 paths
    W = tuned_waves(tuning)
    for L in lines:
        assert L["compact"] == (variant == "compact"), (variant, L)
        if variant == "compact":
            want = min(W, 8) if W is not None else 8
        else:
            cap = 12 if mode == "sat" else 16
            want = min(W, cap) if W is not None else (min(12, cap) if L["launch"] > 2 * N_CU else cap)
        assert L["waves"] == want, (variant, tuning, L)
        if areas is not None:
            assert L["areas"] == areas, (variant, L)
        elif variant == "compact":
            assert L["areas"] == 0
        else:
            # the realistic automaton's 527 maneuvers never fit LDS; the 12-trim automaton's do next to a small soup
            assert L["areas"] == (0 if mpa_type == MpaType.realistic else 1), (variant, L)


def variant_problems(variant, count, seed=None, Hp=None):
    mode, mpa_type, vHp, vseed, _ = VARIANTS[variant]
    return problems.problem_set(mode, vseed if seed is None else seed, count, Hp=vHp if Hp is None else Hp, mpa_type=mpa_type)


def unbounded(options):
    u = copy.copy(options)
    u.max_nodes = 1 << 30
    return u


# ---------------------------------------------------------------- the variant x feature matrix


@pytest.mark.parametrize("variant", NAMES)
def test_batch_parity(variant, monkeypatch, capfd):
    set_tuning(monkeypatch, variant)
    options, mpa, iters = variant_problems(variant, 8)
    check_batch(options, mpa, iters)
    assert_variant(layouts(capfd), variant, mpa)


TUNINGS = ["force_tie=1", "share_min=64,tile=32,round0=128", "mid_min=0,mid_fill=256", "ready=256,round0=300,helpers=0", "waves=5,round0=7"]


@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("variant", NAMES)
def test_tuning_changes_the_path_not_the_result(variant, tuning, monkeypatch, capfd):
    """Forced replay through the binary heap, rounds shared with helper workgroups, every far list fed through the mid list, a
    ready list smaller than a round, five wavefronts: the oracle's records, pop sequences and trees on every variant."""
    set_tuning(monkeypatch, variant, tuning)
    options, mpa, iters = variant_problems(variant, 8)
    gpu, stats = check_batch(options, mpa, iters)
    assert_variant(layouts(capfd), variant, mpa, tuning)
    assert stats["kernel"] == 2
    if tuning.startswith("force_tie"):
        assert stats["queue_fallbacks"] >= len(iters)
    if tuning.startswith("share_min"):
        assert stats["shared_rounds"] > 0 and 0 < stats["helper_checked"] < stats["nodes_processed"], stats


# realistic-automaton problems whose oracle searches pop many tied minima: (problem_set seed at Hp 5, vehicle, tied pops)
TIED_REALISTIC = {"interx": [(3, 1, 619), (6, 3, 280)], "sat": [(7, 1, 188), (6, 5, 144), (3, 2, 30), (4, 6, 30)]}


@pytest.mark.parametrize("variant", NAMES)
def test_real_ties_fall_back_to_the_binary_heap(variant, monkeypatch, capfd):
    """Searches that pop tied minimal keys: problems.symmetric_problem with the variant's automaton (single_speed at Hp 6: 129 tied
    pops of 742 with InterX), and for the realistic automaton -- whose symmetric problem ties only where the order decides nothing
    (3 tied pops, no replay) -- also road problems with hundreds of tied pops (TIED_REALISTIC).  Two copies of each in one batch
    return identical records, equal to the oracle's, and at least one search ended on the replay through the binary heap (not sat2:
    see below)."""
    set_tuning(monkeypatch, variant)
    mode, mpa_type, _, _, _ = VARIANTS[variant]
    realistic = mpa_type == MpaType.realistic
    Hp = 5 if realistic else 6
    options = problems.make_options(mode, Hp=Hp, mpa_type=mpa_type)
    mpa = problems.get_mpa(options)
    tied = [problems.symmetric_problem(options, mpa)]
    if realistic:
        for seed, v, _ in TIED_REALISTIC[mode]:
            tied.append(problems.problem_set(mode, seed, v + 1, Hp=Hp, mpa_type=mpa_type)[2][v])
    _, _, traces = _oracle().plan_batch(options, mpa, tied, trace=True)
    assert all(problems.tied_pops(t) > 0 for t in traces[1:] if realistic) and problems.tied_pops(traces[-1]) > 0
    rng = np.random.default_rng(5)
    ordinary = problems.road_problem(rng, options, mpa, convex=(mode == "sat"))
    gpu, stats = check_batch(options, mpa, [ordinary] + tied + tied)
    assert_variant(layouts(capfd), variant, mpa)
    if variant != "sat2":
        assert stats["queue_fallbacks"] >= 1, stats
    # (sat2: none of the tied searches found for it -- these four and two more -- meets equal keys where the order decides, so none
    # ends on the replay; its replay path is covered with force_tie=1 in test_tuning_changes_the_path_not_the_result)
    k = len(tied)
    assert gpu[1 : 1 + k].tobytes() == gpu[1 + k :].tobytes()


@pytest.mark.parametrize("variant", NAMES)
def test_arena_regrows_from_64_nodes(variant, monkeypatch, capfd):
    set_tuning(monkeypatch, variant)
    options, mpa, iters = variant_problems(variant, 6, seed=22)
    options.max_nodes = 1 << 22
    _, ref, _ = _oracle().plan_batch(options, mpa, iters, n_threads=THREADS)
    assert (ref["status"] != abi.ARENA_OVERFLOW).all()
    options.max_nodes = 64
    options.max_vehicles = 8
    h = Handle(options)
    h.upload_mpa(mpa)
    gpu = h.plan_batch(iters)
    assert_records_equal(gpu, ref, "grown arena (%s)" % variant)
    nodes, regrows = h.arena_nodes()
    assert regrows >= 1 and nodes >= int(ref["n_expanded"].max())
    h.close()
    assert_variant(layouts(capfd), variant, mpa)


@pytest.mark.parametrize("variant", NAMES)
def test_step_with_predecessors(variant, monkeypatch, capfd):
    """A two-level coupling DAG over 12 of the variant's problems in one pdmpc_plan_step: the second level's searches start
    speculatively and verify their trees against the first level's areas when those arrive."""
    set_tuning(monkeypatch, variant)
    options, mpa, iters = variant_problems(variant, 12, seed=13)
    preds = [[] for _ in range(4)] + [sorted({i % 4, (i + 1) % 4}) for i in range(8)]
    prob = {"iters": iters, "preds": preds, "fallback": [None] * 12, "level_sizes": [4, 8]}
    ref, _ = _oracle().plan_step(unbounded(options), mpa, prob, n_threads=THREADS)
    options.max_vehicles = 12
    options.max_nodes = 1 << 15
    h = Handle(options)
    h.upload_mpa(mpa)
    arrivals = 0
    for rep in range(2):
        gpu = h.plan_step(iters, preds, [[] for _ in iters])
        assert_records_equal(gpu, ref, "step %d (%s)" % (rep, variant))
        st = h.stats()
        assert st["safe_replans"] == 0
        arrivals += st["speculation_arrivals"]
    h.close()
    assert arrivals > 0
    assert_variant(layouts(capfd), variant, mpa)


HELPED_STEP_SEED = 13  # problem_set seed at which every variant shares rounds, has helpers check entries AND meets arrivals (see below)
HELPED_STEP_TUNING = "share_min=64,tile=32,round0=128"  # (TUNINGS[1]: rounds of 128 nodes, shared from 64 entries on, 32 entries per seat)


def helped_step(variant, seed):
    """test_step_with_predecessors' step (12 problems, levels 4 + 8, two repetitions) under HELPED_STEP_TUNING, PDMPC_TUNING already
    set: the counters summed over the repetitions, and the records of both against the oracle's."""
    options, mpa, iters = variant_problems(variant, 12, seed=seed)
    preds = [[] for _ in range(4)] + [sorted({i % 4, (i + 1) % 4}) for i in range(8)]
    prob = {"iters": iters, "preds": preds, "fallback": [None] * 12, "level_sizes": [4, 8]}
    ref, _ = _oracle().plan_step(unbounded(options), mpa, prob, n_threads=THREADS)
    options.max_vehicles = 12
    options.max_nodes = 1 << 15
    h = Handle(options)
    h.upload_mpa(mpa)
    total = {"safe_replans": 0, "shared_rounds": 0, "helper_checked": 0, "nodes_processed": 0, "speculation_arrivals": 0}
    for rep in range(2):
        gpu = h.plan_step(iters, preds, [[] for _ in iters])
        assert_records_equal(gpu, ref, "helped step %d (%s, seed %d)" % (rep, variant, seed))
        st = h.stats()
        for k in total:
            total[k] += st[k]
    h.close()
    return total, mpa


@pytest.mark.parametrize("variant", NAMES)
def test_helpers_mirror_a_search_with_predecessors(variant, monkeypatch, capfd):
    """Seated helper workgroups AND predecessors on every instantiation: the second level's searches share their rounds, so their
    helpers mirror a soup with predecessor slots -- NaN slots, expected areas, the areas that arrive (HB_MASK), the lists rebuilt after
    an arrival -- and their verdicts go into records that must be the oracle's byte for byte.  The owner/helper contract of
    csrc/bk_shared.hpp is what this holds together."""
    set_tuning(monkeypatch, variant, HELPED_STEP_TUNING)
    total, mpa = helped_step(variant, HELPED_STEP_SEED)
    print("helped step (%s): %s" % (variant, total))
    assert total["safe_replans"] == 0, total
    assert total["shared_rounds"] > 0, total
    assert 0 < total["helper_checked"] < total["nodes_processed"], total
    assert total["speculation_arrivals"] > 0, total
    assert_variant(layouts(capfd), variant, mpa, HELPED_STEP_TUNING)


@pytest.mark.parametrize("variant", ["bulk", "wide"])
def test_road_network_closed_loop(variant, monkeypatch, capfd):
    """Ten vehicles on the lab map for five steps, every step against the oracle; arrival verification ran on this instantiation
    and the safety net never did."""
    from oracle import oracle
    from pdmpc.controller import PrioritizedSequentialController
    from pdmpc.mpa import get_mpa
    from pdmpc.road_network import boundary_provider, commonroad_scenario

    set_tuning(monkeypatch, variant)
    _, mpa_type, Hp, _, _ = VARIANTS[variant]
    options = Config(scenario_type=ScenarioType.commonroad, amount=10, Hp=Hp, mpa_type=mpa_type, max_vehicles=16, max_nodes=1 << 15)
    sc = commonroad_scenario(options, seed=1)
    mpa = get_mpa(options)
    h = Handle(options)
    h.upload_mpa(mpa)
    ctl = PrioritizedSequentialController(options, sc, mpa, None, coupling="distance", boundary_provider=boundary_provider(sc))
    total = {"speculation_arrivals": 0, "safe_replans": 0}

    def plan_step(prob):
        gpu = h.plan_step(prob["iters"], prob["preds"], [f if f is not None else [] for f in prob["fallback"]])
        ref, _ = oracle.plan_step(unbounded(options), mpa, prob, n_threads=THREADS)
        assert_records_equal(gpu, ref, "closed loop (%s)" % variant)
        st = h.stats()
        for k in total:
            total[k] += st[k]
        return [info_from_record(gpu[i], Hp) for i in range(len(gpu))]

    for _ in range(5):
        ctl.step(plan_step=plan_step)
    h.close()
    assert total["speculation_arrivals"] > 0 and total["safe_replans"] == 0, total
    assert_variant(layouts(capfd), variant, mpa)


@pytest.mark.parametrize("variant", NAMES)
def test_oversubscribed_reverse_dispatch(variant, monkeypatch, capfd):
    """600 copies of four independent searches, more than the chip holds at once, workgroups handed out in reverse order: every
    copy returns the original's record, which is the oracle's, and no search waited on another (no safe re-plan)."""
    set_tuning(monkeypatch, variant, "reverse_dispatch=1")
    distinct, copies = 4, 600
    options, mpa, iters = variant_problems(variant, distinct, seed=11)
    _, ref, _ = _oracle().plan_batch(unbounded(options), mpa, iters, n_threads=THREADS)
    options.max_vehicles = copies
    options.max_nodes = 1 << 14
    h = Handle(options)
    h.upload_mpa(mpa)
    batch = [iters[i % distinct] for i in range(copies)]
    recs = h.plan_step(batch, [[] for _ in batch], None)
    st = h.stats()
    h.close()
    assert_records_equal(recs[:distinct], ref, "the originals (%s)" % variant)
    want = recs[np.arange(copies) % distinct]
    bad = [i for i in range(copies) if recs[i : i + 1].tobytes() != want[i : i + 1].tobytes()]
    assert not bad, "copies in slots %s differ from the original's" % bad[:8]
    assert st["safe_replans"] == 0
    lines = layouts(capfd)
    assert_variant(lines, variant, mpa, "reverse_dispatch=1")
    assert all(L["launch"] == copies for L in lines)


# ---------------------------------------------------------------- layout limits


def far_obstacles(it, n):
    """`n` small static obstacles 30 m and more away from the vehicle: beyond any tree's reach, so only the soup grows (the
    problem's own near obstacles still decide edges)."""
    x, y = float(it.x0[0]), float(it.x0[1])
    out = list(it.obstacles)
    for i in range(n):
        out.append(problems.rect(x + 30.0 + 0.4 * (i % 50), y + 30.0 + 0.4 * (i // 50), 0.3 * i, 0.24, 0.12))
    return out


def with_soup(it, n):
    c = copy.copy(it)
    c.obstacles = far_obstacles(it, n)
    return c


def first_true(pred, lo=0, hi=16):
    """Smallest n >= lo with pred(n), pred monotone and pred(lo) false: doubling, then bisection."""
    while not pred(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


def is_capacity_error(e):
    return "status %d" % ERR_CAPACITY in str(e)


def soup_batch(iters, n):
    return [with_soup(it, n) for it in iters]


def bulk_probe(h, batch, capfd):
    """Plan `batch`: the layout line of its launch, or None for PDMPC_ERR_CAPACITY (the soup a launch needs is its largest
    vehicle's)."""
    capfd.readouterr()
    try:
        h.plan_batch(batch)
    except BackendError as e:
        assert is_capacity_error(e), e
        assert not layouts(capfd)
        return None
    lines = layouts(capfd)
    assert len(lines) >= 1
    return lines[-1]


def assert_soup_parity(h, options, mpa, iters, ctx):
    gpu = h.plan_batch(iters)
    _, ref, _ = _oracle().plan_batch(unbounded(options), mpa, iters, n_threads=THREADS)
    assert_records_equal(gpu, ref, ctx)


@pytest.mark.parametrize("variant", ["bulk", "sat1", "sat2"])
def test_maneuver_areas_move_to_l2_when_the_soup_grows(variant, monkeypatch, capfd):
    """compute_lds_bulk keeps the maneuver areas in LDS while the soup leaves room and reads them from L2 beyond: both sides of the
    step plan like the oracle.  (With the realistic automaton on InterX the areas are always in L2: see test_batch_parity.)"""
    set_tuning(monkeypatch, variant)
    options, mpa, iters = variant_problems(variant, 3, seed=17)
    options.max_vehicles = 4
    h = Handle(options)
    h.upload_mpa(mpa)
    first = bulk_probe(h, soup_batch(iters, 0), capfd)
    if VARIANTS[variant][1] == MpaType.realistic:
        assert first["areas"] == 0  # (527 maneuvers: the areas never fit, at any soup)
        n0 = 0
    else:
        assert first["areas"] == 1
        n0 = first_true(lambda n: (bulk_probe(h, soup_batch(iters, n), capfd) or {"areas": 0})["areas"] == 0)
        assert bulk_probe(h, soup_batch(iters, n0 - 1), capfd)["areas"] == 1
        assert_soup_parity(h, options, mpa, [with_soup(it, n0 - 1) for it in iters], "areas 1 at the edge (%s)" % variant)
    assert bulk_probe(h, soup_batch(iters, n0 + 1), capfd)["areas"] == 0
    capfd.readouterr()
    assert_soup_parity(h, options, mpa, [with_soup(it, n0 + 1) for it in iters], "areas 0 (%s)" % variant)
    assert_variant(layouts(capfd), variant, mpa, areas=0)
    h.close()


def test_compact_falls_back_to_the_full_layout(monkeypatch, capfd):
    """compact=1 with a soup beyond the compact budget (half the LDS) runs the full layout (no compact tag) and plans like the oracle."""
    set_tuning(monkeypatch, "compact")
    options, mpa, iters = variant_problems("compact", 3, seed=17)
    options.max_vehicles = 4
    h = Handle(options)
    h.upload_mpa(mpa)
    assert bulk_probe(h, soup_batch(iters, 0), capfd)["compact"]
    n = first_true(lambda n: not bulk_probe(h, soup_batch(iters, n), capfd)["compact"])
    capfd.readouterr()
    assert_soup_parity(h, options, mpa, [with_soup(it, n - 1) for it in iters], "compact at the edge")
    lines = layouts(capfd)
    assert lines and all(L["compact"] for L in lines)
    assert_soup_parity(h, options, mpa, [with_soup(it, n) for it in iters], "compact falling back to the full layout")
    lines = layouts(capfd)
    assert lines and not any(L["compact"] for L in lines) and lines[-1]["waves"] == 16
    h.close()


@pytest.mark.parametrize("variant", ["bulk", "sat1", "wide"])
def test_capacity_error_at_the_lds_limit_leaves_no_state_behind(variant, monkeypatch, capfd):
    """The largest soup that fits plans like the oracle; one obstacle more is PDMPC_ERR_CAPACITY before any kernel runs; then the
    same handle plans an ordinary batch like the oracle (bank flags, step weights and the LDS high-water mark left as they were)."""
    set_tuning(monkeypatch, variant)
    options, mpa, iters = variant_problems(variant, 3, seed=17)
    options.max_vehicles = 4
    h = Handle(options)
    h.upload_mpa(mpa)
    n = first_true(lambda n: bulk_probe(h, soup_batch(iters, n), capfd) is None)
    assert_soup_parity(h, options, mpa, [with_soup(it, n - 1) for it in iters], "largest soup (%s)" % variant)
    assert_variant(layouts(capfd), variant, mpa, areas=0)
    big = [with_soup(it, n) for it in iters]
    h.set_step_weights([1.0, 2.0, 3.0])
    with pytest.raises(BackendError, match="status %d" % ERR_CAPACITY):
        h.plan_step(big, [[], [0], [1]], [[], [], []])
    assert not layouts(capfd)
    with pytest.raises(BackendError, match="status %d" % ERR_CAPACITY):
        h.plan_batch(big)
    assert_soup_parity(h, options, mpa, iters, "after the capacity error (%s)" % variant)
    assert_variant(layouts(capfd), variant, mpa)
    h.close()


def test_sampled_optimizer_capacity_and_areas_in_l2():
    """compute_lds_sampled: the soup grows until the layout fails.  The largest soup that fits runs the areas-0 branch (the
    automaton's area tables are larger than one obstacle's columns, so a layout with them would not fit one obstacle less either) and
    equals the oracle; one more is PDMPC_ERR_CAPACITY; the same handle then plans an ordinary batch like the oracle."""
    options, mpa, iters = variant_problems("bulk", 3, seed=17)
    options.max_vehicles = 4
    seeds = [3, 4, 5]
    h = Handle(options)
    h.upload_mpa(mpa)

    def fails(n):
        try:
            h.plan_batch_sampled(soup_batch(iters, n), seeds)
            return False
        except BackendError as e:
            assert is_capacity_error(e), e
            return True

    n = first_true(fails)
    n_man = sum(1 for row in mpa.maneuvers for m in row if m is not None)
    assert n_man * 3 * abi.VMAX * 16 > options.Hp * 6 * 16  # (area tables against one obstacle's columns: 5 points + separator per step)
    big = [with_soup(it, n - 1) for it in iters]
    gpu = h.plan_batch_sampled(big, seeds)
    _, ref = _oracle().plan_batch_sampled(options, mpa, big, seeds, n_threads=THREADS)
    assert_records_equal(gpu, ref, "sampled, largest soup")
    assert fails(n)
    gpu = h.plan_batch_sampled(iters, seeds)
    _, ref = _oracle().plan_batch_sampled(options, mpa, iters, seeds, n_threads=THREADS)
    assert_records_equal(gpu, ref, "sampled after the capacity error")
    h.close()


def test_joint_search_capacity_then_recovery():
    """layout_joint: a two-vehicle problem whose soups do not fit LDS is PDMPC_ERR_CAPACITY; the same handle then plans like the
    reference, and the largest soup that fits too."""
    import joint_reference as jr
    from pdmpc.centralized import centralized_mpa, centralized_options
    from test_gpu_joint import shifted

    options = centralized_options(Config(scenario_type=ScenarioType.circle, amount=2, Hp=3, mpa_type=MpaType.single_speed, max_vehicles=4))
    mpa = centralized_mpa(options)
    sym = problems.symmetric_problem(options, mpa)
    prob = [sym, shifted(sym, 0.0, 3.0)]
    h = Handle(options)
    h.upload_mpa(mpa)

    def fails(n):
        try:
            h.plan_joint([[with_soup(prob[0], n), with_soup(prob[1], n)]])
            return False
        except BackendError as e:
            assert is_capacity_error(e), e
            return True

    n = first_true(fails)
    edge = [[with_soup(prob[0], n - 1), with_soup(prob[1], n - 1)]]
    from test_joint_reference import assert_records_equal as joint_equal

    joint_equal(h.plan_joint(edge), jr.plan_joint(options, mpa, edge, max_nodes=h.arena_nodes()[0]), "largest soup")
    assert fails(n)
    joint_equal(h.plan_joint([prob]), jr.plan_joint(options, mpa, [prob], max_nodes=h.arena_nodes()[0]), "after the capacity error")
    h.close()


# ---------------------------------------------------------------- horizon limits

HP16_SEEDS = {  # problem_set(..., count 1, Hp 16) seeds whose oracle trees stay small (nodes, oracle time on one core)
    "bulk": [3],  # count 6 at seed 3: 1 582 .. 29 312 nodes, 0.06 s for all six
    "wide": [5, 11, 15, 23],  # 95 255, 63 015, 79 123 (exhausted), 60 616 nodes; 0.06 .. 0.11 s each
    "sat1": [2, 6, 8, 10],  # 2 578, 3 864, 2 252, 5 752 nodes; under 0.01 s each
}


def hp16_problems(variant):
    mode, mpa_type, _, _, _ = VARIANTS[variant]
    if variant == "bulk":
        return problems.problem_set(mode, 3, 6, Hp=16, mpa_type=mpa_type)
    iters = []
    for s in HP16_SEEDS[variant]:
        options, mpa, its = problems.problem_set(mode, s, 1, Hp=16, mpa_type=mpa_type)
        iters += its
    return options, mpa, iters


@pytest.mark.parametrize("variant", ["bulk", "wide", "sat1"])
def test_horizon_16(variant, monkeypatch, capfd):
    """Hp = PDMPC_HP_MAX.  Problems picked by seed (HP16_SEEDS; a free road with the realistic automaton at Hp 16 runs for minutes in
    the oracle), and the oracle's trees are asserted to stay under 200 000 nodes so a change of the generators cannot make this slow."""
    assert abi.HP_MAX == 16
    set_tuning(monkeypatch, variant)
    options, mpa, iters = hp16_problems(variant)
    bounded = copy.copy(options)
    bounded.max_nodes = 200000
    _, ref, _ = _oracle().plan_batch(bounded, mpa, iters, n_threads=THREADS)
    assert (ref["status"] != abi.ARENA_OVERFLOW).all(), ref["n_expanded"]
    options.max_vehicles = len(iters)
    options.max_nodes = 1 << 15
    h = Handle(options)
    h.upload_mpa(mpa)
    assert_records_equal(h.plan_batch(iters), ref, "Hp 16 (%s)" % variant)
    h.close()
    assert_variant(layouts(capfd), variant, mpa)


@pytest.mark.parametrize("variant", ["bulk", "wide", "sat1"])
def test_horizon_1(variant, monkeypatch, capfd):
    """Hp = 1, including a search exhausted at its first step (a wall through the vehicle), with full trees and pop traces."""
    set_tuning(monkeypatch, variant)
    options, mpa, iters = variant_problems(variant, 6, seed=3, Hp=1)
    x, y = iters[0].x0[0], iters[0].x0[1]
    iters[0].obstacles = [problems.rect(x, y, np.pi / 2, 1.2, 0.05)]
    gpu, _ = check_batch(options, mpa, iters)
    assert gpu["status"][0] == abi.EXHAUSTED and (gpu["status"][1:] == abi.OK).any()
    assert_variant(layouts(capfd), variant, mpa)


@pytest.mark.parametrize("Hp", [1, 16])
def test_sampled_optimizer_at_the_horizon_limits(Hp):
    options, mpa, iters = problems.problem_set("interx", 3, 6, Hp=Hp)
    x, y = iters[0].x0[0], iters[0].x0[1]
    iters[0].obstacles = [problems.rect(x, y, np.pi / 2, 1.2, 0.05)]
    options.max_vehicles = 8
    seeds = [11 + i for i in range(len(iters))]
    h = Handle(options)
    h.upload_mpa(mpa)
    gpu = h.plan_batch_sampled(iters, seeds)
    h.close()
    _, ref = _oracle().plan_batch_sampled(options, mpa, iters, seeds, n_threads=THREADS)
    assert_records_equal(gpu, ref, "sampled Hp %d" % Hp)
    assert ref["status"][0] == abi.EXHAUSTED and (ref["status"] == abi.OK).any()


def test_joint_search_at_hp_1():
    """Two vehicles, Hp 1: a free pair and a pair whose first vehicle is walled in (exhausted at its first step).  (Hp 16 is out of
    reach of the Python reference: two free vehicles at Hp 8 already expand 227 380 joint nodes, 7 s.)"""
    import joint_reference as jr
    from pdmpc.centralized import centralized_mpa, centralized_options
    from test_gpu_joint import shifted
    from test_joint_reference import assert_records_equal as joint_equal

    options = centralized_options(Config(scenario_type=ScenarioType.circle, amount=2, Hp=1, mpa_type=MpaType.single_speed, max_vehicles=4))
    mpa = centralized_mpa(options)
    sym = problems.symmetric_problem(options, mpa)
    walled = copy.copy(sym)
    walled.obstacles = [problems.rect(0.0, 0.0, np.pi / 2, 1.2, 0.05)]
    probs = [[sym, shifted(sym, 0.0, 3.0)], [walled, shifted(sym, 0.0, 3.0)]]
    h = Handle(options)
    h.upload_mpa(mpa)
    got = h.plan_joint(probs)
    want = jr.plan_joint(options, mpa, probs, max_nodes=h.arena_nodes()[0])
    h.close()
    joint_equal(got, want, "joint Hp 1")
    assert (want["status"][:2] == abi.OK).all() and (want["status"][2:] == abi.EXHAUSTED).all()


def test_horizon_outside_1_to_16_and_a_short_automaton_are_refused():
    for Hp in (0, 17):
        options = problems.make_options("interx", Hp=6)
        options.Hp = Hp
        with pytest.raises(BackendError, match="Hp"):
            Handle(options)
    short = problems.make_options("interx", Hp=4)
    mpa4 = problems.get_mpa(short)
    options = problems.make_options("interx", Hp=6)
    h = Handle(options)
    with pytest.raises(BackendError):
        h.upload_mpa(mpa4)
    h.close()


# ---------------------------------------------------------------- priority enumeration at its limits


def count_on_device(h, A):
    """K from the count-only call (max_out 0): the true count rides on the capacity error."""
    with pytest.raises(CapacityError) as e:
        h.unique_priorities(A, 0)
    return e.value.count


def n_edges(A):
    return int(np.triu(A, 1).sum())


@pytest.mark.timeout(300)
def test_priority_counts_at_29_to_32_edges():
    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 12)
    h = Handle(options)
    cases = [
        # 32-edge forest: two stars of 16 edges: K = 2^32, beyond uint32
        (disjoint_union(star(16), star(16)), 1 << 32),
        # E 29: C_5 + C_6 + a 18-edge path
        (disjoint_union(cycle(5), cycle(6), tree_path(18)), (2**5 - 2) * (2**6 - 2) * 2**18),
        # E 30: three C_7 + a 9-edge star
        (disjoint_union(cycle(7), cycle(7), cycle(7), star(9)), (2**7 - 2) ** 3 * 2**9),
        # E 31: K_5 + C_9 + a 12-edge path
        (disjoint_union(complete(5), cycle(9), tree_path(12)), math.factorial(5) * (2**9 - 2) * 2**12),
        # E 32: K_8 with 4 pendant edges
        (pendant(complete(8), 4), math.factorial(8) * 2**4),
    ]
    for A, K in cases:
        assert 29 <= n_edges(A) <= 32 and closed_form_count(A) == K
        assert count_on_device(h, A) == K, (n_edges(A), K)
    assert n_edges(cases[0][0]) == 32
    h.close()


def test_priorities_on_vertices_32_and_above_equal_the_host_twin():
    """n = 64, five triangles on vertices 40..54 and every low vertex isolated: 6^5 = 7 776 orderings, the placed mask of the order
    kernel beyond bit 31."""
    A = np.zeros((64, 64), dtype=np.int64)
    for t in range(5):
        a, b, c = 40 + 3 * t, 41 + 3 * t, 42 + 3 * t
        for r, s in ((a, b), (a, c), (b, c)):
            A[r, s] = A[s, r] = 1
    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 12)
    h = Handle(options)
    assert count_on_device(h, A) == 6**5
    got_p, got_m = h.unique_priorities(A, 6**5)
    want_p, want_m = unique_priorities_call(A, 6**5)
    h.close()
    assert len(got_m) == 6**5
    assert np.array_equal(got_m, want_m) and np.array_equal(got_p, want_p)
    assert np.array_equal(np.sort(got_p, axis=0), np.tile(np.arange(1, 65)[:, None], (1, len(got_m))))


def test_priority_limits_are_capacity_errors():
    options = Config(scenario_type=ScenarioType.circle, amount=4, Hp=5, max_vehicles=8, max_nodes=1 << 12)
    h = Handle(options)
    A33 = disjoint_union(star(16), star(17))
    assert n_edges(A33) == 33
    for A in (A33, np.zeros((65, 65), dtype=np.int64)):
        with pytest.raises(CapacityError) as e:
            h.unique_priorities(A, 1 << 20)
        assert e.value.count == -1
    h.close()
