"""The device open list (csrc/heap_queue.hpp) at every length, LDS boundary and tie pattern, against the reference's
std::priority_queue (through the oracle), and its two users where their open lists leave LDS.

The scripts come from tests/heap_cases.py; tests/test_heap_cases.py shows on the CPU that they reach every decision point of the device
code and that a wrong heap would pop another sequence on them.  Here: the device pops exactly what the oracle pops, for every key family
at every lds_entries; pdmpc_debug_heap_script refuses what it must; the replay that ends a tied graph search (bk_replay) and the joint
search (joint_kernel.hip) run searches whose open lists are asserted -- from the reference's own trace -- to exceed what the launch plan
keeps in LDS, and return the reference's records, pop sequences and trees.
"""
import copy
import re
import time

import numpy as np
import pytest

from pdmpc.backend import BackendError, Handle
from pdmpc.config import Config

import heap_cases as hc
import joint_reference as jr
import problems
from joint_limit_cases import peak_open_list
from test_gpu_joint import circle_iters
from test_gpu_kernel_matrix import VARIANTS, first_true, is_capacity_error, set_tuning
from test_gpu_parity import check_batch
from test_joint_reference import assert_records_equal as joint_equal
from test_sampled_budget_reference import launch_plan

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def handle():
    h = Handle(Config(Hp=5, max_vehicles=2, max_nodes=1024))
    yield h
    h.close()


# ---------------------------------------------------------------- scripts


@pytest.mark.parametrize("kind,family,hl", hc.GPU_CASES, ids=["%s-%s-%d" % c for c in hc.GPU_CASES])
def test_script_pops_equal_std_priority_queue(handle, kind, family, hl):
    ops, ids, keys = hc.script(kind, family, hl)
    got, _, _ = handle.heap_script(ops, ids, keys, lds_entries=hl)
    want = _oracle().pq_script(ops, ids, keys)
    assert len(got) == len(want) == int((ops == 1).sum())
    bad = np.flatnonzero(got != want)
    assert not len(bad), "%s %s lds_entries %d: pop %d of %d is %d, the reference's is %d" % (kind, family, hl, bad[0], len(want), got[bad[0]], want[bad[0]])


def test_refusals_leave_the_handle_usable(handle):
    ops, ids, keys = hc.script("fill", "five", 64)
    ops, ids, keys = ops[:500], ids[:500], keys[:500]
    want = _oracle().pq_script(ops, ids, keys)
    for lds in (62, 65, 8194):
        with pytest.raises(BackendError, match="lds_entries"):
            handle.heap_script(ops, ids, keys, lds_entries=lds)
        assert np.array_equal(handle.heap_script(ops, ids, keys, lds_entries=64)[0], want)
    got, _, _ = handle.heap_script([], [], [], lds_entries=64)
    assert len(got) == 0
    assert np.array_equal(handle.heap_script(ops, ids, keys, lds_entries=8192)[0], want)


# ---------------------------------------------------------------- the replay of a graph search beyond its LDS part


LAYOUT =re.compile(r"pdmpc LDS layout( \(compact\))?: launch (\d+) waves (\d+)(?: areas \d)? near (\d+) ")

# (variant of tests/test_gpu_kernel_matrix.py, problem_set seed, Hp, vehicle, extra tuning, wavefronts, near capacity, peak computed when this was written)
REPLAY_CASES = [
    ("bulk", 0, 6, 1, "waves=4", 4, 1024, 2340),  # 6 326 nodes, 3 994 pops
    ("compact", 0, 6, 1, "waves=4", 4, 512, 2340),
    ("sat1", 0, 6, 2, "waves=4", 4, 1024, 1361),  # 3 720 nodes, 2 368 pops
    ("sat1", 3, 8, 7, "", 12, 3072, 5948),  # the default wavefronts: 14 895 nodes, 8 955 pops
    # the default wavefronts on a search of 148 427 nodes and 137 222 pops: beyond the oracle's trace (65 536), so the peak is a lower
    # bound from the trace's first part and check_batch compares the records (with n_popped, n_expanded, the reference's ids along the
    # path) and the counts
    ("sat1", 0, 8, 2, "", 12, 3072, None),
]


@pytest.mark.parametrize("variant,seed,Hp,vehicle,tuning,waves,near,peak", REPLAY_CASES, ids=["%s-seed%d-Hp%d-v%d" % c[:4] for c in REPLAY_CASES])
def test_replay_beyond_lds(variant, seed, Hp, vehicle, tuning, waves, near, peak, monkeypatch, capfd):
    """force_tie=1 ends the search on bk_replay, whose heap keeps `near` entries in LDS and the rest in the far list's arrays."""
    mode, mpa_type, _, _, _ = VARIANTS[variant]
    set_tuning(monkeypatch, variant, ",".join(t for t in ("force_tie=1", tuning) if t))
    options, mpa, iters = problems.problem_set(mode, seed, vehicle + 1, Hp=Hp, mpa_type=mpa_type)
    iters = [iters[vehicle]]
    ref_options = copy.copy(options)
    ref_options.max_nodes = 1 << 30  # (the reference's tree is unbounded)
    _, _, traces = _oracle().plan_batch(ref_options, mpa, iters, trace=True)
    seen = peak_open_list(traces[0].pops, traces[0].tree["parent"])
    print("%s seed %d Hp %d vehicle %d: peak open list %d, %d nodes, %d pops in the trace" % (variant, seed, Hp, vehicle, seen, len(traces[0].tree["parent"]), len(traces[0].pops)))
    if peak is not None:
        assert seen == peak
    capfd.readouterr()
    gpu, stats = check_batch(options, mpa, iters)  # records, pop sequence and tree (as sequences: force_tie=1 is set)
    lines = LAYOUT.findall(capfd.readouterr().err)
    assert lines, "no LDS layout line: the search kernel did not run"
    for compact, launch, w, n in lines:
        assert (compact != "") == (variant == "compact") and int(w) == waves
        assert int(n) == int(w) * 64 * (2 if compact else 4) == near
        assert seen > int(n), "the replay's heap stays in LDS"
    assert stats["kernel"] == 2
    assert stats["queue_fallbacks"] >= len(iters)


# ---------------------------------------------------------------- the joint search beyond its LDS part


def joint_plan_candidates(h, options, mpa, soup_caps):
    """The heap_lds of every joint plan (pdmpc_launch_plan_host) over `soup_caps` whose LDS total is the last launch's (stats)."""
    total = h.stats()["lds_bytes"]
    print("LDS bytes of the last launch: %d" % total)
    n_man = sum(1 for row in mpa.maneuvers for m in row if m is not None)
    out = set()
    for s in soup_caps:
        rc, p = launch_plan(dict(checker=h.cfg.checker, Hp=options.Hp, n_trims=mpa.n_trims, n_man=n_man, n_cu=256, device_share=1, max_nodes=1 << 15, kind=2, count=1,
                                 n_chained=0, soup_cap=s, ll_cap=0, cand_cap=0, safe=0))
        if rc == 0 and p["total"] == total:
            out.add(p["heap_lds"])
    return out


def joint_soup_fits(options, mpa, s):
    n_man = sum(1 for row in mpa.maneuvers for m in row if m is not None)
    return launch_plan(dict(checker=0, Hp=options.Hp, n_trims=mpa.n_trims, n_man=n_man, n_cu=256, device_share=1, max_nodes=1 << 15, kind=2, count=1, n_chained=0, soup_cap=s,
                            ll_cap=0, cand_cap=0, safe=0))[0] == 0


def reference_peak(options, mpa, prob, max_nodes):
    recs, info = jr.search(options, jr.JointMpa(mpa), prob, max_nodes)
    return recs, peak_open_list(info["pops"], info["tree"]["parent"])


@pytest.mark.parametrize("steps,peak", [(0, 11297), (8, 16694)])
def test_joint_search_beyond_lds(steps, peak):
    """The two-vehicle circle problems at Hp 5: open lists beyond the 8192 entries LDS can hold at most."""
    options, mpa, iters = circle_iters(2, 5, steps)
    h = Handle(options)
    h.upload_mpa(mpa)
    got = h.plan_joint([iters])
    # no obstacle, no boundary: the launch's soup_cap is a few columns (separators).  Over 48 consecutive soup_caps (64 heap entries of
    # 12 bytes = 48 columns of 16) the LDS total tells the plans apart, so exactly one of them is the launch's -- or none, and this fails
    assert not any(it.obstacles or it.dynamic_obstacle_area or it.predicted_lanelet_boundary[0] is not None for it in iters)
    planned = joint_plan_candidates(h, options, mpa, range(1, 48))
    want, seen = reference_peak(options, mpa, iters, h.arena_nodes()[0])
    h.close()
    print("joint circle after %d steps: peak open list %d, heap_lds %s" % (steps, seen, sorted(planned)))
    assert seen == peak
    assert len(planned) == 1 and 256 <= max(planned) <= 8192 and seen > max(planned)
    joint_equal(got, want, "joint circle after %d steps" % steps)


def far_soup(it, n_big, n_small):
    """`it` with n_big 40-gons and n_small rectangles 30 m and more away: only the soup grows (few large polygons keep the reference
    quick: it tests every polygon at every pop)."""
    x, y = float(it.x0[0]), float(it.x0[1])
    a = 2.0 * np.pi * np.arange(41) / 40.0
    out = list(it.obstacles)
    for i in range(n_big):
        out.append(np.vstack([x + 30.0 + 0.5 * (i % 40) + 0.2 * np.cos(a), y + 30.0 + 0.5 * (i // 40) + 0.2 * np.sin(a)]))
    for i in range(n_small):
        out.append(problems.rect(x + 30.0 + 0.4 * (i % 50), y - 30.0 - 0.4 * (i // 50), 0.3 * i, 0.24, 0.12))
    c = copy.copy(it)
    c.obstacles = out
    return c


def test_joint_search_beyond_the_smallest_lds_part():
    """The largest soup that fits leaves the open list 256 entries of LDS (layout_joint's minimum): the two-vehicle circle problem at
    Hp 3 from standstill, whose open list grows to 1787."""
    options, mpa, iters = circle_iters(2, 3, 0)
    h = Handle(options)
    h.upload_mpa(mpa)

    def fails(n_big, n_small):
        try:
            h.plan_joint([[far_soup(it, n_big, n_small) for it in iters]])
            return False
        except BackendError as e:
            assert is_capacity_error(e), e
            return True

    n_big = first_true(lambda n: fails(n, 0)) - 1
    n_small = first_true(lambda n: fails(n_big, n), hi=4) - 1
    prob = [far_soup(it, n_big, n_small) for it in iters]
    got = h.plan_joint([prob])
    # the launch's soup_cap: one more rectangle per vehicle (5 points and a separator, once per step: 2 * Hp * 6 = 36 columns) does not
    # fit, so it is within 36 of the largest soup_cap that plans; over the last 40 the LDS total tells the plans apart (see above)
    s_max = first_true(lambda s: not joint_soup_fits(options, mpa, s), lo=1, hi=1024) - 1
    assert 2 * options.Hp * 6 <= 40
    planned = joint_plan_candidates(h, options, mpa, range(s_max - 40, s_max + 1))
    want, seen = reference_peak(options, mpa, prob, h.arena_nodes()[0])
    print("joint, largest soup (%d 40-gons and %d rectangles per vehicle, soup_cap about %d): peak open list %d, heap_lds %s" % (n_big, n_small, s_max, seen, sorted(planned)))
    assert planned == {256}
    assert seen == 1787 and seen > 256
    joint_equal(got, want, "joint at the largest soup")
    assert fails(n_big, n_small + 1)
    h.close()


# ---------------------------------------------------------------- report


def test_report_cells_and_cycles(handle):
    """Prints, per lds_entries, the cycles per pop and push of the oscillation script with random keys, and the cells that script
    reaches there (the whole table of all scripts: tests/test_heap_cases.py prints it; profiles/heap_limits.txt holds both)."""
    table = {}
    lines = []
    for hl in hc.ALL_HLS:
        ops, ids, keys = hc.script("oscillation", "random", hl)
        t0 = time.perf_counter()
        got, cyc_pop, cyc_push = handle.heap_script(ops, ids, keys, lds_entries=hl)
        dt = time.perf_counter() - t0
        out, cells = hc.model_cells(ops, ids, keys, [hl])
        assert got.tolist() == out
        table[hl] = cells[hl]
        lines.append("lds_entries %5d: %6d operations, %6.0f cycles per pop, %6.0f per push, call %.3f s" % (hl, len(ops), cyc_pop, cyc_push, dt))
    print("\n" + "\n".join(lines))
    print(hc.format_cell_table(table))
