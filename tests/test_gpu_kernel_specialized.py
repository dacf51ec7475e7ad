"""The two instantiations of every search kernel (csrc/pdmpc_device.h: ProductSwitches): the product one, with the debug and test
switches compiled in at their defaults, and the generic one (`_any`), which reads them from KernelArgs.  Both plan like the oracle,
byte for byte, and the launch picks the product instantiation exactly when its switches are the compiled-in ones.

Every test proves which instantiation ran from the "pdmpc LDS layout" line (PDMPC_TUNING debug_lds=1), which ends on the kernel's
name.  Problems and sizes are those of tests/test_gpu_kernel_matrix.py; per variant one batch and its oracle records are computed
once and shared.
"""
import functools
import re

import numpy as np
import pytest

from pdmpc.backend import Handle

import problems
from test_gpu_kernel_matrix import THREADS, TIED_REALISTIC, VARIANTS, bulk_probe, first_true, set_tuning, soup_batch, unbounded, variant_problems, with_soup
from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu

# variant of the matrix -> the kernel it runs
KERNELS = {"bulk": "pdmpc_bulk_kernel", "wide": "pdmpc_bulk_kernel_wide", "sat1": "pdmpc_bulk_kernel_sat", "compact": "pdmpc_bulk_kernel_compact"}
NAMES = list(KERNELS)
KERNEL_LINE = re.compile(r"pdmpc LDS layout[^\n]* kernel (\w+)")


def _oracle():
    from oracle import oracle

    return oracle


def kernels_run(capfd):
    """The kernel names of the layout lines since the last read."""
    return KERNEL_LINE.findall(capfd.readouterr().err)


def assert_instantiation(capfd, variant, generic):
    names = kernels_run(capfd)
    assert names, "no LDS layout line: the search kernel did not run"
    assert set(names) == {KERNELS[variant] + ("_any" if generic else "")}, (variant, names)


@functools.lru_cache(maxsize=None)
def batch(variant):
    """A dozen of the variant's problems and the oracle's records (read-only: shared by the tests)."""
    options, mpa, iters = variant_problems(variant, 12)
    _, ref, _ = _oracle().plan_batch(unbounded(options), mpa, iters, n_threads=THREADS)
    ref.setflags(write=False)
    return options, mpa, iters, ref


def plan_batch(options, mpa, iters):
    import copy

    o = copy.copy(options)
    o.max_vehicles = len(iters)
    o.max_nodes = 1 << 15
    h = Handle(o)
    h.upload_mpa(mpa)
    gpu = h.plan_batch(iters)
    h.close()
    return gpu


@pytest.mark.parametrize("variant", NAMES)
def test_batch_parity_on_both_instantiations(variant, monkeypatch, capfd):
    options, mpa, iters, ref = batch(variant)
    set_tuning(monkeypatch, variant)
    capfd.readouterr()
    product = plan_batch(options, mpa, iters)
    assert_instantiation(capfd, variant, generic=False)
    assert_records_equal(product, ref, "product instantiation (%s)" % variant)
    set_tuning(monkeypatch, variant, "generic=1")
    generic = plan_batch(options, mpa, iters)
    assert_instantiation(capfd, variant, generic=True)
    assert generic.tobytes() == product.tobytes()


@functools.lru_cache(maxsize=None)
def step(variant):
    """The two-level coupling DAG of test_gpu_kernel_matrix.test_step_with_predecessors over 12 of the variant's problems, and the
    oracle's records (read-only: shared by the tests)."""
    options, mpa, iters = variant_problems(variant, 12, seed=13)
    preds = [[] for _ in range(4)] + [sorted({i % 4, (i + 1) % 4}) for i in range(8)]
    prob = {"iters": iters, "preds": preds, "fallback": [None] * 12, "level_sizes": [4, 8]}
    ref, _ = _oracle().plan_step(unbounded(options), mpa, prob, n_threads=THREADS)
    ref.setflags(write=False)
    options.max_vehicles = 12
    options.max_nodes = 1 << 15
    return options, mpa, iters, preds, ref


@pytest.mark.parametrize("variant", NAMES)
def test_step_with_predecessors_on_both_instantiations(variant, monkeypatch, capfd):
    """Hand-over of areas, expected areas, arrivals into running and into finished searches."""
    options, mpa, iters, preds, ref = step(variant)
    capfd.readouterr()
    for generic in (False, True):
        set_tuning(monkeypatch, variant, "generic=1" if generic else "")
        h = Handle(options)
        h.upload_mpa(mpa)
        arrivals = 0
        for rep in range(2):
            gpu = h.plan_step(iters, preds, [[] for _ in iters])
            assert_records_equal(gpu, ref, "step %d (%s, generic %d)" % (rep, variant, generic))
            st = h.stats()
            assert st["safe_replans"] == 0
            arrivals += st["speculation_arrivals"]
        h.close()
        assert arrivals > 0
        assert_instantiation(capfd, variant, generic)


@pytest.mark.parametrize("variant", NAMES)
def test_real_ties_reach_the_replay_on_the_product_instantiation(variant, monkeypatch, capfd):
    """force_tie is compiled in as 0: the replay through the binary heap is still reached by searches that meet real ties."""
    mode, mpa_type, _, _, _ = VARIANTS[variant]
    realistic = variant == "wide"
    options = problems.make_options(mode, Hp=5 if realistic else 6, mpa_type=mpa_type)
    mpa = problems.get_mpa(options)
    tied = [problems.symmetric_problem(options, mpa)]
    if realistic:  # (its symmetric problem ties only where the order decides nothing: the matrix test's road problems with hundreds of tied pops as well)
        for seed, v, _ in TIED_REALISTIC[mode]:
            tied.append(problems.problem_set(mode, seed, v + 1, Hp=5, mpa_type=mpa_type)[2][v])
    rng = np.random.default_rng(5)
    tied = [problems.road_problem(rng, options, mpa, convex=(mode == "sat"))] + tied + tied  # (the batch of the matrix test: an ordinary problem, the tied ones twice)
    _, ref, traces = _oracle().plan_batch(unbounded(options), mpa, tied, trace=True)
    assert problems.tied_pops(traces[-1]) > 0
    set_tuning(monkeypatch, variant)
    options.max_vehicles = len(tied)
    options.max_nodes = 1 << 15
    capfd.readouterr()
    h = Handle(options)
    h.upload_mpa(mpa)
    gpu = h.plan_batch(tied)
    st = h.stats()
    h.close()
    assert_instantiation(capfd, variant, generic=False)
    assert_records_equal(gpu, ref, "tied searches (%s)" % variant)
    assert st["queue_fallbacks"] >= 1, st


@pytest.mark.parametrize("variant", ["bulk", "sat1"])
def test_areas_moved_to_l2_select_the_generic_instantiation(variant, monkeypatch, capfd):
    """The kernels whose product instantiation has the maneuver areas in LDS: a soup grown until the areas move to L2 (as
    test_maneuver_areas_move_to_l2_when_the_soup_grows grows it) runs the generic instantiation and plans like the oracle.
    Not covered: the two kernels whose product instantiation has the areas in L2.  The compact layout never puts them in LDS, so
    its launches cannot differ from the constant; a wide automaton (more than 64 trims) small enough to keep its areas in LDS would
    always run pdmpc_bulk_kernel_wide_any, but the only wide automaton there is, the realistic one, never fits them."""
    set_tuning(monkeypatch, variant)
    options, mpa, iters = variant_problems(variant, 3, seed=17)
    options.max_vehicles = 4
    h = Handle(options)
    h.upload_mpa(mpa)
    assert bulk_probe(h, soup_batch(iters, 0), capfd)["areas"] == 1
    n0 = first_true(lambda n: (bulk_probe(h, soup_batch(iters, n), capfd) or {"areas": 0})["areas"] == 0)
    grown = [with_soup(it, n0 + 1) for it in iters]
    capfd.readouterr()
    gpu = h.plan_batch(grown)
    assert_instantiation(capfd, variant, generic=True)
    gpu_small = h.plan_batch(iters)
    assert_instantiation(capfd, variant, generic=False)
    h.close()
    _, ref, _ = _oracle().plan_batch(unbounded(options), mpa, grown, n_threads=THREADS)
    assert_records_equal(gpu, ref, "areas in L2 (%s)" % variant)
    _, ref_small, _ = _oracle().plan_batch(unbounded(options), mpa, iters, n_threads=THREADS)
    assert_records_equal(gpu_small, ref_small, "areas back in LDS (%s)" % variant)


SWITCHES = ["tentative=0", "fast_arrival=0", "speculate=0", "force_tie=1", "debug_tail=1"]


def without_debug_tail(records, Hp):
    """debug_tail leaves counters in the unused last rows of path_nodes (rows Hp + 1 and up): everything else of the records."""
    r = records.copy()
    r["path_nodes"][:, Hp + 1 :, :] = 0
    return r


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("variant", NAMES)
def test_a_switch_off_its_default_selects_the_generic_instantiation(variant, switch, monkeypatch, capfd):
    """On the step with predecessors, where expected areas, the early publication of finished searches and speculation decide the
    path a search takes: the generic instantiation runs its non-default branches and returns the oracle's records."""
    options, mpa, iters, preds, ref = step(variant)
    set_tuning(monkeypatch, variant, switch)
    capfd.readouterr()
    h = Handle(options)
    h.upload_mpa(mpa)
    gpu = h.plan_step(iters, preds, [[] for _ in iters])
    assert h.stats()["safe_replans"] == 0
    h.close()
    assert_instantiation(capfd, variant, generic=True)
    if switch.startswith("debug_tail"):
        gpu, ref = without_debug_tail(gpu, options.Hp), without_debug_tail(ref, options.Hp)
    assert_records_equal(gpu, ref, "%s (%s)" % (switch, variant))
