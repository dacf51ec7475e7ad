"""The inputs of tests/test_gpu_heap_limits.py, judged on the CPU (tests/heap_cases.py): the model that counts the device heap's decision
points pops what the oracle's std::priority_queue pops on every script the GPU module runs; the scripts reach every decision point
(cell) of csrc/heap_queue.hpp; and five wrong heaps each pop another sequence on them.  The last is the evidence that the GPU
comparison would notice such a defect: no wrong heap is ever run on the device.
"""
import numpy as np
import pytest

import heap_cases as hc
import joint_reference as jr


def _oracle():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def table_and_pops():
    return hc.cell_table()


def pops_key(kind, family, hl):
    return (kind, family, hl if kind == "oscillation" else 0)


def test_model_equals_the_oracle_on_every_gpu_script(table_and_pops):
    _, pops = table_and_pops
    scripts = hc.distinct_scripts()
    assert {(k, f) for k, f, _, _ in scripts} == {(k, f) for k, f, _ in hc.GPU_CASES}
    total = 0
    for kind, family, (ops, ids, keys), hls in scripts:
        want = _oracle().pq_script(ops, ids, keys)
        assert np.array_equal(pops[pops_key(kind, family, hls[0])], want), (kind, family, hls)
        assert len(ops) <= 300000  # one device call each
        total += len(ops) * len(hls)
    print("%d distinct scripts, %d device calls, %d script operations on the device" % (len(scripts), len(hc.GPU_CASES), total))


def test_plain_model_equals_the_instrumented_one_and_joint_reference(table_and_pops):
    """model_pops (the one the wrong heaps are variations of) on one script of every family and kind, and tests/joint_reference.py's
    restatement on the shortest."""
    _, pops = table_and_pops
    for kind, family, hl in [("fill", f, 64) for f in hc.FAMILIES] + [("oscillation", "zeros", 64), ("oscillation", "random", 2048), ("deep", "low_word", 64)]:
        ops, ids, keys = hc.script(kind, family, hl)
        assert hc.model_pops(ops, ids, keys) == pops[pops_key(kind, family, hl)].tolist(), (kind, family)
    ops, ids, keys = hc.script("oscillation", "five", 1054)
    assert np.array_equal(jr.pq_script(ops, ids, keys), pops[pops_key("oscillation", "five", 1054)])


def test_survey_known_answer():
    ids = [1, 2, 3, 4, 5, 6]
    keys = [1.0, 0.5, 0.5, 0.5, 2.0, 0.5]
    script = ([0] * 6 + [1] * 7, ids + [0] * 7, keys + [0.0] * 7)
    want = [2, 3, 6, 4, 1, 5, -1]
    assert hc.model_pops(*script) == want
    assert hc.model_cells(*script, [64])[0] == want
    assert _oracle().pq_script(*script).tolist() == want


def test_every_cell_is_reached(table_and_pops):
    table, _ = table_and_pops
    print("\n" + hc.format_cell_table(table))
    total = {c: sum(table[hl][c] for hl in table) for c in hc.CELLS}
    assert not [c for c in hc.CELLS if total[c] == 0]
    # the equalities of the round rule: 32 * (hole + 1) + 30 == HL runs the mixed form (HL 1054, second round at hole 31), == HL - 2 the
    # LDS form (HL 64 at the first round, HL 1056 and 2048 at the second)
    assert table[1054]["round_threshold_eq_HL"] > 0
    assert all(table[hl]["round_threshold_eq_HL_minus_2"] > 0 for hl in (64, 1056, 2048))
    # every HL sees both forms of push and pop, the three transition lengths and a lone left child on either side of HL
    for hl in hc.ALL_HLS:
        for c in ("push_hole_lds", "push_hole_hbm", "push_climb_crosses_HL", "pop_form_lds", "pop_form_mixed", "pop_len_HL_minus_1", "pop_len_HL", "pop_len_HL_plus_1",
                  "round_mixed", "lone_taken_lds", "lone_taken_mixed", "lone_child_at_HL_minus_1", "lone_child_in_hbm", "final_climb_crosses_HL"):
            assert table[hl][c] > 0, (hl, c)
    assert table[2048]["pop_rounds_3"] > 0 and table[8192]["pop_rounds_3"] > 0


def test_keys_are_what_the_families_say():
    def bits(k):
        return np.ascontiguousarray(k).view(np.uint64)

    for family in hc.FAMILIES:
        ops, ids, keys = hc.fill_and_drain(family)
        k = keys[ops == 0]
        assert not np.isnan(k).any() and not (k < 0).any()
        if family in hc.TIE_FREE:
            assert len(np.unique(k)) == len(k)
        else:
            assert len(np.unique(k)) < len(k) / 2  # (denormal: 60 % of its keys are one of eight values)
    k = hc.fill_and_drain("random")[2]
    assert (bits(k) & np.uint64(0xFFFFF)).any()  # a full mantissa
    ops, ids, k = hc.fill_and_drain("low_word")
    k = k[ops == 0]
    assert len(np.unique(bits(k) >> np.uint64(32))) == 1 and len(np.unique(k)) == 12
    ops, ids, k = hc.fill_and_drain("powers_of_two")
    assert not (bits(k) & np.uint64(0xFFFFFFFF)).any() and len(np.unique(k[ops == 0])) == 41
    ops, ids, k = hc.fill_and_drain("zeros")
    k = k[ops == 0]
    assert ((k == 0) & np.signbit(k)).sum() > 1000 and ((k == 0) & ~np.signbit(k)).sum() > 1000 and (k > 0).sum() > 1000
    ops, ids, k = hc.fill_and_drain("infinity")
    assert np.isinf(k).sum() > 1000
    ops, ids, k = hc.fill_and_drain("denormal")
    k = k[ops == 0]
    assert (k > 0).all() and (k < 2.2250738585072014e-308).all() and (k <= 8 * hc.DENORMAL_MIN).sum() > 1000
    ops, ids, k = hc.fill_and_drain("huge")
    assert (k[ops == 0] >= 1e308).all() and np.isfinite(k).all()
    ops, ids, k = hc.fill_and_drain("random")
    assert (ids[ops == 0] == 0).sum() > 100 and (ids == 2**31 - 1).sum() > 100
    for family in hc.FAMILIES:  # no other script has a negative zero: (e) can show in `zeros` only
        if family != "zeros":
            for kind, f, (ops, ids, keys), _ in hc.distinct_scripts():
                if f == family:
                    assert not ((keys == 0) & np.signbit(keys)).any()


# the families in which a wrong heap must pop another sequence than the right one, and why the others are exempt
TIED = [f for f in hc.FAMILIES if f not in hc.TIE_FREE]
MUST_SHOW = {
    # (a), (b): `>=` for `>` and the other child among equal siblings change something only where two keys are equal; the scripts of
    # ascending, descending and random have no two equal keys (test_keys_are_what_the_families_say)
    "push_ge": TIED,
    "equal_siblings_left": TIED,
    # (c): without the step the value lands in the parent of the lone child and the child stays; with it the child moves up and the value
    # climbs from the child's place.  Both leave the same heap whenever value.key < child.key, which is every lone step of the
    # descending script (asserted below: `lone_taken_value_not_less` is 0 there)
    "no_lone_left_child": [f for f in hc.FAMILIES if f != "descending"],
    # (d): shows where two keys that differ have equal high words: low_word (all of them) and denormal (the small ones).  In the other
    # families with ties, dropping the low word keeps every distinct pair of keys distinct and in order (asserted below); in the tie-free
    # families two live keys share a high word only by chance: reported, not required
    "high_word_only": ["low_word", "denormal"],
    # (e): only `zeros` has a -0.0
    "negative_zero_less": ["zeros"],
}


def scripts_of(family):
    out = [("fill", family, 64)]
    if family in hc.OSC_FAMILIES:
        out.append(("oscillation", family, 64))
    if family in hc.DEEP_FAMILIES:
        out.append(("deep", family, 64))
    return out


def test_the_inputs_discriminate(table_and_pops):
    _, pops = table_and_pops
    lines = ["%-20s" % "wrong model \\ family" + "".join("%14s" % f[:13] for f in hc.FAMILIES)]
    for wrong in hc.WRONG_MODELS:
        row = []
        for family in hc.FAMILIES:
            first = None  # the first differing pop over the family's scripts
            for kind, f, hl in scripts_of(family):
                ops, ids, keys = hc.script(kind, f, hl)
                want = pops[pops_key(kind, f, hl)].tolist()
                got = hc.model_pops(ops, ids, keys, wrong=wrong, want=want)
                if got != want:
                    first = "%s@%d" % (kind[:4], len(got))
                    break
            must = family in MUST_SHOW[wrong]
            assert first is not None or not must, (wrong, family)
            row.append(first if first else ("same" if not must else "MISSED"))
        lines.append("%-20s" % wrong + "".join("%14s" % r for r in row))
    print("\n" + "\n".join(lines))
    print("(entry: script kind @ number of pops up to the first one that differs; same: exempt, see MUST_SHOW)")


def test_the_exemptions_hold():
    ops, ids, keys = hc.fill_and_drain("descending")
    assert hc.model_cells(ops, ids, keys, [64])[1][64]["lone_taken_value_not_less"] == 0
    assert hc.model_cells(*hc.fill_and_drain("ascending"), [64])[1][64]["lone_taken_value_not_less"] > 0
    for family in TIED:
        if family in MUST_SHOW["high_word_only"]:
            continue
        for kind, f, hl in scripts_of(family):
            k = np.unique(hc.script(kind, f, hl)[2])
            cut = (k.view(np.uint64) & np.uint64(0xFFFFFFFF00000000)).view(np.float64)
            assert (np.diff(cut) > 0).all(), family  # (np.unique sorts; +0.0 and -0.0 are one value to it, as to the heap)
