"""Command scripts for the device open list (csrc/heap_queue.hpp) and an instrumented model of it.  TEST INFRASTRUCTURE ONLY: no GPU, no
oracle.

The model is libstdc++'s push_heap / pop_heap as tests/joint_reference.py restates them (std::priority_queue with comp(a, b) =
a.key > b.key), written over two flat lists so that it can count, per operation, which decision points ("cells") of the device code the
operation goes through.  Every cell is a pure function of the script and of HL (lds_entries: how many heap entries live in LDS), so
the table is computed here, without the device: tests/test_heap_cases.py requires every cell to be reached by the scripts that
tests/test_gpu_heap_limits.py runs, and shows that each of five wrong heaps pops another sequence on them.

The device code in the model's terms (heap_queue.hpp):
  push        hole = length before the push; `hole < HL` picks the LDS-only form.  The entry climbs while the parent's key is strictly greater.
  pop         len = length after the pop; `len < HL` picks the LDS-only form.  The hole sinks in rounds of up to five levels; inside a
              mixed pop the round that starts at `hole` runs in the LDS-only form iff 32 * (hole + 1) + 30 < HL (rounds start at hole
              0, then at a node of level 5 (31 .. 62), then of level 10 (1023 .. 2046): the sum is 62, 1054 .. 2046, 32798 ..).
              A lone left child at the bottom is stepped to; the value (the former last entry) is placed at the hole and climbs from
              there unless the key that just moved into the hole's parent says it stays.
"""
import functools
from collections import Counter

import numpy as np

# ---------------------------------------------------------------- the model


def model_pops(ops, ids, keys, wrong=None, want=None):
    """The pops of a script (-1 on an empty queue).  wrong: None or one of WRONG_MODELS.  want: the right pops; the run then stops at
    the first pop that differs and returns what it has (so a wrong model costs as many operations as it needs to show)."""
    if wrong == "high_word_only":  # (d) keys compared by their high 32 bits: the low word is dropped before anything is compared
        keys = (np.ascontiguousarray(keys, dtype=np.float64).view(np.uint64) & np.uint64(0xFFFFFFFF00000000)).view(np.float64)
    if wrong == "negative_zero_less":  # (e) -0.0 < +0.0: no script has a negative key, so -0.0 -> -1.0 is that comparator
        keys = np.ascontiguousarray(keys, dtype=np.float64).copy()
        assert not (keys < 0).any()
        keys[(keys == 0) & np.signbit(keys)] = -1.0
    ge_push = wrong == "push_ge"  # (a) `>=` instead of `>` in __push_heap
    flip = wrong == "equal_siblings_left"  # (b) equal siblings: the left child instead of the right
    no_lone = wrong == "no_lone_left_child"  # (c) the bottom step to a lone left child left out
    K, I, out = [], [], []
    for o, i, k in zip(np.asarray(ops).tolist(), np.asarray(ids).tolist(), np.asarray(keys, dtype=np.float64).tolist()):
        if o == 0:
            pos = len(K)
            K.append(k)
            I.append(i)
            vk, vi = k, i
        else:
            if not K:
                out.append(-1)
            else:
                out.append(I[0])
            if want is not None and out[-1] != want[len(out) - 1]:
                return out
            if not K:
                continue
            vk, vi = K.pop(), I.pop()
            ln = len(K)
            if ln == 0:
                continue
            half = (ln - 1) >> 1
            pos = 0
            while pos < half:
                r = 2 * pos + 2
                if (K[r] >= K[r - 1]) if flip else (K[r] > K[r - 1]):
                    r -= 1
                K[pos] = K[r]
                I[pos] = I[r]
                pos = r
            if not no_lone and (ln & 1) == 0 and pos == (ln - 2) >> 1:
                c = 2 * pos + 1
                K[pos] = K[c]
                I[pos] = I[c]
                pos = c
        while pos > 0:  # std::__push_heap(first, pos, 0, value)
            p = (pos - 1) >> 1
            if (K[p] >= vk) if ge_push else (K[p] > vk):
                K[pos] = K[p]
                I[pos] = I[p]
                pos = p
            else:
                break
        K[pos] = vk
        I[pos] = vi
    return out


WRONG_MODELS = ["push_ge", "equal_siblings_left", "no_lone_left_child", "high_word_only", "negative_zero_less"]

# every cell the scripts must reach (tests/test_heap_cases.py: test_every_cell_is_reached)
CELLS = [
    # push
    "push_hole_lds", "push_hole_hbm", "push_climb_0", "push_climb_some", "push_climb_root", "push_climb_crosses_HL", "push_stops_at_equal",
    # pop: length after the pop, form, rounds
    "pop_len_0", "pop_len_1", "pop_len_2", "pop_form_lds", "pop_form_mixed", "pop_len_HL_minus_1", "pop_len_HL", "pop_len_HL_plus_1",
    "pop_rounds_0", "pop_rounds_1", "pop_rounds_2", "pop_rounds_3",
    "round_lds_in_mixed_pop", "round_mixed", "round_threshold_eq_HL", "round_threshold_eq_HL_minus_2",
    "last_chain_1", "last_chain_2", "last_chain_3", "last_chain_4", "last_chain_5",
    # sibling step
    "sibling_right_gt", "sibling_right_lt", "sibling_equal",
    # lone left child
    "lone_taken_lds", "lone_taken_mixed", "lone_not_taken_lds", "lone_not_taken_mixed", "lone_child_at_HL_minus_1", "lone_child_in_hbm",
    # final placement
    "final_stays_equal", "final_stays_less", "final_climbs", "final_climb_crosses_HL", "final_climb_to_root", "final_hole_0",
    # empty pop
    "pop_empty_start", "pop_empty_middle",
]


def model_cells(ops, ids, keys, hls):
    """(pops, {HL: Counter of cells}) of a script, the right model only.  The heap is run once; each operation is classified per HL."""
    cells = {hl: Counter() for hl in hls}
    common = Counter()  # the cells that do not depend on HL
    hls = list(hls)
    K, I, out = [], [], []
    pushed = False
    for o, i, k in zip(np.asarray(ops).tolist(), np.asarray(ids).tolist(), np.asarray(keys, dtype=np.float64).tolist()):
        if o == 0:
            pushed = True
            hole = pos = len(K)
            K.append(k)
            I.append(i)
            while pos > 0:
                p = (pos - 1) >> 1
                if K[p] > k:
                    K[pos] = K[p]
                    I[pos] = I[p]
                    pos = p
                else:
                    break
            K[pos] = k
            I[pos] = i
            climb = "push_climb_0" if pos == hole else ("push_climb_root" if pos == 0 else "push_climb_some")
            stop_eq = pos > 0 and K[(pos - 1) >> 1] == k
            common[climb] += 1
            if stop_eq:
                common["push_stops_at_equal"] += 1
            for hl in hls:
                if hole < hl:
                    cells[hl]["push_hole_lds"] += 1
                else:
                    cells[hl]["push_hole_hbm"] += 1
                    if pos < hl:
                        cells[hl]["push_climb_crosses_HL"] += 1
            continue
        if not K:
            out.append(-1)
            common["pop_empty_middle" if pushed else "pop_empty_start"] += 1
            continue
        out.append(I[0])
        vk, vi = K.pop(), I.pop()
        ln = len(K)
        if ln == 0:
            common["pop_len_0"] += 1
            continue
        half = (ln - 1) >> 1
        hole = 0
        starts = []
        chain = 0
        n_gt = n_lt = n_eq = 0
        pk = 0.0
        while hole < half:  # one round: up to five levels
            starts.append(hole)
            chain = 0
            while chain < 5 and hole < half:
                r = 2 * hole + 2
                kr, kl = K[r], K[r - 1]
                if kr > kl:
                    n_gt += 1
                    r -= 1
                elif kr < kl:
                    n_lt += 1
                else:
                    n_eq += 1
                pk = K[r]
                K[hole] = pk
                I[hole] = I[r]
                hole = r
                chain += 1
        lone = (ln & 1) == 0 and hole == (ln - 2) >> 1
        if lone:
            c = 2 * hole + 1
            pk = K[c]
            K[hole] = pk
            I[hole] = I[c]
            hole = c
        bottom = pos = hole
        if hole == 0:
            final = "final_hole_0"
        elif pk == vk:
            final = "final_stays_equal"
        elif pk < vk:
            final = "final_stays_less"
        else:
            final = "final_climbs"
            while pos > 0:
                p = (pos - 1) >> 1
                if K[p] > vk:
                    K[pos] = K[p]
                    I[pos] = I[p]
                    pos = p
                else:
                    break
        K[pos] = vk
        I[pos] = vi
        if ln <= 2:
            common["pop_len_%d" % ln] += 1
        common["pop_rounds_%d" % len(starts) if len(starts) <= 3 else "pop_rounds_4_or_more"] += 1
        if starts:
            common["last_chain_%d" % chain] += 1
        common["sibling_right_gt"] += n_gt
        common["sibling_right_lt"] += n_lt
        common["sibling_equal"] += n_eq
        common[final] += 1
        if final == "final_climbs" and pos == 0:
            common["final_climb_to_root"] += 1
        if lone and not vk < pk:
            common["lone_taken_value_not_less"] += 1  # (not a cell of the device code: where leaving the lone step out can show)
        for hl in hls:
            c = cells[hl]
            mixed = ln >= hl
            form = "mixed" if mixed else "lds"
            c["pop_form_" + form] += 1
            if ln == hl - 1:
                c["pop_len_HL_minus_1"] += 1
            elif ln == hl:
                c["pop_len_HL"] += 1
            elif ln == hl + 1:
                c["pop_len_HL_plus_1"] += 1
            if mixed:
                for s in starts:
                    t = 32 * (s + 1) + 30
                    c["round_lds_in_mixed_pop" if t < hl else "round_mixed"] += 1
                    if t == hl:
                        c["round_threshold_eq_HL"] += 1
                    elif t == hl - 2:
                        c["round_threshold_eq_HL_minus_2"] += 1
            c[("lone_taken_" if lone else "lone_not_taken_") + form] += 1
            if lone:
                if bottom == hl - 1:
                    c["lone_child_at_HL_minus_1"] += 1
                elif bottom >= hl:
                    c["lone_child_in_hbm"] += 1
            if final == "final_climbs" and bottom >= hl and pos < hl:
                c["final_climb_crosses_HL"] += 1
    for hl in hls:
        cells[hl].update(common)
    return out, cells


# ---------------------------------------------------------------- keys

FAMILIES = ["equal", "two", "five", "ascending", "descending", "random", "low_word", "powers_of_two", "zeros", "infinity", "denormal", "huge"]
TIE_FREE = ["ascending", "descending", "random"]  # every key of a script differs from every other one
DENORMAL_MIN = 5e-324


class KeyGen:
    """Keys of one family in push order (fixed seed)."""

    def __init__(self, family, seed):
        self.family = family
        self.rng = np.random.default_rng(seed)
        self.at = 0

    def take(self, n):
        f, rng = self.family, self.rng
        j = np.arange(self.at, self.at + n)
        self.at += n
        if f == "equal":
            return np.full(n, 1.7)
        if f == "two":
            return np.array([0.1, 0.2])[rng.integers(0, 2, n)]
        if f == "five":
            return np.array([0.1, 0.2, 0.3, 0.7, 1.1])[rng.integers(0, 5, n)]
        if f == "ascending":
            return (j + 1) * 0.1
        if f == "descending":
            return ((1 << 22) - j) * 0.1
        if f == "random":
            return rng.random(n)  # 53 random bits each
        if f == "low_word":
            return 1.0 + rng.integers(0, 12, n) * 2.0**-52  # only the low 32 bits differ
        if f == "powers_of_two":
            return 2.0 ** rng.integers(-20, 21, n).astype(np.float64)  # only the high 32 bits differ
        if f == "zeros":
            return np.array([0.0, -0.0, 0.0, -0.0, 1e-300, 2.5e-7])[rng.integers(0, 6, n)]
        if f == "infinity":
            return np.array([np.inf, 0.5, 1.0, np.inf, 2.0, 1e300])[rng.integers(0, 6, n)]
        if f == "denormal":
            small = rng.integers(1, 9, n)  # 1 .. 8 units of the smallest denormal: ties, high word 0
            large = rng.integers(1, 1 << 51, n)  # anywhere in the denormal range
            return np.where(rng.random(n) < 0.6, small, large).astype(np.float64) * DENORMAL_MIN
        if f == "huge":
            return 1e308 * (1.0 + 0.1 * rng.integers(0, 6, n))  # up to 1.5e308 < DBL_MAX
        raise ValueError(f)


class Script:
    def __init__(self, family, seed):
        self.kg = KeyGen(family, seed)
        self.ops, self.keys = [], []
        self.length = 0

    def push(self, n=1):
        self.ops.append(np.zeros(n, dtype=np.int32))
        self.keys.append(self.kg.take(n))
        self.length += n

    def pop(self, n=1):
        self.ops.append(np.ones(n, dtype=np.int32))
        self.keys.append(np.zeros(n))
        self.length = max(self.length - n, 0)

    def done(self, special_ids=False):
        ops = np.concatenate(self.ops)
        keys = np.concatenate(self.keys)
        ids = np.where(ops == 0, np.cumsum(ops == 0), 0).astype(np.int32)  # pushes carry 1, 2, 3, ..
        if special_ids:  # ids are payload: 0 and INT32_MAX among them
            at = np.flatnonzero(ops == 0)
            ids[at[::7]] = 0
            ids[at[3::7]] = 2**31 - 1
        return ops, ids, keys


# ---------------------------------------------------------------- script families

FILL_LENGTHS = list(range(1, 200))
DEEP_LENGTHS = [1050, 1053, 1054, 1055, 1056, 1057, 1086, 1118, 1130, 2046, 2047, 2048, 2049, 2050, 2051, 2080, 2120]
DEEP_FAMILIES = ["two", "five", "random", "low_word"]
OSC_FAMILIES = ["five", "random", "low_word", "zeros"]
SMALL_HLS = [64, 66, 94, 96, 126, 128]
LARGE_HLS = [1054, 1056, 2048, 8192]
ALL_HLS = SMALL_HLS + LARGE_HLS
DEEP_HLS = [64] + LARGE_HLS
ROUND_SUMS = [62, 1054, 2046]  # 32 * (hole + 1) + 30 at the first, leftmost second and rightmost second round


@functools.lru_cache(maxsize=None)
def fill_and_drain(family):
    """For L = 1 .. 199: push L entries, pop L + 1 times (the last pop is on the empty queue).  Starts with a pop on the empty queue."""
    s = Script(family, 1000 + FAMILIES.index(family))
    s.pop()
    for L in FILL_LENGTHS:
        s.push(L)
        s.pop(L + 1)
    return s.done(special_ids=(family == "random"))


@functools.lru_cache(maxsize=None)
def oscillation(family, hl):
    """Fill to HL + d (d = -3 .. 3) and to each of ROUND_SUMS +- 2, in ascending order; at each of these lengths alternate push / pop,
    pop / push and push-push-pop-pop, so that an entry stored at the edge of LDS is read back by the very next operation."""
    s = Script(family, 2000 + 16 * FAMILIES.index(family) + ALL_HLS.index(hl))
    targets = sorted({hl + d for d in range(-3, 4)} | {t + e for t in ROUND_SUMS for e in range(-2, 3)})
    for t in targets:
        s.push(t - s.length)
        for _ in range(60):
            s.push()
            s.pop()
        for _ in range(60):
            s.pop()
            s.push()
        for _ in range(40):
            s.push(2)
            s.pop(2)
    s.pop(s.length + 1)
    return s.done()


@functools.lru_cache(maxsize=None)
def deep(family):
    """Fill and drain at lengths around the second-round thresholds (1054 ..) and where a pop takes three rounds (2049 ..)."""
    s = Script(family, 3000 + FAMILIES.index(family))
    for L in DEEP_LENGTHS:
        s.push(L)
        s.pop(L + 1)
    return s.done()


# (kind, family, HL): what tests/test_gpu_heap_limits.py runs, one device call each
GPU_CASES = (
    [("fill", f, hl) for f in FAMILIES for hl in SMALL_HLS]
    + [("oscillation", f, hl) for f in OSC_FAMILIES for hl in ALL_HLS]
    + [("deep", f, hl) for f in DEEP_FAMILIES for hl in DEEP_HLS]
)


def script(kind, family, hl):
    if kind == "fill":
        return fill_and_drain(family)
    if kind == "oscillation":
        return oscillation(family, hl)
    return deep(family)


def distinct_scripts():
    """[(kind, family, script, [HLs it runs at])] over GPU_CASES, each script once"""
    seen = {}
    for kind, family, hl in GPU_CASES:
        key = (kind, family, hl if kind == "oscillation" else 0)
        seen.setdefault(key, (kind, family, script(kind, family, hl), []))[3].append(hl)
    return list(seen.values())


@functools.lru_cache(maxsize=None)
def cell_table():
    """{HL: Counter} summed over GPU_CASES, and the model's pops per distinct script: {(kind, family, hl or 0): pops}"""
    table = {hl: Counter() for hl in ALL_HLS}
    pops = {}
    for kind, family, (ops, ids, keys), hls in distinct_scripts():
        out, cells = model_cells(ops, ids, keys, hls)
        pops[(kind, family, hls[0] if kind == "oscillation" else 0)] = np.array(out, dtype=np.int32)
        for hl in hls:
            table[hl].update(cells[hl])
    return table, pops


def format_cell_table(table):
    hls = sorted(table)
    lines = ["%-32s" % "cell \\ lds_entries" + "".join("%9d" % hl for hl in hls) + "%10s" % "all"]
    extra = sorted({c for hl in hls for c in table[hl]} - set(CELLS))
    for cell in CELLS + extra:
        row = [table[hl][cell] for hl in hls]
        lines.append("%-32s" % cell + "".join("%9d" % v for v in row) + "%10d" % sum(row))
    return "\n".join(lines)
