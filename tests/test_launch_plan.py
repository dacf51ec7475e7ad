"""The plan of a launch (csrc/launch_plan.hpp), through its window pdmpc_launch_plan_host: no GPU.

tests/golden/launch_plans.json holds the plans of 342 queries as commit c35012512fa0 (the last one with the planning in api.cpp, written
against the handle) computed them: a default-constructed pdmpc_handle -- empty buffers, null stream, no device needed -- was filled with
the query's numbers and handed to that commit's parse_tuning, compute_lds_bulk / compute_lds_sampled / layout_joint, set_launch_args,
launch_policy, bulk_variant and bulk_generic; `slice` restates the two rules of its dispatch() (lines 473 and 476), `kernel` is the name
table of its print_bulk_layout (the sampled and joint kernels by their symbol).  The queries: both checkers, the three automata of
pdmpc.mpa, Hp 2 / 6 / 8 / 16, launch sizes either side of every n_cu rule at n_cu 256, the chained count either side of half the launch,
device_share 1 / 2 / 4, safe or not, arenas of 512 and 2^17 nodes, the tuning strings a test or a benchmark of this repository sets, and
soup_cap / ll_cap / cand_cap either side of every rung of the three layouts' ladders (found by scanning on that commit).  A row's comment
names the lines of that commit's api.cpp the row goes through.  A change of a row is a change of behaviour: it needs a reason of its
own, and a measurement.
"""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

from pdmpc import abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_plans.json")))
QF, PF, ROWS = GOLDEN["query_fields"], GOLDEN["plan_fields"], GOLDEN["rows"]
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -4
SAT, INTERX = 0, 1
SEARCH, SAMPLED, JOINT = 0, 1, 2
HP_MAX, VMAX, JOINT_MAX, WAVE = 16, 8, 4, 64
LDS_MAX = 160 * 1024


def plan(tuning="", **query):
    """(rc, {field: value} incl. kernel, last error) of pdmpc_launch_plan_host"""
    lib = backend.load_library()
    q, p = abi.LaunchQuery(**query), abi.LaunchPlan()
    rc = lib.pdmpc_launch_plan_host(tuning.encode() if tuning is not None else None, ctypes.byref(q), ctypes.byref(p))
    if rc:
        return rc, None, lib.pdmpc_last_error().decode()
    out = {f: getattr(p, f) for f in PF}
    out["kernel"] = p.kernel.decode()
    return rc, out, ""


def base_query(**kw):
    q = dict(checker=INTERX, Hp=8, n_trims=12, n_man=54, n_cu=256, device_share=1, max_nodes=1 << 17, kind=SEARCH, count=20, n_chained=0, soup_cap=300, ll_cap=120, cand_cap=400,
             safe=0)
    q.update(kw)
    return q


def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "pdmpc.h")).read()
    for name, value in (("HP_MAX", HP_MAX), ("VMAX", VMAX), ("JOINT_MAX", JOINT_MAX), ("OK", OK), ("ERR_INVALID", ERR_INVALID), ("ERR_CAPACITY", ERR_CAPACITY), ("CHECK_SAT", SAT),
                        ("CHECK_INTERX", INTERX)):
        m = re.search(r"PDMPC_%s\s*=?\s*\(?(-?\d+)" % name, text)
        assert m and int(m.group(1)) == value, name


def test_every_golden_plan_field_for_field():
    assert len(ROWS) >= 300
    for row in ROWS:
        rc, got, err = plan(row["tuning"], **dict(zip(QF, row["query"])))
        assert rc == row["rc"], row
        if rc:
            assert err == row["error"], row
            continue
        assert [got[f] for f in PF] == row["plan"], (row, dict(zip(PF, row["plan"])), got)
        assert got["kernel"] == row["kernel"], row


def test_golden_covers_every_kernel_every_kind_and_both_errors():
    assert {r["kernel"] for r in ROWS if not r["rc"]} == {"pdmpc_bulk_kernel" + v + g for v in ("", "_wide", "_sat", "_compact") for g in ("", "_any")} | {"pdmpc_sampled_kernel",
                                                                                                                                                         "pdmpc_joint_kernel"}
    kind = QF.index("kind")
    assert {r["query"][kind] for r in ROWS if r["rc"] == ERR_CAPACITY} == {SEARCH, SAMPLED, JOINT}


# ---- properties, computed here from the definitions of csrc/pdmpc_device.h (PDMPC_LKX_*, LdsPathRegion, PDMPC_JOINT_INTS)


def a16(x):
    return (x + 15) & ~15


PATH_BYTES = a16(4 * ((HP_MAX + 2) + 2 * (HP_MAX + 1) + 128 + HP_MAX))
JOINT_INTS = JOINT_MAX * (HP_MAX + 1) + 3 * JOINT_MAX + HP_MAX + 1


def mpa_sizes(q, p):
    words = (q["n_trims"] + 63) // 64
    return [("mask", q["Hp"] * q["n_trims"] * words * 8), ("man_index", q["n_trims"] ** 2 * 2), ("pose", q["n_man"] * 32), ("area", q["n_man"] * 3 * VMAX * 16 if p["areas_in_lds"] else 0)]


def fixed_regions(W, RC, P):
    """PDMPC_LKX_*(W, RC, P): (name, offset) of the fixed regions, and PDMPC_LKX_FIXED_END"""
    threads = W * WAVE
    sizes = [("ref", 3 * HP_MAX * 8), ("shape", W * (2 * VMAX + 1) * 16), ("path", PATH_BYTES), ("cand", a16(12 * threads)), ("expand", 2 * HP_MAX * HP_MAX * 8 + 16 * 16),
             ("bk_near_key", a16(P * threads * 8)), ("bk_near_id", a16(P * threads * 4)), ("bk_ready", RC * 8), ("bk_hist", 3072 * 4), ("bk_misc", 2048),
             ("bk_pshape", a16(HP_MAX * VMAX * 16 + HP_MAX * 4 + HP_MAX * 8 + HP_MAX * 4)), ("bk_reach", HP_MAX * 4 * 8 + 3 * HP_MAX * 4 + 16 + 32 + 64)]
    off, out = 0, []
    for name, size in sizes:
        out.append((name, off, size))
        off += size
    return out, off


def regions(q, p):
    """[(name, offset, bytes)] of the plan's kind"""
    soup = max(q["soup_cap"], 1) * 16
    if q["kind"] == SEARCH:
        fixed, end = fixed_regions(*((8, 512, 2) if p["compact"] else (16, 2048, 4)))
        for name, off, _ in fixed:
            assert p[name] == off, (name, q)  # the kernel addresses these with immediates
        assert p["reach"] == end and p["tree16"] == p["bk_hist"]
        lists = (max(q["soup_cap"], 1) + (0 if p["reach_shared"] else (q["Hp"] - 1) * max(q["ll_cap"], 0))) * 2 if q["checker"] == INTERX else 0
        sizes = dict(mpa_sizes(q, p) + [("reach", lists), ("soup", soup), ("vstate", p["NV"]), ("nodes", p["NL"] * 64)])
        return fixed + [(n, p[n], s) for n, s in sizes.items()]
    if q["kind"] == SAMPLED:
        sizes = dict(mpa_sizes(q, p) + [("ref", 3 * HP_MAX * 8), ("shape", (2 * VMAX + 1) * 16), ("path", PATH_BYTES), ("soup", soup), ("cand", a16(max(q["cand_cap"], 1) * 4)),
                                        ("expand", 2 * HP_MAX * HP_MAX * 8 + 16 * 16), ("tree16", a16(288 * 18 * 2)), ("rand", a16(q["Hp"] * 250 * 8))])
    else:
        sizes = dict(mpa_sizes(q, p) + [("ref", JOINT_MAX * 3 * HP_MAX * 8), ("shape", JOINT_MAX * 2 * VMAX * 16), ("ints", JOINT_INTS * 4), ("succ", JOINT_MAX * q["n_trims"] * 4),
                                        ("soup", soup), ("heap_key", p["heap_lds"] * 8), ("heap_id", p["heap_lds"] * 4)])
    return [(n, p[n], s) for n, s in sizes.items()]


def test_properties_of_every_golden_plan_that_fits():
    checked = 0
    for row in ROWS:
        q = dict(zip(QF, row["query"]))
        rc, p, _ = plan(row["tuning"], **q)
        if rc:
            continue
        checked += 1
        regs = sorted(regions(q, p), key=lambda r: (r[1], r[2]))
        for name, off, size in regs:
            assert off % 16 == 0, (name, row)
            assert off + size <= p["total"], (name, row)
        for (n0, o0, s0), (n1, o1, _) in zip(regs, regs[1:]):
            assert o0 + s0 <= o1, (n0, n1, row)
        assert p["total"] % 16 == 0 and p["total"] <= (LDS_MAX // 2 if p["compact"] else LDS_MAX), row
        if q["kind"] == JOINT:
            assert p["heap_lds"] >= 256 and p["heap_lds"] % 64 == 0 and p["n_helpers"] == 0, row
            continue
        assert p["bk_ready_cap"] <= 3 * WAVE * p["n_waves"], row
        assert p["bk_round"] <= p["ready"] // 2 - 16, row
        assert 0 <= p["bk_helpers_first"] <= p["n_helpers"], row
        if q["safe"] or q["kind"] != SEARCH:
            assert p["n_helpers"] == 0, row
        if q["kind"] == SEARCH:
            assert p["NL"] <= q["max_nodes"] and p["NV"] <= q["max_nodes"] and p["NV"] % 16 == 0, row
    assert checked >= 300


def first_soup_where(pred, tuning="", lo=1, hi=12000):
    """the first soup_cap at which pred(rc, plan) holds (a rung once left is not taken again: bisection)"""
    assert not pred(*plan(tuning, **base_query(soup_cap=lo))[:2]) and pred(*plan(tuning, **base_query(soup_cap=hi))[:2])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(*plan(tuning, **base_query(soup_cap=mid))[:2]) else (mid, hi)
    return hi


LAYOUT_KIND = ("compact", "areas_in_lds", "reach_shared")


def test_the_ladder_of_the_search_layout():
    """InterX, single_speed, Hp 8: a growing soup moves the maneuver areas to L2, then shares the boundary's reach list, then does not fit;
    the plan one column below each rung differs from the plan at it in exactly that respect."""
    to_l2 = first_soup_where(lambda rc, p: rc or not p["areas_in_lds"])
    shared = first_soup_where(lambda rc, p: rc or p["reach_shared"])
    refused = first_soup_where(lambda rc, p: rc != 0)
    assert 1 < to_l2 < shared < refused
    for at, changed in ((to_l2, {"areas_in_lds": (1, 0)}), (shared, {"reach_shared": (0, 1)})):
        (_, below, _), (_, here, _) = plan(**base_query(soup_cap=at - 1)), plan(**base_query(soup_cap=at))
        assert {f: (below[f], here[f]) for f in LAYOUT_KIND if below[f] != here[f]} == changed
        # (with its areas in L2 the one-word InterX kernel runs its generic twin: ProductSwitches::areas_in_lds)
        assert (below["kernel"], here["kernel"]) == (("pdmpc_bulk_kernel", "pdmpc_bulk_kernel_any") if "areas_in_lds" in changed else ("pdmpc_bulk_kernel_any",) * 2)
        assert (below["n_waves"], below["ready"], below["variant"]) == (here["n_waves"], here["ready"], here["variant"])
    rc, _, err = plan(**base_query(soup_cap=refused))
    assert rc == ERR_CAPACITY and err == "obstacle soup (%d columns) + MPA tables do not fit into %d B of LDS" % (refused, LDS_MAX)
    rc, last, _ = plan(**base_query(soup_cap=refused - 1))
    assert rc == OK and last["reach_shared"] == 1 and last["areas_in_lds"] == 0 and last["NL"] >= 16
    # compact=1: the first soup that sends the launch back to the full layout (whose areas are in LDS again)
    full = first_soup_where(lambda rc, p: rc or not p["compact"], tuning="compact=1")
    (_, below, _), (_, here, _) = plan("compact=1", **base_query(soup_cap=full - 1)), plan("compact=1", **base_query(soup_cap=full))
    assert 1 < full < to_l2
    assert (below["compact"], below["areas_in_lds"], below["n_waves"], below["kernel"]) == (1, 0, 8, "pdmpc_bulk_kernel_compact") and below["total"] <= LDS_MAX // 2
    assert (here["compact"], here["areas_in_lds"], here["n_waves"], here["kernel"]) == (0, 1, 16, "pdmpc_bulk_kernel")
    assert {f: here[f] for f in PF} == {f: plan(**base_query(soup_cap=full))[1][f] for f in PF}  # ... the plan of a launch that never asked


@pytest.mark.parametrize("tuning, text", [("rounds=3", "PDMPC_TUNING: unknown key 'rounds'"), ("round", "PDMPC_TUNING: 'round' is not key=value"), ("round=", "PDMPC_TUNING: 'round=' is not key=value"),
                                          ("ready=2k", "PDMPC_TUNING: value of 'ready' is not an integer"), ("compact=2", "PDMPC_TUNING: compact takes -1, 0 or 1"),
                                          ("waves=8,compact=-2", "PDMPC_TUNING: compact takes -1, 0 or 1")])
def test_a_malformed_tuning_string_is_refused(tuning, text):
    rc, _, err = plan(tuning, **base_query())
    assert rc == ERR_INVALID and err == text


def test_tuning_values_are_clamped():
    assert plan("ready=100", **base_query())[1]["ready"] == 256
    assert plan("ready=5000", **base_query())[1]["ready"] == 2048
    assert plan("ready=1000", **base_query())[1]["ready"] == 960  # (a multiple of 64)
    assert plan("tile=5000", **base_query())[1]["bk_tile"] == 768
    assert plan("tile=1", **base_query())[1]["bk_tile"] == 8
    assert plan("waves=99", **base_query())[1]["n_waves"] == 16
    assert plan("waves=1", **base_query())[1]["n_waves"] == 4
    assert plan("spin_limit=1", **base_query())[1]["spin_limit"] == 1024
    assert plan("share_min=1", **base_query())[1]["bk_share_min"] == 32
    assert plan(None, **base_query())[1] == plan("", **base_query())[1] == plan(",,", **base_query())[1]


# the two patterns the GPU tests read the debug_lds line with (test_gpu_kernel_matrix.py, test_gpu_kernel_specialized.py)
LAYOUT_LINE = re.compile(r"pdmpc LDS layout( \(compact\))?: launch (\d+) waves (\d+)(?: areas (\d))?")
KERNEL_LINE = re.compile(r"pdmpc LDS layout[^\n]* kernel (\w+)")

LINE_PROGRAM = r"""
#include "launch_plan.hpp"
int main(int argc, char** argv) {
    Tuning T;
    std::string err;
    if (argc != 4 || !parse_tuning(argv[1], T, err)) return 2;
    LaunchDims d;
    d.checker = PDMPC_CHECK_INTERX, d.Hp = 8, d.n_trims = 12, d.n_man = 54, d.max_nodes = 1u << 17, d.soup_cap = atoi(argv[3]), d.ll_cap = 120, d.cand_cap = 400;
    mpa_table_sizes(d);
    LaunchPlan p;
    if (plan_launch(T, d, kPlanSearch, atoi(argv[2]), 0, false, p, err)) return 3;
    fputs(format_bulk_layout(p, atoi(argv[2])).c_str(), stdout);
    return 0;
}
"""


def test_the_debug_lds_line_of_a_plan(tmp_path):
    """launch_plan.hpp in a program of its own (host compiler, no HIP header on the command line's include path but the repository's):
    the line format_bulk_layout gives for a plan is what the GPU tests' patterns read, with the plan's numbers."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    cxx = cxx if os.path.exists(cxx) else (shutil.which("clang++") or shutil.which("g++"))
    assert cxx, "no host compiler"
    src = tmp_path / "line.cpp"
    src.write_text(LINE_PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "p-dmpc_amd", "csrc"), str(src), "-o", str(tmp_path / "line")], check=True)
    for tuning, count, soup in (("", 20, 300), ("compact=1", 20, 300), ("", 1280, 300), ("", 20, 2000), ("force_tie=1", 257, 300)):
        line = subprocess.run([str(tmp_path / "line"), tuning, str(count), str(soup)], check=True, capture_output=True, text=True).stdout
        _, p, _ = plan(tuning, **base_query(count=count, soup_cap=soup))
        m = LAYOUT_LINE.match(line)
        assert m and line.endswith("\n") and line.count("\n") == 1, line
        assert (bool(m.group(1)), int(m.group(2)), int(m.group(3))) == (bool(p["compact"]), count, p["n_waves"]), line
        assert (m.group(4) is None) == bool(p["compact"]) and (p["compact"] or int(m.group(4)) == p["areas_in_lds"]), line
        assert KERNEL_LINE.findall(line) == [p["kernel"]], line
        near = (2 if p["compact"] else 4) * p["n_waves"] * WAVE
        assert line.split(": ", 1)[1] == "launch %d waves %d %snear %d ready %d nv %d nl %d total %d kernel %s\n" % (
            count, p["n_waves"], "" if p["compact"] else "areas %d " % p["areas_in_lds"], near, p["ready"], p["NV"], p["NL"], p["total"], p["kernel"])


def test_the_plan_header_names_no_handle_and_no_hip_header():
    text = open(os.path.join(ROOT, "p-dmpc_amd", "csrc", "launch_plan.hpp")).read()
    assert "pdmpc_handle" not in text and "hip_runtime" not in text and "handle.hpp" not in text
