#!/usr/bin/env python3
"""Where a search kernel reloads spilled scalar registers (no GPU needed: hipcc cross-compiles the listing).

Compiles one bulk_kernel*.hip to gfx950 assembly with the flags the Makefile builds it with (taken from `make -n`, not copied) and
prints per kernel: SGPR spills, instructions and v_readlane / v_writelane / s_nop in the kernel and in its largest loop (the round
loop), and per pass loop -- the check-item loops, the other loops with at least 200 f64 operations and the ten loops with the most
reloads per instruction -- its length, its reloads and the spill slot (register, lane) of every reload site, so that a block of
kernel arguments reloaded whole for one field shows up as consecutive lanes.  Counts vector lane moves and nothing else.

usage: tools/spill_report.py [bulk_kernel.hip] [--csrc DIR] [--json]

A loop is the span from a label to the last backward branch to it.  Where the compiler re-enters an unrolled check-item body
part-way (a label inside it, branched back to from just behind its end, with the same f64 operations), that is the same loop.
The check-item loops are the copies of one source loop (bk_check_items): among the loops with at least 200 f64 operations and no
such loop inside, those whose f64 count occurs both inside the round loop (the owner's copies) and outside it (the helper
workgroups' copy).  DESIGN.md section 3.9 reads this report;
profiles/scalar_diet.txt holds it for the parent and the result of the change that introduced it.
"""
import argparse
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_MIN = 200  # f64 operations from which a loop is reported as an arithmetic loop
TOP_DENSE = 10


def compile_command(csrc, source):
    """The Makefile's compile line of `source`'s object, as `make -n` prints it."""
    obj = "../../build/obj/%s.o" % source
    out = subprocess.run(["make", "-n", "-B", "-C", csrc, obj], capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        words = shlex.split(line)
        if words and os.path.basename(words[0]).startswith("hipcc") and source in words and "-c" in words:
            return words
    raise RuntimeError("make -n shows no hipcc line for %s" % source)


def listing(csrc, source):
    words = compile_command(csrc, source)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "listing.s")
        cmd = []
        skip = False
        for w in words:
            if skip:
                skip = False
                continue
            if w == "-c":
                continue
            if w == "-o":
                skip = True
                continue
            cmd.append(w)
        cmd += ["--cuda-device-only", "-S", "-o", asm]
        subprocess.run(cmd, cwd=csrc, check=True, capture_output=True)
        with open(asm) as f:
            return f.read().splitlines()


LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
READLANE = re.compile(r"^\s+v_readlane_b32\s+\S+,\s*v(\d+),\s*(\d+)")
INSTR = re.compile(r"^\s+([a-z]\w+)")


def kernels_of(lines):
    """{kernel name: its instruction lines and labels} for every .amdhsa_kernel of the listing, in order; and the metadata's spill counts."""
    names = [m.group(1) for m in (re.match(r"^\s+\.amdhsa_kernel\s+(\w+)", l) for l in lines) if m]
    spills = {}
    name = None
    for l in lines:
        m = re.match(r"^\s+\.name:\s+(\w+)", l)
        if m:
            name = m.group(1)
        m = re.match(r"^\s+\.sgpr_spill_count:\s+(\d+)", l)
        if m and name:
            spills[name] = int(m.group(1))
    bodies = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        bodies[name] = lines[start + 1 : end]
    return names, bodies, spills


def analyse(body):
    """Instructions of a kernel body and its loops: [(first, last)] instruction indices, a loop per label with a backward branch."""
    instr = []  # (mnemonic, line)
    label_at = {}
    back = {}
    for l in body:
        m = LABEL.match(l)
        if m:
            label_at[m.group(1)] = len(instr)
            continue
        m = INSTR.match(l)
        if not m or l.lstrip().startswith((".", ";")):
            continue
        b = BRANCH.match(l)
        if b and b.group(1) in label_at:
            back[b.group(1)] = len(instr)  # (the last backward branch to the label closes the loop)
        instr.append((m.group(1), l))
    loops = sorted((label_at[lb], last) for lb, last in back.items())
    return instr, loops


def count(instr, first, last):
    c = {"instructions": last - first + 1, "v_readlane": 0, "v_writelane": 0, "s_nop": 0, "f64": 0}
    for op, _ in instr[first : last + 1]:
        if op.startswith("v_readlane"):
            c["v_readlane"] += 1
        elif op.startswith("v_writelane"):
            c["v_writelane"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op.endswith("_f64") or "_f64_" in op:
            c["f64"] += 1
    return c


def slots(instr, first, last):
    """Reload sites of a span as {vgpr: [lanes]} in the order of the listing."""
    out = {}
    for _, l in instr[first : last + 1]:
        m = READLANE.match(l)
        if m:
            out.setdefault(int(m.group(1)), []).append(int(m.group(2)))
    return out


def lanes_text(lanes):
    """[0, 1, 2, 5, 0, 1] -> '0-2 5 0-1' (runs of consecutive lanes, in listing order)."""
    runs = []
    for x in lanes:
        if runs and x == runs[-1][1] + 1:
            runs[-1][1] = x
        else:
            runs.append([x, x])
    return " ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in runs)


def report(name, body, spill_count):
    instr, loops = analyse(body)
    whole = count(instr, 0, len(instr) - 1)
    rnd = max(loops, key=lambda lp: lp[1] - lp[0]) if loops else None
    info = {"kernel": name, "sgpr_spills": spill_count, "kernel_counts": whole, "round_loop": count(instr, *rnd) if rnd else None, "pass_loops": []}
    counted = [(lp, count(instr, *lp)) for lp in loops]
    # the arithmetic loops: at least F64_MIN f64 operations and no loop of that kind inside
    heavy = [(lp, c) for lp, c in counted if c["f64"] >= F64_MIN]
    heavy = [(lp, c) for lp, c in heavy if not any(o[0] < lp[0] <= o[1] < lp[1] and oc["f64"] == c["f64"] for o, oc in heavy)]  # (second entries into the same body)
    leaf = [(lp, c) for lp, c in heavy if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o, _ in heavy)]
    inside = lambda lp: bool(rnd and rnd[0] <= lp[0] and lp[1] <= rnd[1] and lp != rnd)
    both = {c["f64"] for lp, c in leaf if inside(lp)} & {c["f64"] for lp, c in leaf if not inside(lp)}  # (the same body on both sides)
    check = [(lp, c) for lp, c in leaf if c["f64"] in both]
    other = [(lp, c) for lp, c in leaf if c["f64"] not in both]
    dense = sorted((x for x in counted if x[1]["v_readlane"] > 0 and x[1]["f64"] < F64_MIN), key=lambda x: -x[1]["v_readlane"] / x[1]["instructions"])[:TOP_DENSE]
    for kind, group in (("check", check), ("f64", other), ("dense", dense)):
        for lp, c in group:
            info["pass_loops"].append({"kind": kind, "first": lp[0], "last": lp[1], "in_round_loop": inside(lp), "counts": c,
                                       "slots": {("v%d" % v): lanes for v, lanes in slots(instr, *lp).items()}})
    return info


def print_report(info):
    k, r = info["kernel_counts"], info["round_loop"]
    print("kernel %s: SGPR spills %d" % (info["kernel"], info["sgpr_spills"]))
    print("  %-12s %7s %11s %12s %6s" % ("", "instr", "v_readlane", "v_writelane", "s_nop"))
    print("  %-12s %7d %11d %12d %6d" % ("kernel", k["instructions"], k["v_readlane"], k["v_writelane"], k["s_nop"]))
    if r:
        print("  %-12s %7d %11d %12d %6d" % ("round loop", r["instructions"], r["v_readlane"], r["v_writelane"], r["s_nop"]))
    for kind, title in (("check", "check-item loops"), ("f64", "other loops with >= %d f64 operations" % F64_MIN), ("dense", "the %d other loops with the most reloads per instruction" % TOP_DENSE)):
        print("  %s:" % title)
        for lp in info["pass_loops"]:
            if lp["kind"] != kind:
                continue
            c = lp["counts"]
            print("    instr %6d..%-6d len %5d f64 %4d reloads %4d  %s" % (lp["first"], lp["last"], c["instructions"], c["f64"], c["v_readlane"], "in the round loop" if lp["in_round_loop"] else "outside the round loop"))
            for v, lanes in lp["slots"].items():
                print("        %s lanes %s" % (v, lanes_text(lanes)))


def run(source="bulk_kernel.hip", csrc=None):
    csrc = csrc or os.path.join(ROOT, "p-dmpc_amd", "csrc")
    names, bodies, spills = kernels_of(listing(csrc, source))
    return [report(n, bodies[n], spills.get(n, 0)) for n in names]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("source", nargs="?", default="bulk_kernel.hip")
    ap.add_argument("--csrc", default=None, help="the csrc directory of the checkout to report on (default: this one's)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    infos = run(a.source, a.csrc)
    if a.json:
        json.dump(infos, sys.stdout)
        print()
    else:
        for info in infos:
            print_report(info)
    return 0


if __name__ == "__main__":
    sys.exit(main())
