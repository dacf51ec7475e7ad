"""Build-time properties of the two instantiations of every search kernel (no GPU needed: hipcc cross-compiles gfx950 code):
the register budget of tests/test_build.py for all eight, and what the product instantiations are there for -- fewer spilled scalar
registers and fewer reloads of them (v_readlane) in the round loop and its check-item loops (DESIGN.md section 3.9,
tools/spill_report.py)."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PRODUCT = ("pdmpc_bulk_kernel", "pdmpc_bulk_kernel_wide", "pdmpc_bulk_kernel_sat", "pdmpc_bulk_kernel_compact")

# v_readlane in the round loop of pdmpc_bulk_kernel before it had two instantiations, and with nothing but the switches and the
# areas' place made constants (both from the same compiler): the generic twin may not exceed the first, the product one not the second
ROUND_LOOP_RELOADS_BEFORE = 1171
ROUND_LOOP_RELOADS_SWITCHES_ONLY = 857
CHECK_ITEM_RELOADS = 8

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")


@needs_hipcc
@pytest.mark.timeout(900)
def test_all_eight_kernels_fit_their_budget_and_the_product_ones_spill_fewer_scalars():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resources", "RESOURCE_SRCS=bulk_kernel.hip bulk_kernel_wide.hip bulk_kernel_sat.hip bulk_kernel_compact.hip"], capture_output=True, text=True,
                         check=True).stdout
    seen = {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    for product in PRODUCT:
        generic = product + "_any"
        for kernel in (product, generic):
            assert kernel in seen, seen.keys()
            assert seen[kernel]["scratch"] == 0 and seen[kernel]["vgpr_spill"] == 0, (kernel, seen[kernel])
            assert seen[kernel]["vgprs"] <= (168 if "_sat" in kernel else 128), (kernel, seen[kernel])
        assert seen[product]["sgpr_spill"] < seen[generic]["sgpr_spill"], (product, seen[product], seen[generic])


def spill_report():
    spec = importlib.util.spec_from_file_location("spill_report", os.path.join(ROOT, "tools", "spill_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_hipcc
@pytest.mark.timeout(900)
def test_reloads_in_the_round_loop_and_the_check_item_loops():
    infos = {i["kernel"]: i for i in spill_report().run("bulk_kernel.hip")}
    product, generic = infos["pdmpc_bulk_kernel"], infos["pdmpc_bulk_kernel_any"]
    print({k: (v["sgpr_spills"], v["round_loop"]) for k, v in infos.items()})
    # (the report's check-item loops: the helper workgroups' copy of bk_check_items lies outside the round loop, the owner's inside it)
    for info in (product, generic):
        check = [lp for lp in info["pass_loops"] if lp["kind"] == "check"]
        assert len([lp for lp in check if not lp["in_round_loop"]]) == 1, [(lp["first"], lp["last"]) for lp in check]
        info["owner_check"] = [lp for lp in check if lp["in_round_loop"]]
        assert len(info["owner_check"]) >= 1
    assert all(lp["counts"]["v_readlane"] <= CHECK_ITEM_RELOADS for lp in product["owner_check"]), [lp["counts"] for lp in product["owner_check"]]
    assert product["round_loop"]["v_readlane"] <= ROUND_LOOP_RELOADS_SWITCHES_ONLY, product["round_loop"]
    assert generic["round_loop"]["v_readlane"] <= ROUND_LOOP_RELOADS_BEFORE, generic["round_loop"]
