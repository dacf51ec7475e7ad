"""Build-time properties of the kernels of the choice over the ranks of a group (csrc/group_choice_kernel.hip; no GPU needed: hipcc
cross-compiles gfx950 code objects)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

GROUP_CHOICE_KERNELS = ("pdmpc_group_entries_kernel", "pdmpc_group_cells_kernel", "pdmpc_group_gather_kernel")


@pytest.mark.timeout(300)
def test_group_choice_kernels_use_no_scratch_memory_and_spill_nothing():
    """`make resources` lists group_choice_kernel.hip with the other kernels; its three kernels use no scratch memory and spill no
    register (they are latency-bound passes over a few hundred entries: a spill would be a sign of a mistake, not of pressure)."""
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    with open(os.path.join(CSRC, "Makefile")) as f:
        listed = [line for line in f if line.startswith("RESOURCE_SRCS")]
    assert listed and "group_choice_kernel.hip" in listed[0], "make resources does not cover group_choice_kernel.hip"
    out = subprocess.run(["make", "-s", "-C", CSRC, "resources", "RESOURCE_SRCS=group_choice_kernel.hip"], capture_output=True, text=True, check=True).stdout
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    for kernel in GROUP_CHOICE_KERNELS:
        assert kernel in seen, seen.keys()
        assert seen[kernel] == {"scratch": 0, "vgpr_spill": 0, "sgpr_spill": 0}, (kernel, seen[kernel])
