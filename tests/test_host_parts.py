"""The native step controller as stages with narrow state: every stage header of csrc/step_controller.cpp
compiles alone, and the two that restate reference functions do not know the controller (no GPU needed: host compiler, syntax only)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p-dmpc_amd", "csrc")
PARTS = ("step_types.hpp", "step_inputs.hpp", "step_hdv.hpp", "step_priorities.hpp", "step_state.hpp", "step_assembly.hpp", "step_batch.hpp", "step_prepare.hpp")


def test_every_stage_compiles_alone_without_unused_functions():
    """`make host-parts`: each header as a translation unit of its own, then step_controller.cpp, under -Wall -Wunused-function
    -Wunused-member-function -Werror -- a stage names only the stages above it --, then all of them as one text without the `inline` and
    `[[maybe_unused]]` markers that those warnings pass over: no helper or member function of any stage is unused."""
    run = subprocess.run(["make", "-s", "-C", CSRC, "host-parts"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert [line.split()[-1] for line in run.stdout.splitlines() if line.startswith("ok")] == list(PARTS) + ["step_controller.cpp", "merged"], run.stdout


def test_inputs_and_priorities_do_not_know_the_controller():
    """What a step reads of the traffic, and couplings -> a prioritization, take the parts of the state they read (or plain arrays):
    the controller is not named in either file, so a signature there says what the stage depends on.  Nor does the HDV stage know it
    or the handle: the device calls reach its batch path as a callable.  (Its refusals keep their texts, which name entry points
    -- pdmpc_controller_set_hdvs and others --, so there the type's name is looked for as a whole word.)"""
    for name in ("step_inputs.hpp", "step_priorities.hpp"):
        assert "pdmpc_controller" not in open(os.path.join(CSRC, name)).read(), name
    hdv_stage = open(os.path.join(CSRC, "step_hdv.hpp")).read()
    assert not re.search(r"\bpdmpc_controller\b", hdv_stage) and "pdmpc_handle" not in hdv_stage and "pdmpc_group" not in hdv_stage
