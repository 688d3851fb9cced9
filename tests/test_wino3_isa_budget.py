"""Upper bounds on the bookkeeping conv_wino3_kernel pays on its vector pipe (scripts/wino3_isa_audit.py: kernels_conv3.hip
compiled to gfx950 assembly with the Makefile's flags).  Needs the ROCm compiler, no GPU.

Beside an exact-fp32 MFMA no vector instruction is hidden (tools/mfma_shadow_probe.cpp), so every one that is not
arithmetic of the convolution is step time.  Two groups of them were taken off the vector pipe and a third lost its branches; this file keeps it so.
Instances in the order SKIP=0 XF=1, SKIP=0 XF=0, SKIP=1 XF=1, SKIP=1 XF=0; "before" is the build this change started from.

* accumulator reset: the item's first stage is a copy of the stage body whose opening MFMAs take C = 0 (section
  `first_stage` of the audit), instead of 256 v_accvgpr_write per item.
      accvgpr_write, item + first stage     before 256 / 256 / 256 / 256       now 0 / 0 / 0 / 0
* scalar state spilled to VGPR lanes: the fused-skip section and the epilogue read the launch's constants from the
  kernarg segment where they use them; the residual is requested through a descriptor of zero records when there is
  none (no zeroing moves, no branch).
      sgpr_spill_count                      before 83 / 108 / 128 / 140        now 25 / 21 / 37 / 34
      readlane + writelane per item         before 95 / 114 / 135 / 183        now 31 / 23 / 49 / 42
      valu_total per item                   before 1086 / 1105 / 1226 / 1274   now 735 / 728 / 869 / 863
  "per item" = the item section + what the first-stage copy holds beyond a stage of the loop (first_stage - stage), so
  that nothing escapes the count by moving into the copy.  (Before, there was no copy: the figures are the item section's.)
* the stage body stays ONE basic block (stage_branches = 1, the back edge; before 4 / 3 / 4 / 3): the first-stage copy and
  the loop then meet the register allocator's 256 tied accumulators at one header each.  This guards the structure; it is
  no bound of the halo set-up.  The split of that set-up into a per-item and a per-chunk part that RUN at different
  rates was not built, so - as for any lever that was dropped - its clump count (group0_clump_valu) has no bound here.
  What was kept of it (the thread's (hy, hx) divided out once per workgroup, range tests without branches) is measured in
  profiles/r12_wino3_bookkeeping.txt, not asserted.
* the first-stage copy is judged as a stage, not as part of the item section (scripts/wino3_isa_audit.py says why): it may
  hold what a stage of the loop holds - the 64-bit adds of the weight pointers - and no more of them.

Every bound is the figure of this build plus 16 instructions of compiler drift, and lies strictly below the figure
before."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("wino3_isa_audit", os.path.join(REPO, "scripts", "wino3_isa_audit.py"))
audit_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit_mod)

pytestmark = pytest.mark.skipif(audit_mod.find_hipcc() is None, reason="hipcc not found")

INSTANCES = ["SKIP=0 XF=1", "SKIP=0 XF=0", "SKIP=1 XF=1", "SKIP=1 XF=0"]
SLACK = 16
#                      SKIP=0 XF=1  SKIP=0 XF=0  SKIP=1 XF=1  SKIP=1 XF=0
BEFORE = {
    "accvgpr_write": (256, 256, 256, 256),
    "lanes": (95, 114, 135, 183),
    "valu_total": (1086, 1105, 1226, 1274),
    "sgpr_spill_count": (83, 108, 128, 140),
}
NOW = {
    "accvgpr_write": (0, 0, 0, 0),
    "lanes": (31, 23, 49, 42),
    "valu_total": (735, 728, 869, 863),
    "sgpr_spill_count": (25, 21, 37, 34),
}


def bound(key, inst):
    i = INSTANCES.index(inst)
    b = NOW[key][i] + SLACK
    assert b < BEFORE[key][i], (key, inst, b, BEFORE[key][i])  # a bound that does not hold the gain is no bound
    return b


@pytest.fixture(scope="module")
def audit():
    asm = audit_mod.compile_asm()
    res = audit_mod.audit(asm)
    for name, d in audit_mod.spill_counts(asm).items():  # (the code-object metadata at the end of the listing)
        res[name]["meta"].update(d)
    return res


def per_item(r, key):
    """Item section + what the first-stage copy spends beyond a stage of the loop."""
    s = r["sections"]
    keys = ("readlane", "writelane") if key == "lanes" else (key,)
    return sum(s["item"][k] + max(s["first_stage"][k] - s["stage"][k], 0) for k in keys)


@pytest.mark.parametrize("inst", INSTANCES)
def test_first_stage_copy_is_a_whole_stage(audit, inst):
    s = audit[inst]["sections"]
    assert s["first_stage"]["mfma"] == 512 and s["stage"]["mfma"] == 512, s
    assert s["first_stage"]["scratch"] == 0 and s["first_stage"]["accvgpr_mov"] == 0, s["first_stage"]
    assert s["first_stage"]["u64_add"] <= s["stage"]["u64_add"], (s["first_stage"], s["stage"])


@pytest.mark.parametrize("inst", INSTANCES)
def test_no_accumulator_is_zeroed_by_a_write(audit, inst):
    s = audit[inst]["sections"]
    n = s["item"]["accvgpr_write"] + s["first_stage"]["accvgpr_write"]
    print(inst, "accvgpr_write per item", n)
    assert n <= bound("accvgpr_write", inst), s


@pytest.mark.parametrize("inst", INSTANCES)
def test_lane_traffic_per_item(audit, inst):
    n = per_item(audit[inst], "lanes")
    print(inst, "readlane + writelane per item", n)
    assert n <= bound("lanes", inst), audit[inst]["sections"]


@pytest.mark.parametrize("inst", INSTANCES)
def test_vector_instructions_per_item(audit, inst):
    n = per_item(audit[inst], "valu_total")
    print(inst, "valu_total per item", n)
    assert n <= bound("valu_total", inst), audit[inst]["sections"]


@pytest.mark.parametrize("inst", INSTANCES)
def test_scalar_spills(audit, inst):
    n = audit[inst]["meta"]["sgpr_spill_count"]
    print(inst, "sgpr_spill_count", n)
    assert n <= bound("sgpr_spill_count", inst), audit[inst]["meta"]


@pytest.mark.parametrize("inst", INSTANCES)
def test_stage_body_is_one_block(audit, inst):
    r = audit[inst]
    print(inst, "stage_branches", r["stage_branches"], "group0_clump_valu (not bounded)", r["group0_clump_valu"])
    assert r["stage_branches"] == 1, r["stage_branches"]
