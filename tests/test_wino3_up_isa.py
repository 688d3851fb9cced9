"""What the compiler makes of conv_wino3_up_kernel, the upsampling form of the three-axis Winograd kernel (kernels_conv3.hip
compiled to gfx950 assembly with the Makefile's flags, split into sections by scripts/wino3_isa_audit.py's helpers).  Needs
the ROCm compiler, no GPU.

The form exists to run the 27 pseudo-taps whose A operands are not identically zero: 18 groups of 12 MFMAs = 216 per stage,
in the stage loop and in the item's first-stage copy (whose opening MFMAs take C = 0), and to read only the 27 live
accumulator sets in the epilogue (108 registers).  Like the generic instances it must stay one stage block without scratch
or spilled vector registers.  The audit script finds the generic instances by their template arguments; this kernel has a
name of its own, so the pattern and the stage size are brought along here."""
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("wino3_isa_audit_up", os.path.join(REPO, "scripts", "wino3_isa_audit.py"))
audit_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit_mod)
audit_mod.STAGE_MFMAS = 216  # (this copy of the module only: the first-stage copy is told from the item section by its size)

pytestmark = pytest.mark.skipif(audit_mod.find_hipcc() is None, reason="hipcc not found")

NAME = r"_ZN\S*conv_wino3_up_kernelE\S*"


@pytest.fixture(scope="module")
def up():
    asm = audit_mod.compile_asm()
    m = re.search(r"^(" + NAME + r"):", asm, re.M)
    assert m, "conv_wino3_up_kernel not found in the listing"
    body = asm[m.end():asm.index("\t.section", m.end())].split("\n")
    sec_ops = audit_mod.split_sections(body)
    counts = {sec: {k: 0 for k in audit_mod.CLASSES} for sec in audit_mod.SECTIONS}
    for sec, op in sec_ops:
        for k, pred in audit_mod.CLASSES.items():
            if pred(op):
                counts[sec][k] += 1
    mm = re.search(r"\.name:\s+" + NAME + r"\n(.*?)\.wavefront_size", asm, re.S)
    assert mm, "no code-object metadata for conv_wino3_up_kernel"
    meta = {key: int(re.search(r"\." + key + r":\s*(\d+)", mm.group(1)).group(1))
            for key in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}
    branches = sum(1 for sec, op in sec_ops if sec == "stage" and op.startswith("s_cbranch"))
    print({s: {k: v for k, v in c.items() if v} for s, c in counts.items()}, meta, "stage_branches", branches)
    return counts, meta, branches


def test_the_generic_pattern_does_not_see_it():
    assert not re.match(r"_ZN\S*conv_wino3_kernelILb([01])ELb([01])E\S*", "_ZN4holo12_GLOBAL__N_120conv_wino3_up_kernelE10ConvParams")


def test_stage_and_first_stage_copy_run_the_live_taps_only(up):
    s = up[0]
    assert s["stage"]["mfma"] == 216 and s["first_stage"]["mfma"] == 216, s
    assert s["item"]["mfma"] == 0 and s["prologue"]["mfma"] == 0, s


def test_one_stage_block(up):
    assert up[2] == 1, up[2]


def test_no_scratch_and_no_vector_spill(up):
    s, meta, _ = up
    assert all(s[sec]["scratch"] == 0 for sec in s), s
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta


def test_accumulator_file_traffic(up):
    """Only the 27 live sets are read (4 registers each), none is zeroed by a write or moved."""
    s = up[0]
    assert s["item"]["accvgpr_read"] == 108, s["item"]
    for sec in ("item", "first_stage", "stage"):
        assert s[sec]["accvgpr_write"] == 0 and s[sec]["accvgpr_mov"] == 0, (sec, s[sec])
    assert s["stage"]["accvgpr_read"] == 0 and s["first_stage"]["accvgpr_read"] == 0, s
