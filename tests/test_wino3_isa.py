"""What the compiler makes of conv_wino3_kernel around its stage loop (scripts/wino3_isa_audit.py: kernels_conv3.hip compiled
to gfx950 assembly with the Makefile's flags, every instance split into prologue / item loop outside the stage loop / stage
loop).  Needs the ROCm compiler, no GPU.

Per item the arithmetic needs 256 accumulator reads (each accumulator register leaves the accumulation file once) and,
while the stage body stays one basic block for every chunk, 256 zeroing writes.  Everything else the register allocator
used to add there - accumulators renamed through arch VGPRs, live values parked in the accumulation file, scratch spills,
64-bit address arithmetic for every store - must stay out."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("wino3_isa_audit", os.path.join(REPO, "scripts", "wino3_isa_audit.py"))
audit_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit_mod)

pytestmark = pytest.mark.skipif(audit_mod.find_hipcc() is None, reason="hipcc not found")

INSTANCES = ["SKIP=0 XF=0", "SKIP=0 XF=1", "SKIP=1 XF=0", "SKIP=1 XF=1"]


@pytest.fixture(scope="module")
def audit():
    return audit_mod.audit(audit_mod.compile_asm())


def test_all_four_instances_are_found(audit):
    assert sorted(audit) == INSTANCES


@pytest.mark.parametrize("inst", INSTANCES)
def test_no_scratch_traffic_in_the_item_loop(audit, inst):
    s = audit[inst]["sections"]
    assert s["item"]["scratch"] == 0 and s["stage"]["scratch"] == 0, s


@pytest.mark.parametrize("inst", INSTANCES)
def test_no_64_bit_vector_adds_outside_the_stage_loop(audit, inst):
    assert audit[inst]["sections"]["item"]["u64_add"] == 0, audit[inst]["sections"]["item"]


@pytest.mark.parametrize("inst", INSTANCES)
def test_accumulator_file_traffic_outside_the_stage_loop(audit, inst):
    it = audit[inst]["sections"]["item"]
    moves = it["accvgpr_read"] + it["accvgpr_write"] + it["accvgpr_mov"]
    print(inst, {k: it[k] for k in ("accvgpr_read", "accvgpr_write", "accvgpr_mov")})
    assert it["accvgpr_read"] >= 256  # (the output transform is there at all)
    assert moves <= 256 + 256 + 16, it  # 256 reads + 256 reset writes + 16


@pytest.mark.parametrize("inst", INSTANCES)
def test_stage_loop_is_what_it_was(audit, inst):
    st = audit[inst]["sections"]["stage"]
    assert st["mfma"] == 512, st
    assert st["accvgpr_read"] == 0 and st["accvgpr_write"] == 0 and st["accvgpr_mov"] == 0, st
