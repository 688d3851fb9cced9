"""Static bounds on conv_small_kernel's gfx950 code (scripts/rowtile_isa_audit.py: kernels_conv.hip compiled to assembly
with the Makefile's flags).  Needs the ROCm compiler, no GPU.

The kernel's staging - address arithmetic, GroupNorm / FiLM affine, SiLU, padding mask, commit to LDS - runs on the same
vector pipe as its exact-fp32 MFMAs, and the two serialise (tools/coexec_probe.cpp), so what the staging issues is launch
time.  `staging_valu` is the audit's count of vector instructions between a staging group's first activation request and its
first MFMA, on the fp32 instance of the deep levels (fp32 storage, affine + SiLU, no upsampling, whole-group staging):

    before (the kernel with run-time branches, per-chunk 64-bit addresses, the IEEE division)   1946   (same script)
    now                                                                                          723

The bound is the count of this build plus 5 % of compiler drift, and must stay at or below half of the count before.
Registers: every fp32-compute instance keeps within 256 registers with no spilled VGPR and no scratch (two workgroups per CU);
every bf16-compute instance within 168 (three).  No request is waited for on its own: every run of loads that no vmcnt wait
separates holds at least two, and a whole-group instance requests its 16 activation rows, its coefficients and its 16
weight blocks before the first wait."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("rowtile_isa_audit", os.path.join(REPO, "scripts", "rowtile_isa_audit.py"))
audit_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit_mod)

pytestmark = pytest.mark.skipif(audit_mod.find_hipcc() is None, reason="hipcc not found")

DEEP = "BF=0 INBF=0 ACTM=2 UPS=0 WHOLE=1"
BEFORE = 1946
NOW = 723


@pytest.fixture(scope="module")
def audit():
    return audit_mod.audit(audit_mod.compile_asm())


def test_staging_vector_instructions(audit):
    n = audit[DEEP]["staging_valu"]
    bound = int(NOW * 1.05)
    print(DEEP, "staging_valu", n, "bound", bound, "before", BEFORE)
    assert 2 * bound <= BEFORE  # a bound that does not hold the gain is no bound
    assert n <= bound, audit[DEEP]


def test_registers(audit):
    assert DEEP in audit, list(audit)
    for name, r in audit.items():
        print(name, {k: r[k] for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= (168 if name.startswith("BF=1") else 256), (name, r)


def test_requests_are_batched(audit):
    for name, r in audit.items():
        print(name, "loads", r["staging_loads"], "runs", r["load_runs"])
        assert r["load_runs"] and min(r["load_runs"]) >= 2, (name, r)
        if name.startswith("BF=0") and name.endswith("WHOLE=1"):
            assert max(r["load_runs"]) >= 30 and r["staging_loads"] >= 32, (name, r)
