"""unetplan::preactivate_rowtile (holo_diffusion_amd/csrc/unet_plan.cpp), the rewrite pass that lets gn_finalize write the
activated tensor of a deepest-level row-tile convolution once, checked on the CPU.

tests/cpu/rowtile_preact_check.cpp is a stand-alone program (its own main, no HIP, nothing loaded into Python), compiled with
unet_plan.cpp, unet_train_plan.cpp and conv_plan.cpp under AddressSanitizer and UndefinedBehaviorSanitizer.  It builds the
plans of the north-star net (batch 1 and 4), of a net with a GroupNorm group across a concat seam and of a net without an
activated row-tile convolution on made-up addresses, runs the pass behind Planner::build() as unet_exec.cpp does, and checks
which pairs were rewritten, where the scratch lies, that nothing else touches it, that the sizing pass agrees with the placed
one and that every other op is byte-equal to build()'s: the program's header has the list.  (Planner::build() itself is
untouched: tests/test_unet_plan_cpu.py still compares its plans with the golden tables.)"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "holo_diffusion_amd", "csrc")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rowtile_preact") / "rowtile_preact_check")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I", CSRC,
         os.path.join(REPO, "tests", "cpu", "rowtile_preact_check.cpp")] +
        [os.path.join(CSRC, name) for name in ("unet_plan.cpp", "unet_train_plan.cpp", "conv_plan.cpp")] + ["-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_pass_rewrites_the_named_pairs_and_nothing_else(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "rowtile_preact_check: OK" in run.stdout
    assert "north n1: 15 pairs, scratch 262144 bytes" in run.stdout
    assert "north n4: 15 pairs, scratch 1048576 bytes" in run.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stderr, run.stderr[-4000:]


def test_the_debug_line_counts_the_pairs(check_exe):
    """HOLO_DEBUG_PLAN: one new [plan] line per pass with the number of pre-activated pairs; 0 with the knob at 0."""
    env = dict(os.environ, HOLO_DEBUG_PLAN="1")
    run = subprocess.run([check_exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = [line for line in run.stderr.splitlines() if "pairs pre-activated" in line]
    assert lines[0].startswith("[plan] batch 1: 15 finalize + row-tile convolution pairs pre-activated (262144 bytes")
    assert any(line.startswith("[plan] batch 4: 15 ") for line in lines)
    assert lines[-1].startswith("[plan] batch 1: 0 finalize + row-tile convolution pairs pre-activated (0 bytes")
