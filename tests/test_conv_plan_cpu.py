"""The convolution planner (holo_diffusion_amd/csrc/conv_plan.cpp) swept on the CPU.

tests/cpu/conv_plan_check.cpp is a stand-alone program (its own main, no HIP, nothing loaded into Python), compiled together
with conv_plan.cpp under AddressSanitizer and UndefinedBehaviorSanitizer.  It plans about 3000 launches (compute modes,
kernel sizes and strides, grids 2^3 .. 64^3, 4 .. 768 input and 4 .. 256 output channels (a qkv convolution: three times its input), every operand combination the
denoiser builds, batch 1 and 3, 8 .. 256 CUs, the default knobs and every forcing knob of the GPU tests) and checks that
  (a) the plans equal tests/golden/conv_plan_table.txt,
  (b) conv_can_launch - the one check conv_launch makes before it launches - accepts every plan,
  (c) statistics slabs and split-K scratch follow the chosen kernel's rules,
and that every one of the twelve kernels is chosen at least 20 times (see the program's header).

How the golden table was recorded: from the commit BEFORE the planner moved into conv_plan.cpp (0e2dcbb), not from the code
under test.  In a checkout of that commit, `make -C holo_diffusion_amd/csrc emu` builds tests/emu/libholo_emu.so; the same
program, from this tree, is then built against it:
    g++ -O1 -std=c++17 -DCONV_PLAN_RECORD -DHOLO_EMU -I OLD/tests/emu -I OLD/holo_diffusion_amd/csrc \
        tests/cpu/conv_plan_check.cpp -L OLD/tests/emu -lholo_emu -Wl,-rpath,OLD/tests/emu -pthread -o record
    ./record > old_table.txt
and `conv_plan_check` without an argument prints this tree's table.  The two differ in 14 lines, all of one kind: a bf16-mode
1x1x1 convolution of 96 or 160 input channels over at least 4096 voxels, which the old planner put on
conv1x1_bf16_stream_kernel and the old launcher refused (only Cin / 16 = 4, 8, 12, 16 are instantiated).  Those lines hold the
new plan (the row-tile or gather kernel) and end in " *"; every other line is the old table's, byte for byte.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "holo_diffusion_amd", "csrc")
MARKED = 14  # the " *" lines of the golden table (above)


def test_planner_sweep_matches_the_golden_table_and_the_launcher_accepts_every_plan(tmp_path):
    exe = str(tmp_path / "conv_plan_check")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I", CSRC,
         os.path.join(REPO, "tests", "cpu", "conv_plan_check.cpp"), os.path.join(CSRC, "conv_plan.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, os.path.join(REPO, "tests", "golden", "conv_plan_table.txt")], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "conv_plan_check: OK" in run.stdout
    assert f"{MARKED} marked as planned anew" in run.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stderr, run.stderr[-4000:]


def test_planner_unit_is_plain_cpp():
    """conv_plan.h / conv_plan.cpp include nothing of HIP or of the emulation runtime: plain g++ compiles them."""
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, os.path.join(CSRC, "conv_plan.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    for name in ("conv_plan.h", "conv_plan.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "holo_common.h" not in text and "emu_runtime" not in text
