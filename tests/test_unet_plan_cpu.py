"""The denoiser's planner (holo_diffusion_amd/csrc/unet_plan.cpp) swept on the CPU.

tests/cpu/unet_plan_check.cpp is a stand-alone program (its own main, no HIP, nothing loaded into Python), compiled together
with unet_plan.cpp and conv_plan.cpp under AddressSanitizer and UndefinedBehaviorSanitizer.  It builds about 200 plans on
made-up addresses and checks (a) that they equal tests/golden/unet_plan_table.txt, (b) .. (e) that no launch reads memory
another launch was allowed to overwrite, and that the sweep holds every kind of plan: the program's header has the list.
`--self-test` damages a good plan twice and expects (c) and (d) to name exactly the damaged ops.  Every plan is also built
as a sizing pass, on no workspace, so UBSan sees that pass form its addresses, and every knob set must change some plan.

How the golden table was recorded: from the commit BEFORE the planner moved into unet_plan.cpp (4021d14), not from the code
under test.  In a checkout OLD of that commit, `make -C holo_diffusion_amd/csrc emu` builds tests/emu/libholo_emu.so.  A
throw-away recorder of seven lines brings that commit's planner in by textual inclusion (which reaches its anonymous
namespace) and then this tree's check program:
    #include "holo_diffusion_amd/csrc/unet_exec.cpp"
    #define UNET_PLAN_RECORD
    typedef HoloUnet Desc;
    static HoloCtx g_ctx;
    static void set_cus(Desc& d, int cus) { g_ctx.num_cus = cus, d.ctx = &g_ctx; }
    #include "tests/cpu/unet_plan_check.cpp"
built and run as
    g++ -O1 -std=c++17 -DHOLO_EMU -I OLD -I OLD/tests/emu -I OLD/holo_diffusion_amd/csrc -I . -Wno-unknown-pragmas \
        -Wno-attributes recorder.cpp -L OLD/tests/emu -lholo_emu -Wl,-rpath,OLD/tests/emu -pthread -o record
    ./record > tests/golden/unet_plan_table.txt
(`./record tests/golden/unet_plan_table.txt` runs checks (b) .. (e) and the coverage condition on that commit's plans: they
hold there).  `unet_plan_check` without an argument prints this tree's table; the two are equal byte for byte: no line of the
golden table is marked (a trailing " *" would mark one that had to differ).
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "holo_diffusion_amd", "csrc")
MARKED = 0  # the " *" lines of the golden table (above)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unet_plan") / "unet_plan_check")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I", CSRC,
         os.path.join(REPO, "tests", "cpu", "unet_plan_check.cpp"), os.path.join(CSRC, "unet_plan.cpp"),
         os.path.join(CSRC, "conv_plan.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _silent(run):
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stderr, run.stderr[-4000:]


def test_plans_equal_the_parents_and_no_launch_reads_what_another_may_overwrite(check_exe):
    golden = os.path.join(REPO, "tests", "golden", "unet_plan_table.txt")
    assert os.path.getsize(golden) <= 256 * 1024
    run = subprocess.run([check_exe, golden], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "unet_plan_check: OK" in run.stdout
    assert f", {MARKED} lines marked" in run.stdout
    _silent(run)


def test_the_checker_reports_the_two_planted_faults_and_nothing_else(check_exe):
    run = subprocess.run([check_exe, "--self-test"], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "unet_plan_check --self-test: OK" in run.stdout
    assert run.stdout.count("as planted") == 2 and "WRONG" not in run.stdout
    _silent(run)


def test_unet_planner_unit_is_plain_cpp():
    """unet_plan.h / unet_plan.cpp include nothing of HIP or of the emulation runtime: plain g++ compiles them."""
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, os.path.join(CSRC, "unet_plan.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    for name in ("unet_plan.h", "unet_plan.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "holo_common.h" not in text and "emu_runtime" not in text
