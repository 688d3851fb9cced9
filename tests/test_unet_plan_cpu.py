"""The denoiser's planners (holo_diffusion_amd/csrc/unet_plan.cpp, unet_train_plan.cpp) swept on the CPU.

tests/cpu/unet_plan_check.cpp is a stand-alone program (its own main, no HIP, nothing loaded into Python), compiled together
with unet_plan.cpp, unet_train_plan.cpp and conv_plan.cpp under AddressSanitizer and UndefinedBehaviorSanitizer.  It builds
about 200 forward plans on made-up addresses and checks (a) that they equal tests/golden/unet_plan_table.txt, (b) .. (e) that
no launch reads memory another launch was allowed to overwrite, and that the sweep holds every kind of plan; then 288
training plans, (a) against tests/golden/unet_train_plan_table.txt, with (c), (e) and the gradient accounting (f) on the
timeline of the taped forward and the backward ops: the program's header has the list.  `--self-test` damages a good forward
plan twice and a good training plan twice and expects (c), (d) and (f) to name exactly the damaged ops.  Every plan is also
built as a sizing pass, on no workspace, so UBSan sees that pass form its addresses, and every knob set must change some plan.

How the golden tables were recorded: from the PARENT commit's code, not from the code under test.
unet_plan_table.txt: from the commit BEFORE the planner moved into unet_plan.cpp (4021d14).  In a checkout OLD of that
commit, `make -C holo_diffusion_amd/csrc emu` builds tests/emu/libholo_emu.so.  A throw-away recorder of seven lines brought
that commit's planner in by textual inclusion (which reaches its anonymous namespace) and then the check program as it was
when the planner moved:
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
(`./record tests/golden/unet_plan_table.txt` ran checks (b) .. (e) and the coverage condition on that commit's plans: they
held there.)
unet_train_plan_table.txt: from the commit BEFORE the training planner moved into unet_train_plan.cpp (b87f31c), whose
backward launches are closures: opaque, but callable.  The recorder (OLD a checkout of b87f31c; built as above, with
-DCHECK='"<this tree>/tests/cpu/unet_plan_check.cpp"' in place of -I . because OLD has a check program of its own) has
    typedef holo::unetplan::UnetDesc Desc;
    static void set_cus(Desc& d, int cus) { d.num_cus = cus; }
    #include CHECK
behind the #define, and behind that
  * record_train(d, table, batch, ws, t): a HoloUnet u with u.ctx->num_cus = d.num_cus, u.d = d, u.dgrad = table; that
    commit's TrainPlanner(&u, batch, ws, tp).build(); t.b.plan = tp.fwd with bytes = tp.bytes, t.gy_off / gx_off / grad_off
    from tp, t.b.err = holo::get_error() when build() failed; then every closure of tp.bops is called once with a null stream
    and t.blines = g_rec;
  * definitions, in the executable, of the fifteen launchers those closures call - conv_launch, conv_wgrad_launch,
    colsum_launch, gn_bwd_launch, add_launch, split_cat_launch, sumpool2_launch, zero_insert2_launch, conv_dgrad_s2_launch,
    gemm_launch, softmax_rows_launch, attn_ds_launch, transpose_launch, film_bwd_launch, time_embed_bwd_launch - each of
    which appends the bl_* line of its arguments to g_rec and returns 0.  Nothing is dereferenced, no GPU is involved.
    ./record --train > tests/golden/unet_train_plan_table.txt
(`./record` without an argument still prints the forward table of that commit: equal to unet_plan_table.txt.)
`unet_plan_check` without an argument prints this tree's forward table and `unet_plan_check --train` its training table;
each equals its recording byte for byte: no line of either golden table is marked (a trailing " *" would mark one that had to
differ).
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "holo_diffusion_amd", "csrc")
MARKED = 0  # the " *" lines of the two golden tables (above)
UNIT = ("unet_plan.cpp", "unet_train_plan.cpp")  # the planners: plain C++


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unet_plan") / "unet_plan_check")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I", CSRC,
         os.path.join(REPO, "tests", "cpu", "unet_plan_check.cpp")] + [os.path.join(CSRC, name) for name in UNIT] +
        [os.path.join(CSRC, "conv_plan.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _silent(run):
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stderr, run.stderr[-4000:]


def test_plans_equal_the_parents_and_no_launch_reads_what_another_may_overwrite(check_exe):
    golden = [os.path.join(REPO, "tests", "golden", name) for name in ("unet_plan_table.txt", "unet_train_plan_table.txt")]
    for table in golden:
        assert os.path.getsize(table) <= 256 * 1024
    run = subprocess.run([check_exe] + golden, capture_output=True, text=True)
    print(run.stdout[-6000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "unet_plan_check: OK" in run.stdout
    assert f", {MARKED} lines marked" in run.stdout
    _silent(run)


def test_the_checker_reports_the_two_planted_faults_and_nothing_else(check_exe):
    """Two planted faults in a forward plan and two in a training plan."""
    run = subprocess.run([check_exe, "--self-test"], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "unet_plan_check --self-test: OK" in run.stdout
    assert run.stdout.count("as planted") == 4 and "WRONG" not in run.stdout
    _silent(run)


def test_unet_planner_unit_is_plain_cpp():
    """The planners' files include nothing of HIP or of the emulation runtime: plain g++ compiles them."""
    for name in UNIT:
        build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, os.path.join(CSRC, name)],
                               capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
    for name in ("unet_plan.h", "unet_train_plan.h", "bwd_plan.h") + UNIT:
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "holo_common.h" not in text and "emu_runtime" not in text
