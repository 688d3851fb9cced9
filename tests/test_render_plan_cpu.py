"""The renderer's launch plan (holo_diffusion_amd/csrc/render_plan.h) and the view-pool workspace layouts
(viewpool_layout.h) swept on the CPU.

tests/cpu/render_plan_check.cpp is a stand-alone program (its own main, no HIP, nothing loaded into Python), compiled under
AddressSanitizer and UndefinedBehaviorSanitizer.  Its header lists the sweep and the checks it makes from each plan's own
fields; it must print tests/golden/render_plan_table.txt byte for byte.

How the golden table was recorded: from the commit BEFORE the plan existed (153c9c7), never from the code under test, by a
throw-away recorder that is not part of the repository.  That commit's sources were built twice against a copy of
tests/emu/emu_runtime.h whose HOLO_LAUNCH runs nothing and hands the kernel's name (template arguments as the compiler
prints them), grid, workgroup size and the launch parameters' n_cams, n_tiles, xcd, tile_ctr != null, tail_quads and rgb
pointer to a hook: once as the emulation build (the emu=1 lines) and once with EMU_BUILD forced to false as its only other
edit (the emu=0 lines).  The recorder walked the case list of render_plan_check.cpp through the C ABI: HOLO_NUM_CUS and
one HOLO_RENDER* variable set, holo_ctx_create, holo_renderer_create, the ten parameters, holo_renderer_commit,
holo_renderer_set_compute_dtype for the split cases, then
  ws      holo_render_workspace_bytes (and that holo_render refuses one byte less); in training mode, where there is no
          size query, the smallest workspace holo_render_rays accepts, found by offering the grid's bytes + 0, 256, 512, 768;
  kernel, block, and every field of a `list` line: what the hook saw during holo_render / holo_render_rays, the first camera
          of a launch from its rgb pointer.
Because the hook reads the launch parameters, xcd and tail_quads are recorded for emu=0 as well; no field is left to the GPU
comparison alone.  The `vp` lines are the parent's holo_view_pool_workspace_bytes / holo_view_pool_backward_workspace_bytes.
This tree printed all 5112 lines (537 465 bytes) of that recording unchanged (`render_plan_check --full`).  The committed
table is that recording thinned to 332 lines by a fixed rule (every plan whose index hashes to 0 mod 16 with its lists, every
fourth `vp` line; see `kept` in the program) and closed by a digest line of the WHOLE recording - its lines, bytes and 64-bit
FNV-1a, computed from the recorded file by a script of its own -, so every line of the sweep is still held to the parent's.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "holo_diffusion_amd", "csrc")
HEADERS = ("render_plan.h", "viewpool_layout.h")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("render_plan") / "render_plan_check")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", CSRC,
                            os.path.join(REPO, "tests", "cpu", "render_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return path


def _clean(run):
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stderr, run.stderr[-4000:]


def test_plan_sweep_matches_the_golden_table_and_every_check_holds(exe):
    run = subprocess.run([exe, os.path.join(REPO, "tests", "golden", "render_plan_table.txt")], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "render_plan_check: OK" in run.stdout
    assert "36 instantiations planned, 17 bad plans refused, 0 findings" in run.stdout
    _clean(run)


def test_planted_faults_are_found(exe):
    run = subprocess.run([exe, "--self-test"], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "--self-test: OK (4 planted faults found, nothing else)" in run.stdout
    _clean(run)


def test_plan_headers_are_plain_cpp(tmp_path):
    """render_plan.h / viewpool_layout.h include nothing of HIP or of the emulation runtime: plain g++ compiles them."""
    for name in HEADERS:
        unit = tmp_path / (name + ".cpp")
        unit.write_text('#include "%s"\n' % name)
        build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(unit)],
                               capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-4000:]
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "holo_common.h" not in text and "holo_kernels.h" not in text and "emu_runtime" not in text
