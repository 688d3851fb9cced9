"""The float64 folds of holo_diffusion_amd/csrc/mlp_folds.h and their un-folds, checked on the CPU.

tests/cpu/fold_check.cpp is a stand-alone program (its own main, no HIP, nothing loaded into Python): it checks that
every fold equals its layers and that every un-fold is the adjoint of its fold (see its header for the bounds).  It is built
with AddressSanitizer and UndefinedBehaviorSanitizer, so an index past a padded row or column is a failure too.
test_render_oracle_kat.py::test_collapsed_density_net_matches_uncollapsed checks the same algebra of the oracle in torch.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_folds_equal_their_layers_and_unfolds_are_their_adjoints(tmp_path):
    exe = str(tmp_path / "fold_check")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
         "-I", os.path.join(REPO, "holo_diffusion_amd", "csrc"), os.path.join(REPO, "tests", "cpu", "fold_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "fold_check: OK" in run.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stderr, run.stderr[-4000:]
