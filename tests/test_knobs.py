"""CPU, text level: the HOLO_* environment knobs are ONE table (holo_diffusion_amd/csrc/holo_knobs.h).  The library names and
reads them nowhere else, every name the tests / scripts / tools set is a row of it (a misspelt name would silently test the
default path), and INTEGRATION.md documents every row."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "holo_diffusion_amd", "csrc")
TABLE = os.path.join(CSRC, "holo_knobs.h")

# HOLO_* names that are read OUTSIDE the library, and by whom
OUTSIDE = {
    "HOLO_TEST_EMU": "tests/conftest.py and the test modules: run the gpu tests on the host emulation",
    "HOLO_TEST_EMU_SLOW": "tests/test_generate_cli.py: opt into the 15-minute emulated case",
    "HOLO_TEST_MAX_ITER": "tests/support/generate_cli_emu.py: subsample the sampling chains",
    "HOLO_BENCH_OPS": "bench.py: add the per-op table to a run",
    "HOLO_REFERENCE_ROOT": "oracle/make_golden_config.py: where the reference checkout lies",
    "HOLO_NO_AUTOGRAD_TAPE": "holo_diffusion_amd/unet.py: differentiable forwards without the native tape",
    "HOLO_EMU_CUS": "tests/emu/emu_runtime.h: CU count of the emulated device",
    "HOLO_EMU_TRACE": "tests/emu/emu_runtime.h: trace the emulated launches",
}


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def table_names():
    names = re.findall(r'"(HOLO_[A-Z0-9_]+)"', _read(TABLE))
    assert len(names) == len(set(names)), "a knob is listed twice"
    return names


def test_the_library_names_and_reads_its_knobs_in_the_table_only():
    assert len(table_names()) >= 35
    named, reads = [], []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.splitext(path)[1] not in (".h", ".hip", ".cpp"):
            continue
        text = _read(path)
        if re.search(r'"HOLO_[A-Z0-9_]+"', text):
            named.append(os.path.basename(path))
        if "getenv" in text:
            reads.append(os.path.basename(path))
    assert named == ["holo_knobs.h"], named
    assert reads == ["holo_knobs.h"], reads


def test_every_name_set_outside_the_library_is_a_knob():
    known = set(table_names()) | set(OUTSIDE)
    files = [os.path.join(REPO, "bench.py")] + glob.glob(os.path.join(REPO, "holo_diffusion_amd", "*.py"))
    for d in ("tests", "scripts", "tools", "oracle"):
        for root, _, names in os.walk(os.path.join(REPO, d)):
            files += [os.path.join(root, n) for n in names if os.path.splitext(n)[1] in (".py", ".sh", ".cpp", ".h", ".hip")]
    assert len(files) > 50
    unknown = {}
    for path in files:
        text = _read(path)
        found = set(re.findall(r'''["'](HOLO_[A-Z0-9_]+)["']''', text))  # whole literals: environment names, not constants
        if path.endswith(".sh"):
            found |= set(re.findall(r"\b(HOLO_[A-Z0-9_]+)=", text))  # VAR=value in front of a command
        if found - known:
            unknown[os.path.relpath(path, REPO)] = sorted(found - known)
    assert not unknown, unknown


def test_integration_md_documents_every_knob_in_table_order():
    text = _read(os.path.join(REPO, "INTEGRATION.md"))
    section = text[text.index("## 4. Environment knobs"):]
    documented = re.findall(r"^\| `(HOLO_[A-Z0-9_]+)` \|", section, re.M)
    assert documented == table_names()
