#!/usr/bin/env python3
"""Is the DEVICE code of the library the same at two revisions?  (development tool, like kernel_resources.py; no GPU needed)

For every file of SRCS_HIP and SRCS_CPP in holo_diffusion_amd/csrc/Makefile, at the base revision (default HEAD) and in
the working tree:  hipcc $(CXXFLAGS) [-x hip] --offload-device-only -S <file>,  drop the lines that contain __hip_cuid_
(a per-compilation id: two compilations of an unchanged file differ in exactly those lines), compare the rest.
A host-only refactor must print `identical` for every file.

    python scripts/device_code_diff.py [--base REV] [--jobs N] [--keep DIR]

Exit status 1 if any listing differs (the two listings of such a file are kept under --keep, default a temporary directory).
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "holo_diffusion_amd/csrc"


def makefile_vars(path):
    text = open(path).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).split()  # noqa: E731
    flags = [f.replace("$(ARCH)", "gfx950") for f in var("CXXFLAGS")]
    extra = {m.group(1): m.group(2).split() for m in re.finditer(r"^(\S+)\.o: CXXFLAGS \+= (.*)$", text, re.M)}
    return var("SRCS_HIP"), var("SRCS_CPP"), flags, extra


def listing(root, name, flags, extra, out):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + extra.get(os.path.splitext(name)[0], [])
    if name.endswith(".cpp"):
        cmd += ["-x", "hip"]
    cmd += ["--offload-device-only", "-S", name, "-o", out, "-w"]
    res = subprocess.run(cmd, cwd=os.path.join(root, CSRC), capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("%s: %s" % (" ".join(cmd), res.stderr[-2000:]))
    return [line for line in open(out) if "__hip_cuid_" not in line]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    keep = args.keep or tempfile.mkdtemp(prefix="device_code_diff_")
    os.makedirs(keep, exist_ok=True)
    base = os.path.join(keep, "base")
    os.makedirs(base, exist_ok=True)
    tar = subprocess.run(["git", "archive", args.base, CSRC, "include"], cwd=REPO, capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
    jobs = []
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        for tag, root in (("base", base), ("new", REPO)):
            hip, cpp, flags, extra = makefile_vars(os.path.join(root, CSRC, "Makefile"))
            for name in hip + cpp:
                out = os.path.join(keep, "%s.%s.s" % (name, tag))
                jobs.append((name, tag, pool.submit(listing, root, name, flags, extra, out)))
        got = {(name, tag): f.result() for name, tag, f in jobs}
    names = sorted({n for n, _ in got})
    bad = 0
    print("device code, %s against the working tree (%d files):" % (args.base, len(names)))
    for name in names:
        a, b = got.get((name, "base")), got.get((name, "new"))
        same = a is not None and a == b
        bad += not same
        print("  %-28s %s" % (name, "identical (%d lines)" % len(a) if same else "DIFFERENT" if a and b else "only at one revision"))
    print("listings kept in %s" % keep if bad else "all identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
