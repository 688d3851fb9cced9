#!/usr/bin/env python3
"""Static audit of conv_small_kernel's gfx950 code (the row-tile convolution of holo_diffusion_amd/csrc/kernels_conv.hip).

Compiles kernels_conv.hip to assembly with the Makefile's flags (or reads a listing given with --asm) and prints, for every
instance of conv_small_kernel in it:

    vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size   the code object's metadata
    staging_valu     vector instructions (v_*, MFMAs excluded) between the FIRST activation request of a staging group - the
                     first buffer / global load inside the K loop, in layout order - and the group's first MFMA: the address
                     arithmetic of the later requests, the activation, the padding mask, the commit's operand moves
    staging_loads    the loads in that window (activations, coefficients, weights)
    load_runs        the lengths of the runs of loads that no `s_waitcnt vmcnt(..)` separates: a run of 1 is a load that is
                     waited for on its own

The K loop is the loop (by the compiler's loop comments) whose blocks hold the most MFMAs; "layout order" follows the
fall-through path, on which a launch with full groups runs.  The same script counts a listing of another revision
(--asm), whatever that revision's template parameters are.

usage: python scripts/rowtile_isa_audit.py [--asm FILE.s] [--json]
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
from wino3_isa_audit import CSRC, find_hipcc, makefile_flags, split_sections  # noqa: E402,F401

LOAD = ("buffer_load", "global_load", "flat_load")


def compile_asm(extra=()):
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernels_conv.s")
        cmd = [hipcc] + makefile_flags() + list(extra) + ["--cuda-device-only", "-S", "kernels_conv.hip", "-o", out]
        res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + res.stderr[-4000:])
        return open(out).read()


def instance_name(symbol):
    """'BF=0 INBF=0 ACTM=2 UPS=0' from the mangled template arguments (one bool: the kernel before the staging was templated)."""
    args = re.search(r"conv_small_kernelI((?:L[bi]\d+E)+)E", symbol).group(1)
    vals = re.findall(r"L[bi](\d+)E", args)
    names = ("BF", "INBF", "ACTM", "UPS", "WHOLE")
    return " ".join("%s=%s" % (n, v) for n, v in zip(names, vals))


def instances(asm):
    out = collections.OrderedDict()
    for m in re.finditer(r"^(_ZN\S*conv_small_kernelI\S*):", asm, re.M):
        sect = asm.index("\t.section", m.end())
        out[instance_name(m.group(1))] = asm[m.end():sect].split("\n")
    return out


def k_loop_ops(lines):
    """The instructions of the K loop in layout order, as (mnemonic, operands)."""
    blocks, cur, pending = [], None, None
    for l in lines:
        s = l.strip()
        m = re.match(r"(?:(\.LBB\d+_\d+):|; (%bb\.\d+):)\s*(?:;\s*(.*))?$", s)
        if m:
            cur = [m.group(1) or m.group(2), 0, None, []]
            blocks.append(cur)
            pending = cur
            s = "; " + (m.group(3) or "")
        if s.startswith(";") and pending is not None:
            mm = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
            if mm:
                pending[1], pending[2] = int(mm.group(2)), mm.group(1)
            mm = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", s)
            if mm:
                pending[1], pending[2] = int(mm.group(1)), pending[0].lstrip(".L")
            continue
        if not s or s.startswith(".") or s.startswith(";"):
            continue
        pending = None
        if cur is None:
            cur = ["entry", 0, None, []]
            blocks.append(cur)
        parts = s.split(None, 1)
        cur[3].append((parts[0], parts[1] if len(parts) > 1 else ""))
    per_header = collections.Counter()
    for _, depth, header, ops in blocks:
        if depth >= 1:
            per_header[header] += sum(1 for op, _ in ops if op.startswith("v_mfma"))
    if not per_header:
        return []
    header = per_header.most_common(1)[0][0]
    return [o for _, depth, h, ops in blocks if depth >= 1 and h == header for o in ops]


def staging_window(ops):
    """From the first load of the K loop to its first MFMA."""
    start = next((i for i, (op, _) in enumerate(ops) if op.startswith(LOAD)), None)
    if start is None:
        return []
    end = next((i for i in range(start, len(ops)) if ops[i][0].startswith("v_mfma")), len(ops))
    return ops[start:end]


def audit(asm):
    res = collections.OrderedDict()
    for name, lines in instances(asm).items():
        win = staging_window(k_loop_ops(lines))
        runs, run = [], 0
        for op, args in win:
            if op.startswith(LOAD):
                run += 1
            elif op == "s_waitcnt" and "vmcnt" in args and run:
                runs.append(run)
                run = 0
        if run:
            runs.append(run)
        res[name] = {
            "staging_valu": sum(1 for op, _ in win if op.startswith("v_") and not op.startswith("v_mfma")),
            "staging_loads": sum(1 for op, _ in win if op.startswith(LOAD)),
            "staging_lane_moves": sum(1 for op, _ in win if op.startswith(("v_readlane", "v_writelane"))),
            "load_runs": runs,
        }
    for m in re.finditer(r"\.name:\s+(_ZN\S*conv_small_kernelI\S*)\n(.*?)\.wavefront_size", asm, re.S):
        name = instance_name(m.group(1))
        for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            mm = re.search(r"\." + key + r":\s*(\d+)", m.group(2))
            if mm and name in res:
                res[name][key] = int(mm.group(1))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    a = ap.parse_args()
    res = audit(open(a.asm).read() if a.asm else compile_asm())
    if a.json:
        print(json.dumps(res))
        return 0
    for name, r in res.items():
        print("conv_small_kernel<%s>  %s" % (name, "  ".join("%s=%s" % kv for kv in r.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
