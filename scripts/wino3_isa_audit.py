#!/usr/bin/env python3
"""Static audit of conv_wino3_kernel's gfx950 code around its stage loop.

Compiles holo_diffusion_amd/csrc/kernels_conv3.hip to assembly with the Makefile's flags (or reads a listing given with
--asm), splits every conv_wino3_kernel instance by the loop-depth comments the compiler writes

    prologue    blocks in no loop (once per workgroup)
    item        blocks of the item loop (depth 1) outside the stage loop - fused skip, output transform, epilogue, item
                bookkeeping
    first_stage the item's first stage, a copy of the stage body outside the stage loop whose opening MFMAs take C = 0
                (the depth-1 blocks that hold at least half a stage's MFMAs; empty if the kernel has no such copy).
                It is a section of its own, not part of "item": the copy carries what every stage carries (the 64-bit
                adds of the weight pointers among it), and what "item" is judged by - no 64-bit vector add, no
                accumulator move - would otherwise be hidden behind a stage's worth of instructions.  What the copy
                spends BEYOND a stage of the loop belongs to the item (tests/test_wino3_isa_budget.py adds it back).
    stage       the stage loop (the depth-2 loop that holds the 512 MFMAs of a chunk)

and prints, per section, the instruction counts the item boundary is judged by, and `group0_clump_valu`: the vector
instructions between the 16th and the 17th MFMA of the stage loop - the clump behind group 0, where the next stage's halo
addresses are set up (next to the 8 v_pk_add_f32 that form the A operands of group 1) - and `stage_branches`: the
conditional branches inside the stage loop (1 = the back edge alone: the stage body is ONE basic block).
`group0_clump_valu` is a figure to READ, not to assert on: it counts by position, and where the compiler lays the set-up
elsewhere (the XF=1 instances before the straight-line range tests: 8) it counts something else.

usage: python scripts/wino3_isa_audit.py [--asm FILE.s] [--json]
"""
import argparse
import collections
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "holo_diffusion_amd", "csrc")
SECTIONS = ("prologue", "item", "first_stage", "stage")
STAGE_MFMAS = 512
# what is counted: name -> predicate on the mnemonic
CLASSES = collections.OrderedDict(
    [
        ("mfma", lambda op: op.startswith("v_mfma")),
        ("accvgpr_read", lambda op: op.startswith("v_accvgpr_read")),
        ("accvgpr_write", lambda op: op.startswith("v_accvgpr_write")),
        ("accvgpr_mov", lambda op: op.startswith("v_accvgpr_mov")),
        ("v_pk", lambda op: op.startswith("v_pk_")),
        ("v_add_f32", lambda op: op.startswith("v_add_f32") or op.startswith("v_sub_f32")),
        ("v_fmac_f32", lambda op: op.startswith("v_fmac_f32") or op.startswith("v_fma_f32")),
        ("u64_add", lambda op: op.startswith(("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32"))),
        ("readlane", lambda op: op.startswith("v_readlane")),
        ("writelane", lambda op: op.startswith("v_writelane")),
        ("v_mov", lambda op: op.startswith("v_mov_b")),
        ("scratch", lambda op: op.startswith("scratch_")),
        ("buffer_load", lambda op: op.startswith("buffer_load")),
        ("buffer_store", lambda op: op.startswith("buffer_store")),
        ("global_load", lambda op: op.startswith(("global_load", "flat_load"))),
        ("global_store", lambda op: op.startswith(("global_store", "flat_store"))),
        ("valu_total", lambda op: op.startswith("v_") and not op.startswith("v_mfma")),
    ]
)


def makefile_flags():
    """CXXFLAGS of holo_diffusion_amd/csrc/Makefile, with ARCH = gfx950."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


def find_hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def compile_asm(extra=()):
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernels_conv3.s")
        cmd = [hipcc] + makefile_flags() + list(extra) + ["--cuda-device-only", "-S", "kernels_conv3.hip", "-o", out]
        res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + res.stderr[-4000:])
        return open(out).read()


def instances(asm):
    """{'<SKIP, XF>': [lines of the function body], ...} and the metadata lines that follow each body."""
    out = collections.OrderedDict()
    for m in re.finditer(r"^(_ZN\S*conv_wino3_kernelILb([01])ELb([01])E\S*):", asm, re.M):
        end = asm.index(".end_amdhsa_kernel", m.end())
        meta_end = asm.find("\n\t.text", end)
        body_end = asm.index("s_endpgm", m.end())
        # (the last s_endpgm of the function: every path ends in one; take the text up to .section)
        sect = asm.index("\t.section", m.end())
        name = "SKIP=%s XF=%s" % (m.group(2), m.group(3))
        out[name] = (asm[m.end():sect].split("\n"), asm[sect:meta_end if meta_end > 0 else end])
        del body_end
    return out


def split_sections(lines):
    """[(section, mnemonic)] - the section of every instruction.  A block's loop membership is in the comment behind its
    label (or behind `; %bb.N:`): `in Loop: Header=BBx_y Depth=d`, `=>This Loop Header: Depth=d`, `Parent Loop BBx_y Depth=d`
    followed by `=> This Inner Loop Header: Depth=d`."""
    blocks = []  # [label, depth, header (innermost), [mnemonics]]
    cur = None
    pending = None  # a label whose comment continues on the next lines
    for l in lines:
        s = l.strip()
        m = re.match(r"(?:(\.LBB\d+_\d+):|; (%bb\.\d+):)\s*(?:;\s*(.*))?$", s)
        if m:
            label = m.group(1) or m.group(2)
            cur = [label, 0, None, []]
            blocks.append(cur)
            pending = cur
            s = "; " + (m.group(3) or "")
        if s.startswith(";") and pending is not None:
            c = s
            mm = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", c)
            if mm:
                pending[1], pending[2] = int(mm.group(2)), mm.group(1)
            mm = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", c)
            if mm:
                pending[1], pending[2] = int(mm.group(1)), pending[0].lstrip(".L")
            continue
        if not s or s.startswith(".") or s.startswith(";"):
            continue
        pending = None
        if cur is None:
            cur = ["entry", 0, None, []]
            blocks.append(cur)
        cur[3].append(s.split()[0])
    # the stage loop: the depth >= 2 header whose blocks hold the most MFMAs
    per_header = collections.Counter()
    for _, depth, header, ops in blocks:
        if depth >= 2:
            per_header[header] += sum(1 for op in ops if op.startswith("v_mfma"))
    stage_header = per_header.most_common(1)[0][0] if per_header else None
    out = []
    for _, depth, header, ops in blocks:
        sec = "prologue" if depth == 0 else "stage" if (depth >= 2 and header == stage_header) else "item"
        if sec == "item" and 2 * sum(1 for op in ops if op.startswith("v_mfma")) >= STAGE_MFMAS:
            sec = "first_stage"
        out.extend((sec, op) for op in ops)
    return out


def group0_clump(sec_ops):
    """Vector instructions between MFMA 16 and MFMA 17 of the stage loop (in layout order)."""
    n_mfma, valu = 0, 0
    for sec, op in sec_ops:
        if sec != "stage":
            continue
        if op.startswith("v_mfma"):
            n_mfma += 1
            if n_mfma > 16:
                break
        elif n_mfma == 16 and op.startswith("v_"):
            valu += 1
    return valu


def audit(asm):
    res = collections.OrderedDict()
    for name, (lines, meta) in instances(asm).items():
        counts = {sec: collections.OrderedDict((k, 0) for k in CLASSES) for sec in SECTIONS}
        sec_ops = split_sections(lines)
        for sec, op in sec_ops:
            for k, pred in CLASSES.items():
                if pred(op):
                    counts[sec][k] += 1
        md = {}
        for key in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
            mm = re.search(r"\.amdhsa_" + key + r"\s+(\d+)", meta) or re.search(r"\." + key + r":\s*(\d+)", meta)
            if mm:
                md[key] = int(mm.group(1))
        mm = re.search(r"; ScratchSize: (\d+)", meta)
        if mm:
            md["scratch_bytes_per_lane"] = int(mm.group(1))
        res[name] = {"sections": counts, "meta": md, "group0_clump_valu": group0_clump(sec_ops),
                     "stage_branches": sum(1 for sec, op in sec_ops if sec == "stage" and op.startswith("s_cbranch"))}
    return res


def spill_counts(asm):
    """vgpr / sgpr spill counts from the code-object metadata at the end of the listing, by kernel symbol."""
    out = {}
    for m in re.finditer(r"\.name:\s+(_ZN\S*conv_wino3_kernelILb([01])ELb([01])E\S*)\n(.*?)\.wavefront_size", asm, re.S):
        blk = m.group(4)
        d = {}
        for key in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
            mm = re.search(r"\." + key + r":\s*(\d+)", blk)
            if mm:
                d[key] = int(mm.group(1))
        out["SKIP=%s XF=%s" % (m.group(2), m.group(3))] = d
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    a = ap.parse_args()
    asm = open(a.asm).read() if a.asm else compile_asm()
    res = audit(asm)
    for name, d in spill_counts(asm).items():
        if name in res:
            res[name]["meta"].update(d)
    if a.json:
        print(json.dumps(res))
        return 0
    for name, r in res.items():
        print("conv_wino3_kernel<%s>   %s" % (name, "  ".join("%s=%d" % kv for kv in sorted(r["meta"].items()))))
        print("  group0_clump_valu=%d  stage_branches=%d" % (r["group0_clump_valu"], r["stage_branches"]))
        print("  %-14s" % "class" + "".join(" %11s" % s for s in SECTIONS))
        for k in CLASSES:
            print("  %-14s" % k + "".join(" %11d" % r["sections"][s][k] for s in SECTIONS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
