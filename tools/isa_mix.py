#!/usr/bin/env python3
"""Instruction mix of one gfx950 kernel, from the assembly the product flags give.

  python tools/isa_mix.py jet_fb.hip jet_fb_x6ILi4ELb1ELi4ELi1ELb1ELb1E
  python tools/isa_mix.py jet_x6_bwd.hip jet_bwd_x6 --loop inner

The translation unit is compiled to assembly (device side only) with exactly the command line the
Makefile would use for its object (`make -n`, so the per-TU flags are the product's), then the
kernel whose mangled name contains the substring is cut out of the listing and its instructions
are classified BY PREFIX: matrix (v_mfma / v_smfmac), other VALU (v_), LDS (ds_), VMEM (global_,
buffer_, flat_, scratch_), the three scalar bookkeeping opcodes s_nop / s_waitcnt / s_barrier,
and the remaining SALU (s_).  It prints the class counts, the 20 most frequent opcodes and the
register / scratch / occupancy lines of the kernel's resource comment.

--loop outer|inner restricts the count to one loop of the kernel: the widest (outer) or narrowest
(inner) backward branch span that holds matrix instructions -- the tile loop of an unrolled
kernel, the layer loop of a rolled one.  Static counts: a straight-line body's are its dynamic
counts per trip, anything behind a branch is counted once.
"""
import argparse
import collections
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "insr-pde_amd", "csrc")

CLASSES = ("MFMA", "VALU", "SALU", "LDS", "VMEM", "s_nop", "s_waitcnt", "s_barrier", "other")
VMEM_PREFIXES = ("global_", "buffer_", "flat_", "scratch_")
RESOURCE_KEYS = ("NumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy", "LDSByteSize",
                 "SGPRSpill", "VGPRSpill")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(VMEM_PREFIXES):
        return "VMEM"
    if op in ("s_nop", "s_waitcnt", "s_barrier"):
        return op
    if op.startswith("s_"):
        return "SALU"
    return "other"


def compile_command(tu, extra):
    """The Makefile's own compile line for the TU's object, turned into a device-only -S."""
    obj = "../lib/obj/" + os.path.splitext(tu)[0] + ".o"
    make = ["make", "-C", CSRC, "-n", "-B", obj]
    if extra:
        make.append("EXTRA=" + extra)
    out = subprocess.run(make, check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if " -c " in l and tu in l]
    if not lines:
        sys.exit(f"isa_mix: the Makefile has no compile line for {tu}")
    words = shlex.split(lines[-1])
    cmd, skip = [], False
    for w in words:
        if skip:
            skip = False
        elif w == "-o":
            skip = True
        elif w != "-c":
            cmd.append(w)
    return cmd + ["--cuda-device-only", "-S"]


def kernels(asm):
    """{name: (body lines, resource comment lines)} of every .amdhsa kernel in the listing."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    lines = asm.splitlines()
    out = {}
    for name in names:
        a = next((i for i, l in enumerate(lines) if l.startswith(name + ":")), None)
        if a is None:
            continue
        b = a
        while b < len(lines) and not lines[b].lstrip().startswith(".Lfunc_end"):
            b += 1
        res = []
        for l in lines[b:b + 80]:
            m = re.match(r"^\s*;\s*(\w+):\s*(\S+)", l)
            if m and m.group(1) in RESOURCE_KEYS:
                res.append(f"{m.group(1)}: {m.group(2)}")
        out[name] = (lines[a + 1:b], res)
    return out


def parse(body):
    """[(kind, text)]: kind 'label' (text = the label) or 'inst' (text = opcode, operands)."""
    items = []
    for l in body:
        s = l.split(";", 1)[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.L\w+):", s)
            if m:
                items.append(("label", m.group(1), ""))
            continue
        m = re.match(r"^(\w+):$", s)
        if m:
            items.append(("label", m.group(1), ""))
            continue
        parts = s.split(None, 1)
        items.append(("inst", parts[0], parts[1] if len(parts) > 1 else ""))
    return items


def pick_loop(items, which):
    at = {t: i for i, (k, t, _) in enumerate(items) if k == "label"}
    spans = []
    for i, (k, op, args) in enumerate(items):
        if k == "inst" and (op.startswith("s_cbranch") or op == "s_branch"):
            tgt = args.strip()
            if tgt in at and at[tgt] < i:
                n = sum(1 for kk, o, _ in items[at[tgt]:i + 1] if kk == "inst" and classify(o) == "MFMA")
                if n:
                    spans.append((i - at[tgt], at[tgt], i))
    if not spans:
        sys.exit("isa_mix: no loop with matrix instructions in this kernel")
    _, a, b = max(spans) if which == "outer" else min(spans)
    return items[a:b + 1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tu", help="translation unit under insr-pde_amd/csrc, e.g. jet_fb.hip")
    ap.add_argument("name", help="substring of the kernel's mangled name")
    ap.add_argument("--loop", choices=("outer", "inner"), help="count one loop's body only")
    ap.add_argument("--extra", default="", help="further compiler flags (the Makefile's EXTRA)")
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--keep", help="write the listing here")
    a = ap.parse_args()

    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            path = a.keep or os.path.join(d, "tu.s")
            subprocess.run(compile_command(a.tu, a.extra) + ["-o", os.path.abspath(path)], check=True, cwd=CSRC)
            asm = open(path).read()
    ks = kernels(asm)
    hits = sorted(n for n in ks if a.name in n)
    if len(hits) != 1:
        sys.exit(f"isa_mix: {len(hits)} kernels match '{a.name}':\n  " + "\n  ".join(hits or sorted(ks)))
    body, res = ks[hits[0]]
    items = parse(body)
    if a.loop:
        items = pick_loop(items, a.loop)
    ops = [op for k, op, _ in items if k == "inst"]
    cls = collections.Counter(classify(op) for op in ops)
    print(f"kernel {hits[0]}" + (f"  ({a.loop} loop)" if a.loop else ""))
    print(f"instructions {len(ops)}")
    for c in CLASSES:
        if cls[c] or c != "other":
            print(f"  {c:<10} {cls[c]:6d}")
    print("top opcodes")
    for op, n in collections.Counter(ops).most_common(20):
        print(f"  {op:<28} {n:6d}")
    print("resources")
    for r in res:
        print("  " + r)


if __name__ == "__main__":
    main()
