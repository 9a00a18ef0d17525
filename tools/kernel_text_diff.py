#!/usr/bin/env python
"""Do two builds of a .hip file hold the same kernels?  Compares two device-assembly files
(hipcc --offload-arch=gfx950 --cuda-device-only -S, with the flags csrc/Makefile gives the file) kernel by kernel, as text.

Kernels are paired by instantiation: `name<template arguments>`, integers and bools as digits, builtin types as their mangled
letters (f = float, t = the 16-bit storage type of bf16).  A kernel of OLD pairs with the kernel of NEW
that has the same key, or its key extended by zeros (template parameters added later with a false / 0 default);
--alias 'REGEX=REPLACEMENT' rewrites OLD keys first, for kernels that were renamed.  Inside a kernel the symbol's own name and
the numbers of local labels are normalised; everything else, register numbers included, must match for `identical`.  Prints
one row per pair: instruction lines, VGPRs, scratch bytes, spills, occupancy of both sides.  Exit status 1 if a pair differs or
a kernel of OLD has no partner.

usage: python tools/kernel_text_diff.py OLD.s NEW.s [--only REGEX] [--alias 'dq_drop_kernel<(\\d+),(\\d+)>=dq_kernel<\\1,\\2,0,1>' ...]"""
import argparse
import re
import sys


def template_args(rest):
    """The template arguments of a mangled kernel name, `rest` = what follows the name: integers and bools as their digits,
    builtin types as their mangled letters (f = float, t = unsigned short, the bf16 storage type), in order.  Instantiations
    that differ only in a type (ln_bwd_kernel<4, bf16, float, float> / <4, float, float, float>) thereby get keys of their own.
    An argument of any other kind ends the walk: the integers and bools of the whole symbol, as before types were read."""
    args, i = [], 1
    while rest.startswith("I") and i < len(rest) and rest[i] != "E":
        m = re.match(r"L[ib](\d+)E|(DF16b|D[fdhe]|[a-z])", rest[i:])
        if not m:
            return re.findall(r"L[ib](\d+)E", rest)
        args.append(m.group(1) or m.group(2))
        i += m.end()
    return args


def kernels(path):
    """{key: (instruction lines, (VGPRs, scratch, SGPR spills, VGPR spills, LDS, occupancy))} of every kernel in the file."""
    text = open(path).read()
    spills = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)}
    out, sym, lines, labels, res = {}, None, [], {}, {}
    for line in text.split("\n"):
        m = re.match(r"(_Z\w+):", line)
        if m and m.group(1) in spills:                         # (device functions have no metadata entry)
            sym, lines, labels, res = m.group(1), [], {}, {}
        elif sym and not res and not line.startswith(".Lfunc_end"):       # the body
            line = line.split(";")[0].rstrip().replace(sym, "KERNEL")
            line = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line)
            if line.startswith("\t") and not line.startswith("\t."):
                lines.append(line)
        elif sym:                                              # the "; Kernel info:" block behind it
            m = re.match(r"; (NumVgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", line)
            res.update({m.group(1): int(m.group(2))} if m else {"": 0})
            if m and m.group(1) == "Occupancy":
                i, name = 3 if sym.startswith("_ZN") else 2, sym
                while sym[i].isdigit():                        # the last length-prefixed component of the mangled name
                    n = re.match(r"\d+", sym[i:]).group()
                    name, i = sym[i + len(n):i + len(n) + int(n)], i + len(n) + int(n)
                key = name + "<" + ",".join(template_args(sym[i:])) + ">"
                out[key] = (lines, (res["NumVgprs"], res["ScratchSize"], *spills[sym], res["LDSByteSize"], res["Occupancy"]))
                sym = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--alias", action="append", default=[])
    ap.add_argument("--only", default="", help="regex: compare only the kernels of OLD whose key matches")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    bad = 0
    print(f"{'kernel (NEW)':44s} {'lines':>11s}  (VGPRs, scratch, SGPR spills, VGPR spills, LDS, occupancy) old | new   text")
    old = {k: v for k, v in old.items() if re.search(a.only, k)}
    for key, (ol, ores) in sorted(old.items()):
        for al in a.alias:
            pat, rep = al.split("=", 1)
            key = re.sub(pat, rep, key)
        partner = [k for k in new if k == key or re.fullmatch(re.escape(key[:-1]) + r"(,0)*>", k)]
        if len(partner) != 1:
            print(f"{key:44s} no partner in NEW" if not partner else f"{key:44s} ambiguous: {partner}")
            bad += 1
            continue
        nl, nres = new[partner[0]]
        same = ol == nl
        bad += not same or ores != nres
        print(f"{partner[0]:44s} {len(ol):5d} {len(nl):5d}  {ores} | {nres}   {'identical' if same else 'DIFFERENT'}")
    print(f"{len(old)} kernels of OLD, {len(new)} of NEW: " + ("all pairs identical, same resources" if not bad else f"{bad} pairs differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
