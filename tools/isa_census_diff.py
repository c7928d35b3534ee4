#!/usr/bin/env python3
"""Per-kernel census of two hipcc -S listings of the same file, side by side: VGPRs, SGPRs, scratch bytes, LDS bytes, instruction count and
whether the multiset of opcodes (mnemonic counts) is the same.  Register naming and instruction order are not looked at.  For a refactor that
must leave the kernels as they are.  usage: python tools/isa_census_diff.py parent.s new.s [more pairs ...] [--md]
(make the listings as tools/isa_count.py's docstring says, one from each commit; names are demangled with llvm-cxxfilt when it is there)"""
import collections
import os
import re
import subprocess
import sys


def census(path):
    """{mangled kernel name: (vgprs, sgprs, scratch, lds, Counter of mnemonics)}"""
    lines = open(path).read().splitlines()
    kernels = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel")}
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\S*):", lines[i])
        if not m or m.group(1) not in kernels:
            i += 1
            continue
        name, ops, meta = m.group(1), collections.Counter(), {}
        i += 1
        while not lines[i].startswith(".Lfunc_end"):
            t = lines[i].strip()
            if t and not t.startswith((";", ".")) and not t.endswith(":"):
                ops[t.split()[0]] += 1
            i += 1
        while i < len(lines) and not re.match(r"^_Z\S*:", lines[i]):
            mm = re.match(r"^; (NumVgprs|TotalNumSgprs|ScratchSize|LDSByteSize): (\d+)", lines[i])
            if mm and mm.group(1) not in meta:
                meta[mm.group(1)] = int(mm.group(2))
            i += 1
        out[name] = (meta.get("NumVgprs"), meta.get("TotalNumSgprs"), meta.get("ScratchSize"), meta.get("LDSByteSize"), ops)
    return out


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            got = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return {n: re.sub(r"\(.*", "", g.replace("(anonymous namespace)::", "")).replace("void ", "") for n, g in zip(names, got)}
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


args = [a for a in sys.argv[1:] if a != "--md"]
md = "--md" in sys.argv
unequal = 0
if md:
    print("| file | kernel | VGPR parent / new | SGPR parent / new | scratch parent / new | LDS parent / new | instructions parent / new | opcode multiset | equal |")
    print("|---|---|---|---|---|---|---|---|---|")
for a, b in zip(args[0::2], args[1::2]):
    ca, cb = census(a), census(b)
    nice = demangle(sorted(set(ca) | set(cb)))
    for k in sorted(set(ca) | set(cb), key=lambda n: nice[n]):
        if k not in ca or k not in cb:
            unequal += 1
            print(("| %s | `%s` | only in %s |||||| no |" if md else "%s %s only in %s") % (os.path.basename(a), nice[k], "parent" if k in ca else "new"))
            continue
        (va, sa, xa, la, oa), (vb, sb, xb, lb, ob) = ca[k], cb[k]
        same_ops = oa == ob
        eq = same_ops and (va, sa, xa, la) == (vb, sb, xb, lb)
        unequal += not eq
        na, nb = sum(oa.values()), sum(ob.values())
        if md:
            print("| %s | `%s` | %s / %s | %s / %s | %s / %s | %s / %s | %d / %d | %s | %s |" % (os.path.basename(a), nice[k], va, vb, sa, sb, xa, xb, la, lb, na, nb,
                                                                                              "same" if same_ops else "differs", "yes" if eq else "NO"))
        else:
            print("%-18s %-60s vgpr %3s/%3s sgpr %3s/%3s scratch %s/%s lds %s/%s instr %5d/%5d %s" % (os.path.basename(a), nice[k], va, vb, sa, sb, xa, xb, la, lb, na, nb,
                                                                                                   "EQUAL" if eq else "DIFFERS"))
            if not same_ops:
                d = {o: ob[o] - oa[o] for o in set(oa) | set(ob) if oa[o] != ob[o]}
                print("    " + " ".join("%s:%+d" % kv for kv in sorted(d.items())))
print(("\n%d kernel(s) differ" % unequal) if unequal else "\nall kernels equal")
