#!/usr/bin/env python3
"""Kernel by kernel comparison of two builds of one host object: registers, scratch, LDS (as kernel_regs.py reads them) and the disassembled instruction
sequence of the gfx950 code object with addresses, encodings and symbol names left out.  For refactors that must not change generated code.
usage: kernel_diff.py <old object> <new object> [old-name-substring=new-name-substring ...]   (the pairs name kernels that were renamed)
Prints one row per kernel of the old object; exit status 1 if a kernel is missing or differs in anything."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
KEYS = ("agpr_count", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def run(*a, **kw):
    return subprocess.run(a, check=True, capture_output=True, text=True, **kw).stdout


def kernels(obj):
    """{mangled name: (resources, [instruction text])} of the object's code object"""
    obj = os.path.abspath(obj)
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, os.path.basename(obj))
        os.symlink(obj, base)
        run(os.path.join(LLVM, "llvm-objdump"), "--offloading", base, cwd=tmp)
        co = os.path.join(tmp, [f for f in os.listdir(tmp) if "amdgcn" in f][0])
        notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
        dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
    res = {}
    for b in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        b = ".agpr_count:" + b
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        res[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, b).group(1)) for k in KEYS)
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip()) or re.match(r"^[0-9a-f]+ <(\S+)>:$", line.strip())
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            t = re.sub(r"//.*$", "", line)          # the address / encoding comment
            t = re.sub(r"<[^>]*>", "<sym>", t)      # symbol names
            t = " ".join(t.split())
            if t == "...":                          # padding behind the kernel
                continue
            if cur and cur[-1].startswith("s_getpc_b64") and t.startswith("s_add_u32"):
                t = re.sub(r"0x[0-9a-f]+$", "<pcrel>", t)  # the distance to a constant table: an address
            cur.append(t)
    for c in code.values():
        while c and c[-1] == "s_nop 0":  # alignment behind s_endpgm
            c.pop()
    return {n: (r, code.get(n, [])) for n, r in res.items()}


def main(old, new, pairs):
    A, B = kernels(old), kernels(new)
    ren = [p.split("=", 1) for p in pairs]
    bad = 0
    print("# %-6s agpr vgpr sgpr scratch lds : old -> new, instructions old / new, kernel" % "result")
    for name in sorted(A):
        other = name if name in B else None
        if other is None:
            for o, n in ren:
                c = [k for k in B if o in name and n in k and k not in A]
                if len(c) == 1:
                    other = c[0]
        ra, ia = A[name]
        if other is None:
            print("MISSING %s : - , %d / - , %s" % (ra, len(ia), name))
            bad += 1
            continue
        rb, ib = B[other]
        same = ra == rb and ia == ib
        bad += 0 if same else 1
        tag = "same" if same else ("regs" if ia == ib else "code")
        print("%-7s %s -> %s, %d / %d, %s%s" % (tag, " ".join(map(str, ra)), " ".join(map(str, rb)), len(ia), len(ib), name, "" if other == name else " -> " + other))
    for name in sorted(set(B) - set(A) - {k for k in B if any(n in k for _, n in ren)}):
        print("NEW     %s, %d, %s" % (" ".join(map(str, B[name][0])), len(B[name][1]), name))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
