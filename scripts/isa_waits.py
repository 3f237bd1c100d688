#!/usr/bin/env python3
"""The waits on the vector memory counter in one gfx950 kernel, read from the built object (the sibling of isa_mix.py: the device code object is pulled out of
the host object's offload bundle and disassembled the same way).  gfx950 counts a wave's loads AND stores in one counter, vmcnt, and `s_waitcnt vmcnt(N)`
holds the wave until at most N of them are in flight: a wait the compiler places for an operand that was loaded long ago still drains the wave's own stores
down to N.  For the named kernel this lists every `s_waitcnt vmcnt(N)` on one path through the code with
   the vector memory operations issued before it on that path (loads, stores), how many of them are stores issued since the path's first error-image store
   (a buffer store), and the next instruction with its registers (what the wait guards).
A path is a walk from the kernel's entry in layout order: conditional branches fall through unless named with --take (or unless the two instructions in
front make the condition constant), s_branch is followed, the walk ends at s_endpgm (or when it would enter an instruction twice).  Without --take the script walks every path that leaves the fall-through walk at ONE conditional
branch in front of the first store, and reports the one on which most error-image stores lie with no exec-masked skip (s_cbranch_execz) around any of them --
the full-tile path of the exact K2 builds where there is one; otherwise the fall-through walk.  --paths lists the candidates.
usage: isa_waits.py <host object> <mangled-name regex> [--take i,j,..] [--paths] [--json out.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
VMEM = ("global_", "buffer_", "flat_", "scratch_")


def disassemble(obj, pattern):
    """the disassembly of the functions of the object's gfx950 code whose mangled name matches `pattern` (only those: the whole object takes 10 s)"""
    obj = os.path.abspath(obj)
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, os.path.basename(obj))
        os.symlink(obj, base)
        subprocess.run([OBJDUMP, "--offloading", base], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in os.listdir(tmp) if "amdgcn" in f]
        if not co:
            raise SystemExit("no gfx950 code object in %s" % obj)
        co = os.path.join(tmp, co[0])
        rx = re.compile(pattern)
        syms = subprocess.run([OBJDUMP, "-t", co], check=True, capture_output=True, text=True).stdout
        names = sorted({l.split()[-1] for l in syms.splitlines() if " F " in l and ".text" in l and rx.search(l.split()[-1])})
        if not names:
            return ""
        return subprocess.run([OBJDUMP, "-d", "--disassemble-symbols=" + ",".join(names), co], check=True, capture_output=True, text=True).stdout


def kernels(dis, pattern):
    """{mangled name: [(offset, opcode, operands, branch target offset or None)]} of every kernel whose name matches"""
    rx, out, cur, first = re.compile(pattern), {}, None, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur, first = (out.setdefault(m.group(1), []) if rx.search(m.group(1)) else None), None
            continue
        if cur is None:
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*[0-9A-Fa-f ]+?(?:<[^>+]*(?:\+0x([0-9a-f]+))?>)?\s*$", line)
        if not m:
            continue
        addr = int(m.group(3), 16)
        first = addr if first is None else first
        tgt = None
        if m.group(1).startswith(("s_cbranch", "s_branch")):
            tgt = int(m.group(4), 16) if m.group(4) else 0
        cur.append((addr - first, m.group(1), m.group(2), tgt))
    return out


def walk(code, take=()):
    """one path: the indices of the instructions in execution order and the conditional branches met [(position in the walk, index, taken)]"""
    at = {ins[0]: i for i, ins in enumerate(code)}
    i, seen, order, branches = 0, set(), [], []
    while i < len(code) and i not in seen:
        seen.add(i)
        order.append(i)
        _, op, _, tgt = code[i]
        if op == "s_endpgm":
            break
        if op == "s_branch":
            i = at[tgt]
            continue
        if op.startswith("s_cbranch"):
            taken = len(branches) in take
            # a condition the two instructions in front make constant -- the structuriser's `s_mov_b64 s[a:b], 0; s_and_b64 vcc, exec, s[a:b]; s_cbranch_vccz`
            # at the end of a path that returns -- goes the way it must
            if op in ("s_cbranch_vccz", "s_cbranch_vccnz") and len(order) >= 3:
                (_, o1, a1, _), (_, o2, a2, _) = code[order[-3]], code[order[-2]]
                m1, m2 = re.match(r"(s\[\d+:\d+\]), 0$", a1), re.match(r"vcc, exec, (s\[\d+:\d+\])$", a2)
                if o1 == "s_mov_b64" and o2 == "s_and_b64" and m1 and m2 and m1.group(1) == m2.group(1):
                    taken = op == "s_cbranch_vccz"
                # ... or the same with the mask inverted, `s_andn2_b64 vcc, exec, s[a:b]; s_cbranch_vccnz` (the exit of the full-tile path's tile loop)
                if o1 == "s_mov_b64" and o2 == "s_andn2_b64" and m1 and m2 and m1.group(1) == m2.group(1):
                    taken = op == "s_cbranch_vccnz"
            # ... or `s_branch L; L: s_cbranch_execnz <end>` with nothing in between that could have cleared exec: the way out of the rolled tile loop of the
            # full-tile path (a wave that gets there runs with the lanes it had)
            if op == "s_cbranch_execnz" and len(order) >= 2 and code[order[-2]][1] == "s_branch":
                taken = True
            branches.append((len(order) - 1, i, taken))
            if taken:
                i = at[tgt]
                continue
        i += 1
    return order, branches


def report(code, take=()):
    """the waits of one path and what the criterion of a full-tile path needs: error-image stores, and those of them inside an exec-masked skip"""
    order, branches = walk(code, take)
    loads = stores = err_stores = 0
    first_store = None
    waits, skipped_until, guarded, execz = [], -1, 0, 0
    for pos, i in enumerate(order):
        off, op, args, tgt = code[i]
        if op == "s_cbranch_execz" and tgt is not None and tgt > off:
            skipped_until = max(skipped_until, tgt)
            execz += 1
        if op.startswith(VMEM):
            if "_store" in op or "_atomic" in op:
                stores += 1
                if op.startswith("buffer_store"):
                    err_stores += 1
                    first_store = pos if first_store is None else first_store
                    guarded += off < skipped_until
            else:
                loads += 1
        m = re.search(r"vmcnt\((\d+)\)", args) if op == "s_waitcnt" else None
        if m:
            nxt = next((code[j] for j in order[pos + 1:] if code[j][1] not in ("s_waitcnt", "s_nop")), None)
            waits.append(dict(position=pos, offset=off, n=int(m.group(1)), loads_before=loads, stores_before=stores, err_stores_before=err_stores,
                              after_first_store=first_store is not None, next="%s %s" % (nxt[1], nxt[2]) if nxt else ""))
    return dict(take=list(take), order=order, instructions=len(order), loads=loads, stores=stores, err_stores=err_stores, err_stores_under_execz=guarded, execz_skips=execz, waits=waits,
                branches_before_first_store=[b for b, (pos, _, _) in enumerate(branches) if first_store is None or pos < first_store])


def _vregs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def early_overwrites(code, order, states):
    """[(offset, store, idle cycles, instruction)]: vector instructions on the path that WRITE a data register of a buffer store fewer than `states` cycles
    behind it (an instruction is one cycle, s_nop N is N + 1).  Measured on MI355X: at zero cycles behind `buffer_store_dwordx4 .., sNN offen` the store
    wrote the NEW value in some lanes, now and then -- and the compiler's hazard rule leaves the buffer form with a scalar offset register out"""
    bad = []
    for pos, i in enumerate(order):
        off, op, args, _ = code[i]
        if not op.startswith("buffer_store_"):
            continue
        data, idle = _vregs(args.split(",")[0].strip()), 0
        for j in order[pos + 1:]:
            o2, a2 = code[j][1], code[j][2]
            if idle >= states:
                break
            if o2.startswith("v_") and not o2.startswith("v_cmp") and _vregs(a2.split(",")[0].strip()) & data:
                bad.append((off, "%s %s" % (op, args), idle, "%s %s" % (o2, a2)))
                break
            idle += int(a2) + 1 if o2 == "s_nop" else 1
    return bad


def full_tile_path(code):
    """(the chosen path's report, all candidates): among the walks with no error-image store inside an exec-masked skip, the one with the most error-image
    stores, then the fewest exec-masked skips of any kind (a kernel without error images: its partial-sum stores alone sit under one); else the fall-through
    walk"""
    base = report(code)
    cands = [base] + [report(code, (b,)) for b in base["branches_before_first_store"]]
    clean = [c for c in cands if c["stores"] and not c["err_stores_under_execz"]]
    return (max(clean, key=lambda c: (c["err_stores"], -c["execz_skips"])) if clean else base), cands


def table(name, rep):
    lines = ["kernel %s" % name,
             "path: take %s; %d instructions, %d loads, %d stores (%d error-image stores, %d of them inside an s_cbranch_execz skip); %d waits on vmcnt, %d after the first error-image store" %
             (rep["take"] or "none (fall-through)", rep["instructions"], rep["loads"], rep["stores"], rep["err_stores"], rep["err_stores_under_execz"], len(rep["waits"]),
              sum(w["after_first_store"] for w in rep["waits"])),
             "#  offset  vmcnt  loads  stores  err-stores  next instruction"]
    for w in rep["waits"]:
        lines.append("%8x  %5d  %5d  %6d  %10d  %s" % (w["offset"], w["n"], w["loads_before"], w["stores_before"], w["err_stores_before"], w["next"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("obj")
    ap.add_argument("pattern")
    ap.add_argument("--take", default=None)
    ap.add_argument("--paths", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ks = kernels(disassemble(a.obj, a.pattern), a.pattern)
    if not ks:
        raise SystemExit("no kernel matches %r" % a.pattern)
    res = {}
    for name, code in ks.items():
        if a.take is not None:
            rep, cands = report(code, tuple(int(t) for t in a.take.split(",") if t)), []
        else:
            rep, cands = full_tile_path(code)
        print("\n".join(table(name, rep)))
        if a.paths:
            for c in cands:
                print("  candidate take %-6s %5d instructions  %3d error-image stores (%d under execz)  %3d waits" %
                      (c["take"], c["instructions"], c["err_stores"], c["err_stores_under_execz"], len(c["waits"])))
        res[name] = {k: v for k, v in rep.items() if k != "order"}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
