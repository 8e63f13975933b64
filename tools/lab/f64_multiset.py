#!/usr/bin/env python3
"""Analysis (no GPU): has arithmetic moved between two builds?  For every kernel of two device assembly listings (the -save-temps .s of build())
the multiset of floating-point opcodes -- every instruction whose mnemonic holds _f64, counted by mnemonic -- and the kernel's registers and
private segment.  A layout change leaves every multiset equal; a difference means an expression was added, dropped, duplicated or re-associated.

    python3 tools/lab/f64_multiset.py parent/wbc_kernels-hip-amdgcn-amd-amdhsa-gfx950.s build/wbc_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"""
import collections, re, subprocess, sys


def read(path):
    k, cur = {}, None
    meta = collections.defaultdict(dict)
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1); k[cur] = [collections.Counter(), 0]; continue
        m = re.match(r"^\s*\.set (_Z\w+)\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size), (\d+)", line)
        if m:
            meta[m.group(1)][m.group(2)] = int(m.group(3)); continue
        if line.startswith(".Lfunc_end"):
            cur = None; continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op = s.split()[0]
        k[cur][1] += 1
        if "_f64" in op:
            k[cur][0][op] += 1
    return {n: (c, ni, meta.get(n, {})) for n, (c, ni) in k.items() if n in meta}


def dem(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    short = []
    for t in out:
        m = re.search(r"(\w+(<[^>]*>)?)\(", t.replace("(anonymous namespace)::", ""))
        short.append(m.group(1) if m else t[:60])
    return dict(zip(names, short))


if __name__ == "__main__":
    a, b = read(sys.argv[1]), read(sys.argv[2])
    names = sorted(set(a) | set(b)); d = dem(names)
    print("%-58s %-9s %7s %7s | %13s %13s | %9s %9s | %s" % ("kernel", "f64 ops", "f64 A", "f64 B", "instr A", "instr B", "V+A A", "V+A B", "sgpr A/B, scratch A/B"))
    bad = 0
    for n in names:
        if n not in a or n not in b:
            print("%-58s only in one build" % d[n]); bad += 1; continue
        (ca, ia, ma), (cb, ib, mb) = a[n], b[n]
        same = ca == cb
        ra, rb = ma.get("num_vgpr", 0) + ma.get("num_agpr", 0), mb.get("num_vgpr", 0) + mb.get("num_agpr", 0)
        flag = "" if same and rb <= ra and mb.get("private_seg_size", 0) == 0 else "   <-- LOOK"
        bad += bool(flag)
        print("%-58s %-9s %7d %7d | %13d %13d | %3d+%-3d   %3d+%-3d | %d/%d, %d/%d%s" % (
            d[n], "equal" if same else "DIFFERENT", sum(ca.values()), sum(cb.values()), ia, ib, ma.get("num_vgpr", 0), ma.get("num_agpr", 0),
            mb.get("num_vgpr", 0), mb.get("num_agpr", 0), ma.get("numbered_sgpr", 0), mb.get("numbered_sgpr", 0),
            ma.get("private_seg_size", 0), mb.get("private_seg_size", 0), flag))
        if not same:
            for op in sorted(set(ca) | set(cb)):
                if ca[op] != cb[op]: print("      %-28s %6d -> %6d" % (op, ca[op], cb[op]))
    print("%d kernels, %d to look at (a different multiset, more registers than A, or a private segment)" % (len(names), bad))
    sys.exit(1 if bad else 0)
