#!/usr/bin/env python3
"""Analysis (no GPU): walk ONE kernel of a device assembly listing (the -save-temps .s of build()) along a path and list the branches with their
distances in instructions.  Control flow only: labels, s_branch, s_cbranch_*, s_endpgm -- no arithmetic is read or judged.

The walk starts at the kernel's first instruction and FALLS THROUGH every conditional branch, which is what DESIGN section 5 claims of the path a
trotting wavefront runs; an unconditional s_branch is followed (a taken jump by construction).  Where the code is laid out the other way round --
the hot side is the branch target -- name the branch by its ordinal among the conditional branches the walk meets: --take 12,40.  Which
data-dependent exits a trot really takes (the last trip of the fast chain, for one) is the source's knowledge, not this tool's: they are listed as
branches passed, with the distance a taken one would jump.

Also listed, for the whole kernel whatever the path: DETOURS -- conditional branches whose target is a short block that ends in an unconditional
jump back to within --near instructions of where it came from (a hot body reached through a stub placed far away costs two taken jumps).

    python3 tools/lab/trot_branches.py build/wbc_kernels-hip-amdgcn-amd-amdhsa-gfx950.s --kernel ILi1ELb0EJEE [--take 3,7] [--far 256]"""
import re, sys


def kernel_body(path, pick):
    """(name, [(mnemonic, operand text)], {label: index of the instruction it stands in front of}) of the first function whose mangled name holds `pick` (rollout kernels skipped)"""
    ins, labels, name = [], {}, None
    for line in open(path):
        s = line.split(";")[0].rstrip()
        if name is None:
            m = re.match(r"^(_Z\w+):", s)
            if m and pick in m.group(1) and "rollout" not in m.group(1):
                name = m.group(1)
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(ins); continue
        s = s.strip()
        if not s or s.startswith("."):
            continue
        parts = s.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else ""))
    if name is None:
        raise SystemExit("no kernel with %r in %s" % (pick, path))
    return name, ins, labels


def main():
    a = sys.argv[1:]
    opt = lambda k, d: a[a.index(k) + 1] if k in a else d
    path, pick = a[0], opt("--kernel", "wbc_hex_kernelILi1ELb0EJEE")
    take = {int(x) for x in opt("--take", "").split(",") if x}
    far, near, stub = int(opt("--far", "256")), int(opt("--near", "64")), int(opt("--stub", "48"))
    name, ins, labels = kernel_body(path, pick)
    print("kernel %s: %d instructions, %d labels" % (name, len(ins), len(labels)))
    cond = [i for i, (op, _) in enumerate(ins) if op.startswith("s_cbranch")]
    unc = [i for i, (op, _) in enumerate(ins) if op == "s_branch"]
    print("static: %d conditional branches, %d unconditional" % (len(cond), len(unc)))

    # ---- detours, whole kernel
    print("detours (conditional branch -> stub of <= %d instructions -> jump back to within %d of the origin):" % (stub, near))
    nd = 0
    for i in cond:
        t = labels.get(ins[i][1].strip())
        if t is None: continue
        for j in range(t, min(t + stub, len(ins))):
            op, arg = ins[j]
            if op == "s_branch":
                back = labels.get(arg.strip())
                if back is not None and abs(back - i) <= near:
                    nd += 1
                    print("  at %6d  %-18s -> %6d (%+d)  stub %d instructions, back to %6d (%+d)" % (i, ins[i][0], t, t - i, j - t + 1, back, back - j))
                break
            if op.startswith("s_cbranch") or op == "s_endpgm":
                break
    print("  %d found" % nd)

    # ---- the walk
    print("walk from the entry, falling through%s:" % (" except at conditional branch(es) %s" % sorted(take) if take else ""))
    pc, k, taken, passed_far, seen = 0, 0, 0, 0, set()
    taken_far = 0
    # a kernel built with kernel-argument preloading opens with the loads of those arguments and a jump to the instruction behind them, for
    # firmware that does not preload; hardware that does enters behind that block (256 bytes into the kernel) and never runs it
    for i in range(min(8, len(ins))):
        if ins[i][0] == "s_branch" and labels.get(ins[i][1].strip()) == i + 1 and all(op.startswith(("s_load", "s_waitcnt")) for op, _ in ins[:i]):
            print("  (instructions 0..%d: the preload compatibility block, not run where the arguments arrive preloaded -- the walk starts at %d)" % (i, i + 1))
            pc = i + 1
            break
    while pc < len(ins):
        if pc in seen:
            print("  (back at %d: a loop the walk does not leave by falling through -- stop)" % pc); break
        seen.add(pc)
        op, arg = ins[pc]
        if op == "s_endpgm":
            print("  s_endpgm at %d" % pc); break
        if op == "s_branch":
            t = labels[arg.strip()]
            taken += 1; taken_far += abs(t - pc) >= far
            print("  TAKEN  at %6d  s_branch            -> %6d (%+d)" % (pc, t, t - pc))
            pc = t; continue
        if op.startswith("s_cbranch"):
            t = labels[arg.strip()]
            if k in take:
                taken += 1; taken_far += abs(t - pc) >= far
                print("  TAKEN  at %6d  %-18s -> %6d (%+d)   [conditional %d, by --take]" % (pc, op, t, t - pc, k))
                pc = t; k += 1; continue
            passed_far += abs(t - pc) >= far
            print("  passed at %6d  %-18s -> %6d (%+d)   [conditional %d]" % (pc, op, t, t - pc, k))
            k += 1
        pc += 1
    print("walk: %d instructions visited, %d conditional branches met, %d taken jumps (%d of them over >= %d instructions), %d passed branches with a target >= %d away"
          % (len(seen), k, taken, taken_far, far, passed_far, far))


if __name__ == "__main__":
    main()
