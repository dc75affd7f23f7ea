#!/usr/bin/env python3
"""The `s_waitcnt` instructions with a `vmcnt` field inside one loop of a kernel, and what each of them waits for
(from `hipcc -S --cuda-device-only -gline-tables-only`, as tools/isa_lines.py reads it):
    python tools/isa_waits.py <file.s> <mangled kernel name substring> --body <source file> --lines a-b [--depth D] [--via N] [--cold a-b,c,...]
--body / --lines   the loop: the instructions whose inlined-at chain passes through lines a..b of that source file (the step loop
                   of orlg_group_body.h, or of the wave kernel in orlg_kernels.hip)
--depth D          only the basic blocks the compiler's own loop comments place at loop depth >= D (the group kernel's step loop is
                   at depth 2, inside the work queue's loop): the loop's preheader carries the loop's line and is not part of it
--via N            only the copy of the body that was inlined through line N of the file that includes it (a DEFER instantiation
                   of the group kernel holds the body twice: the lean one and the full one, orlg_group_kernels.hip)
--cold             body lines of the blocks the hot path jumps over (replays, refill, reloads): a wait there is marked `cold`
Per wait: its line in the .s file, the body line and the innermost source line of the .loc in force, the counters it names, and
the vector-memory instructions that stand between the previous listed wait and this one IN THE FILE'S ORDER -- loads, stores,
atomics without return, scratch reloads and scratch spills, each with its body line.  On gfx9 `vmcnt` counts all of them in
order, so a `vmcnt(0)` waits for every one of them that the wave has executed.  A static listing: the file's order is not the
control flow, and a wait at a join also answers for the paths that arrive there from elsewhere.  In particular the mark `cold`
comes from the body line of the `.loc` in force and from nothing else: the compiler may lay the tail of a cold block directly
in front of a loop's header, and the tool cannot tell such a wait from one merged INTO the header, which every pass would
execute.  Before a count of hot waits is quoted, look at each `cold` wait that stands next to a loop header in the assembly:
the hot path must branch past it to the header's own label.

The assembly: one instantiation in a translation unit of its own, with the build's flags (build.py FLAGS) --
    // one.hip
    #include "orlg_host.h"
    #include "orlg_group_kernels.hip"      // the wave kernel: "orlg_kernels.hip"
    template __global__ void orlg_rmsa_group_kernel<5, 2, false, true>(const OrlgParams);   // orlg_rmsa_kernel_ff<5, 2, true>
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -I optical-rl-gym-qot-aware_amd/csrc \
          -S --cuda-device-only -gline-tables-only one.hip -o group.s
(compiled from the repository's root, so that the .loc comments name the sources by their paths in it)."""
import re
import sys


def kind(op, operands):
    if op.startswith("scratch_load"):
        return "scratch reload"
    if op.startswith("scratch_store"):
        return "scratch spill"
    if "_atomic_" in op:
        return "atomic+return" if re.search(r"\b(glc|sc0)\b", operands) else "atomic"
    if "_store" in op:
        return "store"
    if "_load" in op:
        return "load"
    return "vmem"


def ranges(arg):
    out = []
    for r in arg.split(","):
        a, _, b = r.partition("-")
        out.append((int(a), int(b or a)))
    return out


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    path, pat = sys.argv[1], sys.argv[2]
    body = opt("--body")
    lo, hi = ranges(opt("--lines"))[0]
    via = opt("--via")
    cold = ranges(opt("--cold")) if opt("--cold") else []
    min_depth = int(opt("--depth", "0"))
    depth, at_label = 0, False   # loop depth of the basic block, from the comments at its label
    inside = False
    cur = None   # (body line or None, innermost "file:line", via line or None)
    since = []
    n_wait = n_hot = 0
    for no, ln in enumerate(open(path), 1):
        if re.match(r"^_Z\w*:", ln) or re.match(r"^\w+:\s*; @", ln):
            inside = pat in ln
            cur = None
            continue
        if not inside:
            continue
        if ln.startswith(".Lfunc_end"):
            inside = False
            continue
        if re.match(r"^\.LBB\d+_\d+:", ln):
            m = re.search(r"in Loop: Header=\S+ Depth=(\d+)|This Loop Header: Depth=(\d+)", ln)
            depth, at_label = (int(m.group(1) or m.group(2)) if m else 0), True
            continue
        if at_label and ln.lstrip().startswith(";"):
            m = re.search(r"This Loop Header: Depth=(\d+)", ln)
            if m:
                depth = int(m.group(1))
            continue
        at_label = False
        if re.match(r"\s*\.loc\s", ln):
            # the chain of the comment: innermost first, "file:line:col @[ file:line:col @[ ... ] ]"
            chain = re.findall(r"([^\s\[\]@;]+):(\d+):\d+", ln.split(";", 1)[1] if ";" in ln else "")
            if chain and chain[0][1] == "0" and cur is not None:
                continue   # "line 0": code the compiler moved or made up (a folded reload, a join) -- it stays with the line before
            bl = vl = None
            for i, (f, l) in enumerate(chain):
                if f.endswith("/" + body) or f == body:
                    bl = int(l)
                    vl = chain[i + 1][1] if i + 1 < len(chain) else None
                    break
            inner = f"{chain[0][0].split('/')[-1]}:{chain[0][1]}" if chain else "?"
            cur = (bl, inner, vl)
            continue
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*)", ln)
        if not m or ln.strip().startswith((".", ";")) or cur is None:
            continue
        bl, inner, vl = cur
        if depth < min_depth or bl is None or not lo <= bl <= hi or (via is not None and vl != via):
            continue
        op, operands = m.group(1), m.group(2).split(";")[0]
        if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            since.append((kind(op, operands), op, bl))
            continue
        if op == "s_waitcnt" and "vmcnt" in operands:
            is_cold = any(a <= bl <= b for a, b in cold)
            n_wait += 1
            n_hot += 0 if is_cold else 1
            print(f"{path.split('/')[-1]}:{no}\tbody {bl}\t{inner}\t{operands.strip()}\t{'cold' if is_cold else 'HOT'}")
            if not since:
                print("\t(no vector-memory instruction since the previous wait)")
            for k, o, b in since:
                print(f"\t{k:15s}{o:28s}body {b}")
            since = []
    print(f"total: {n_wait} waits with a vmcnt field in {body}:{lo}-{hi}" + (f" via line {via}" if via else "") +
          (f", {n_hot} outside the cold lines" if cold else ""))


if __name__ == "__main__":
    main()
