#!/usr/bin/env python3
"""Static model of what issues in the shadow of the matrix instructions in a kernel's step loop.

An FP64 matrix instruction holds the vector pipe for its duration (16x16x4: 64 cycles, 4x4x4: 16) but not the issue of
LDS reads, waits and the other non-vector instructions: those that follow it, up to the next vector instruction, issue
under it at four cycles each.  For a kept device listing (hipcc -save-temps / -S) and a kernel symbol (a substring of the
mangled name is enough) this prints the step loop's instruction mix by class and, for every run of back-to-back matrix
instructions, its kinds, the non-vector instructions behind it and the cycles of the run's LAST instruction they cover:
min(4 x count, duration - 4).  The last line is the total per pass of the loop.  An estimate from the listing, not a
measurement: latencies, waits that park and the LDS queue are not modelled.

usage: python tools/shadow_model.py listing.s 'step_kernelILi50ELi0ELb1ELb0ELb1ELb0E' [--runs]
"""
import argparse
import collections
import re

ISSUE = 4
DURATION = {"16x16x4": 64, "4x4x4": 16}


def kernel_lines(path, name):
    out, inside = [], False
    for line in open(path).read().splitlines():
        if re.match(r"^(_Z\S*%s\S*):" % re.escape(name), line):
            if inside:
                raise SystemExit("%s: more than one symbol matches %r" % (path, name))
            inside = True
            continue
        if inside:
            if line.startswith(".Lfunc_end"):
                break
            out.append(line)
    if not out:
        raise SystemExit("%s: no kernel symbol matches %r" % (path, name))
    return out


HAND = " ;hand"   # parse(mark_hand=True): the end of the operands of an instruction of an inline-assembly block


def parse(lines, mark_hand=False):
    """[(mnemonic, operands)] with labels as ('label', name).  mark_hand: the operands of the instructions the source
    placed by hand (between the compiler's ;;#ASMSTART and ;;#ASMEND) end in HAND."""
    items, hand = [], False
    for line in lines:
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            items.append(("label", m.group(1)))
            continue
        if line.lstrip().startswith(";;#ASM"):
            hand = line.lstrip().startswith(";;#ASMSTART")
            continue
        m = re.match(r"^\s+([a-z][a-z_0-9]*)\s*(.*)$", line)
        if m and not line.lstrip().startswith((";", "//", ".")):
            items.append((m.group(1), m.group(2) + (HAND if mark_hand and hand else "")))
    return items


def cls(name):
    if name.startswith("v_mfma"):
        return "matrix"
    if name.startswith("ds_"):
        return "lds"
    if name.startswith("s_waitcnt"):
        return "wait"
    if name.startswith("s_nop"):
        return "nop"
    if name.startswith("v_"):
        return "vector"
    return "other"


def kind(name):
    for k in DURATION:
        if k in name:
            return k
    raise SystemExit("matrix instruction of unknown duration: " + name)


def step_loop(items):
    """The loop (label .. backward branch to it) that holds the most matrix instructions; the innermost on a tie."""
    where = {v: i for i, (k, v) in enumerate(items) if k == "label"}
    best = None
    for i, (name, ops) in enumerate(items):
        if name == "label" or "branch" not in name:
            continue
        target = ops.split()[-1] if ops else ""
        j = where.get(target)
        if j is None or j > i:
            continue
        body = [it for it in items[j:i + 1] if it[0] != "label"]
        n = sum(1 for it in body if cls(it[0]) == "matrix")
        if best is None or (n, -len(body)) > (best[0], -len(best[1])):
            best = (n, body)
    if best is None or best[0] == 0:
        raise SystemExit("no loop with matrix instructions in this kernel")
    return best[1]


def runs(body):
    """[(kinds of the run, classes of the non-vector instructions behind it)]"""
    out, i = [], 0
    while i < len(body):
        if cls(body[i][0]) != "matrix":
            i += 1
            continue
        kinds = []
        while i < len(body) and cls(body[i][0]) == "matrix":
            kinds.append(kind(body[i][0]))
            i += 1
        behind = []
        while i < len(body) and not body[i][0].startswith("v_"):
            behind.append(cls(body[i][0]))
            i += 1
        out.append((kinds, behind))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("symbol")
    ap.add_argument("--runs", action="store_true", help="one line per run of matrix instructions")
    a = ap.parse_args()
    body = step_loop(parse(kernel_lines(a.listing, a.symbol)))
    mix = collections.Counter(cls(n) for n, _ in body)
    print("step loop: %d instructions" % len(body))
    print("mix: " + ", ".join("%s %d" % (k, mix[k]) for k in ("vector", "matrix", "lds", "wait", "nop", "other")))
    kinds = collections.Counter(kind(n) for n, _ in body if cls(n) == "matrix")
    pipe = sum(DURATION[k] * v for k, v in kinds.items())
    print("matrix: " + ", ".join("%s %d" % kv for kv in sorted(kinds.items())) + ", %d cycles of the pipe" % pipe)
    rs = runs(body)
    total, by_shape = 0, collections.Counter()
    shadow_by_shape = collections.Counter()
    for n, (ks, behind) in enumerate(rs):
        s = min(ISSUE * len(behind), DURATION[ks[-1]] - ISSUE)
        total += s
        shape = "+".join(ks)
        by_shape[shape] += 1
        shadow_by_shape[shape] += s
        if a.runs:
            c = collections.Counter(behind)
            print("run %3d: %-24s behind %2d (%s) shadowed %2d" %
                  (n, shape, len(behind), ", ".join("%s %d" % (k, c[k]) for k in ("lds", "wait", "nop", "other") if c[k]), s))
    print("runs: %d" % len(rs))
    for shape in sorted(by_shape):
        print("  %-24s x %3d  shadowed %5d cycles" % (shape, by_shape[shape], shadow_by_shape[shape]))
    print("shadowed: %d of %d matrix-pipe cycles per pass of the loop" % (total, pipe))


if __name__ == "__main__":
    main()
