#!/usr/bin/env python3
"""The LDS waits of a step kernel's step boundary, from a kept device listing (hipcc -save-temps / -S).

For a kernel symbol (a substring of the mangled name is enough) this prints every `s_waitcnt lgkmcnt(n)` of the step
loop that lies OUTSIDE the piece region: before the loop's first and behind its last matrix instruction, or, in a kernel
without the moment fold, before its first and behind its last hand-placed `ds_read_b128` (inline assembly: the normals'
tables and the pieces of the decomposition; the row-pair kernels also read the accepted point 16 bytes at a time, through
the compiler, and those reads are the boundary's).  Next to each wait stand the LDS
operations it completes (all in flight but the n youngest: they return in issue order) and the number of vector
instructions between the oldest of them and the wait (and between the youngest and the wait) -- what a lone wavefront
had to issue while that operation was on its way.  A wait with few vector instructions behind an operation it covers
parks; one that covers nothing is free.

The walk is linear in layout order (as inflight_check.py's) and goes round the loop once before it reports, so the
waits at the top of a step see what the step before left in flight.  Blocks of the loop that a forward branch jumps
over and that store to global memory are left out of the walk (the save path of StepSave) and counted in the first line
of the output.  For listings of the plain build only: in a -DSMCMC_STEP_PROFILE listing the same rule would drop stamp
code.

usage: python tools/boundary_waits.py listing.s 'step_kernelILi50ELi0ELb1ELb0ELb1ELb0E'
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shadow_model import HAND, cls, kernel_lines, parse  # noqa: E402


def step_loop(items):
    """The loop (label .. backward branch to it) with the most matrix instructions, or without any in the kernel the
    most ds_read_b128; the innermost on a tie.  Labels stay in the result."""
    def weight(body):
        return (sum(1 for n, _ in body if cls(n) == "matrix"), sum(1 for n, _ in body if n == "ds_read_b128"))
    where = {v: i for i, (k, v) in enumerate(items) if k == "label"}
    best = None
    for i, (name, ops) in enumerate(items):
        if name == "label" or "branch" not in name:
            continue
        j = where.get(ops.split()[-1] if ops else "")
        if j is None or j > i:
            continue
        body = items[j:i + 1]
        key = weight(body) + (-len(body),)
        if best is None or key > best[0]:
            best = (key, body)
    if best is None or best[0][:2] == (0, 0):
        raise SystemExit("no step loop in this kernel")
    return best[1]


def plain_step(body):
    """The loop without the blocks a forward branch jumps over that store to global memory (the save path of StepSave:
    a plain step stores nothing, and walked in line its reads and full waits would hide what the commit leaves in
    flight), and without the labels; with it the number of blocks left out."""
    where = {v: i for i, (k, v) in enumerate(body) if k == "label"}
    drop, blocks = set(), 0
    for i, (name, ops) in enumerate(body):
        if name == "label" or "branch" not in name:
            continue
        j = where.get(ops.split()[-1] if ops else "")
        if j is not None and j > i and any(n.startswith(("global_store", "flat_store")) for n, _ in body[i + 1:j]):
            blocks += 0 if i + 1 in drop else 1   # (a block inside one already left out is not counted again)
            drop |= set(range(i + 1, j))
    return [it for i, it in enumerate(body) if i not in drop and it[0] != "label"], blocks


def piece_region(body):
    marks = [i for i, (n, _) in enumerate(body) if cls(n) == "matrix"]
    if not marks:
        marks = [i for i, (n, ops) in enumerate(body) if n == "ds_read_b128" and ops.endswith(HAND)]
    return marks[0], marks[-1]


def boundary_waits(body):
    """[(index in the loop, n, LDS operations covered, mnemonic of the oldest, vector instructions since it, mnemonic of
    the youngest, vector instructions since it)]"""
    first, last = piece_region(body)
    size = len(body)
    queue, out = [], []          # queue: (position over both rounds, mnemonic) of the LDS operations in flight
    vector_before = [0]          # vector instructions in front of each position
    for name, _ in body + body:
        vector_before.append(vector_before[-1] + (1 if cls(name) in ("vector", "matrix") else 0))
    for pos, (name, ops) in enumerate(body + body):
        if cls(name) == "lds":
            queue.append((pos, name))
            continue
        m = re.search(r"lgkmcnt\((\d+)\)", ops) if cls(name) == "wait" else None
        if not m:
            continue
        n = int(m.group(1))
        covered = queue[:len(queue) - n] if n < len(queue) else []
        queue = queue[len(covered):]
        i = pos - size
        if i < 0 or first <= i <= last:
            continue
        if covered:
            out.append((i, n, len(covered), covered[0][1], vector_before[pos] - vector_before[covered[0][0]],
                        covered[-1][1], vector_before[pos] - vector_before[covered[-1][0]]))
        else:
            out.append((i, n, 0, "-", 0, "-", 0))
    return out, first, last, size


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("symbol")
    a = ap.parse_args()
    loop = step_loop(parse(kernel_lines(a.listing, a.symbol), mark_hand=True))
    body, blocks = plain_step(loop)
    waits, first, last, size = boundary_waits(body)
    print("step loop: %d instructions, piece region %d .. %d; left out: %d block(s) that store to global memory, %d instructions" %
          (size, first, last, blocks, sum(1 for it in loop if it[0] != "label") - size))
    for i, n, k, oldest, vec, youngest, vec_young in waits:
        where = "top" if i < first else "end"
        if k:
            print("%s +%5d  s_waitcnt lgkmcnt(%d): covers %2d, oldest %s %d vector instructions back, youngest %s %d" %
                  (where, i, n, k, oldest, vec, youngest, vec_young))
        else:
            print("%s +%5d  s_waitcnt lgkmcnt(%d): covers nothing" % (where, i, n))
    parked = [w for w in waits if w[2]]
    print("waits outside the piece region: %d, of them with something to wait for: %d" % (len(waits), len(parked)))


if __name__ == "__main__":
    main()
