#!/usr/bin/env python3
"""The launch geometry of a rocprofv3 kernel trace, and the comparison of two of them.

    launch_trace.py list  kernel_trace.csv launches.txt > a.txt
                                                          the distinct launches, numbered in order of first appearance --
                                                          `k7 = kernel | grid | block | LDS bytes` -- then the sequence in start
                                                          order by number, a run of N equal launches as `k7*N`
    launch_trace.py diff  a.txt b.txt                     three lines: the two counts, equal or the first difference

The listing leaves out the HIP runtime's own copy and fill kernels (memcpy / memset, `__amd_rocclr_*`).  The trace's own LDS column
holds a kernel's STATIC allocation only, so the dynamic LDS bytes of every launch come from `launches.txt`, the log that a library
built with tools/launch_log.h writes in the same run: launch i of the log is launch i of the trace, and the join fails unless every
pair agrees in grid and block.  `lds 512+32000` is static + dynamic.  (tools/launch_shapes.py is the program to trace;
profiles/launch_record/ holds a pair.)"""
import csv
import itertools
import sys


def listing(path, log):
    rows = [r for r in csv.DictReader(open(path)) if not r["Kernel_Name"].startswith("__amd_rocclr_")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dims = lambda r, what: "x".join(r["%s_%s" % (what, a)] for a in "XYZ") if what + "_X" in r else r[what]        # noqa: E731
    logged = [ln.split() for ln in open(log).read().splitlines()]               # grid X Y block X lds N
    assert len(logged) == len(rows), "%d launches in the trace, %d in the log" % (len(rows), len(logged))
    seq = []
    for i, (r, lg) in enumerate(zip(rows, logged)):
        bx = int(r["Workgroup_Size_X"])
        want = (int(r["Grid_Size_X"]) // bx, int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"]), bx)
        assert want == (int(lg[1]), int(lg[2]), int(lg[4])), "launch %d: the trace has %s %r, the log %r" % (i, r["Kernel_Name"], want, lg)
        seq.append("%s | grid %s | block %s | lds %s+%s" % (r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r["LDS_Block_Size"], lg[6]))
    ids = {}
    for ln in seq:
        ids.setdefault(ln, "k%d" % len(ids))
    runs = ["%s%s" % (ids[ln], "*%d" % n if n > 1 else "") for ln, n in ((ln, len(list(g))) for ln, g in itertools.groupby(seq))]
    return ["%s = %s" % (i, ln) for ln, i in ids.items()] + ["sequence:"] + [" ".join(runs[i:i + 24]) for i in range(0, len(runs), 24)]


def expand(path):
    """the listing back into one line per launch"""
    lines = open(path).read().splitlines()
    cut = lines.index("sequence:")
    table = dict(ln.split(" = ", 1) for ln in lines[:cut])
    out = []
    for run in " ".join(lines[cut + 1:]).split():
        i, _, n = run.partition("*")
        out += [table[i]] * int(n or 1)
    return out


if sys.argv[1] == "list":
    print("\n".join(listing(sys.argv[2], sys.argv[3])))
else:
    a, b = expand(sys.argv[2]), expand(sys.argv[3])
    print("%s: %d launches" % (sys.argv[2], len(a)))
    print("%s: %d launches" % (sys.argv[3], len(b)))
    bad = next((i for i in range(max(len(a), len(b))) if i >= len(a) or i >= len(b) or a[i] != b[i]), None)
    print("the same sequence of (kernel, grid, block, LDS bytes)" if bad is None else
          "FIRST DIFFERENCE at launch %d:\n  %s\n  %s" % (bad, a[bad] if bad < len(a) else "(none)", b[bad] if bad < len(b) else "(none)"))
    sys.exit(0 if bad is None else 1)
