#!/usr/bin/env python3
"""Compare the kernel dispatches of two runs of one program, e.g. against two builds of the library (MCA_HIP_LIB):

    rocprofv3 --kernel-trace -f csv -d OLD_DIR -- python tools/compare_builds.py --child old.json     (the same for NEW_DIR)
    python tools/dispatch_diff.py [--shapes | --kernels SUBSTRING] OLD_DIR NEW_DIR

The ordered lists of (kernel name, grid, workgroup size, LDS bytes) must be equal line by line: the check for what changes no output
byte -- frames per wave, the skew of the resident round, the K split (csrc/stream_plan.h).  Prints the number of dispatches, the distinct
kernels and the first differences; exit status 1 if the lists differ.  --shapes: for a program whose number of calls depends on the clock
(bench.py times some of its parts by duration) -- the SETS of distinct (kernel name, grid, workgroup size, LDS bytes) must be equal, and the
length of the common prefix of the two lists is printed.  --kernels SUBSTRING: only the dispatches whose kernel name holds it (mca:: -- the
library's own) are compared line by line, and the others -- the runtime's copy and fill kernels behind hipMemcpy and hipMemset of a program
that uses the host-pointer calls, whose number is the runtime's business and moves between two runs of one build -- are counted by shape."""
import collections
import csv
import glob
import os
import sys


def dispatches(path):
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)) if os.path.isdir(path) else [path]
    assert files, "no *kernel_trace.csv under " + path
    rows = []
    for n, f in enumerate(files):                       # (a file per process: in the order of their names)
        for r in csv.DictReader(open(f)):
            rows.append((n, int(r["Dispatch_Id"]), (r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"),
                                                      int(r["LDS_Block_Size"]))))
    return [r[2] for r in sorted(rows, key=lambda r: r[:2])]


def main():
    shapes = sys.argv[1] == "--shapes"
    old, new = dispatches(sys.argv[-2]), dispatches(sys.argv[-1])
    if sys.argv[1] == "--kernels":
        rest = [collections.Counter(d for d in run if sys.argv[2] not in d[0]) for run in (old, new)]
        print("other kernels: %d / %d dispatches; by shape, only in one run: %s" % (sum(rest[0].values()), sum(rest[1].values()), dict((rest[0] - rest[1]) + (rest[1] - rest[0]))))
        old, new = ([d for d in run if sys.argv[2] in d[0]] for run in (old, new))
    if shapes:
        a, b = set(old), set(new)
        prefix = next((i for i, (x, y) in enumerate(zip(old, new)) if x != y), min(len(old), len(new)))
        print("%d / %d dispatches, equal up to line %d; %d / %d distinct launch shapes, %d only in one run" % (len(old), len(new), prefix, len(a), len(b), len(a ^ b)))
        for d in sorted(a ^ b)[:10]:
            print("  only in the %s run: %s" % ("first" if d in a else "second", d))
        return 1 if a != b else 0
    differ = [i for i, (a, b) in enumerate(zip(old, new)) if a != b]
    print("%d / %d dispatches of %d / %d distinct kernels, %d lines differ" % (len(old), len(new), len({d[0] for d in old}), len({d[0] for d in new}), len(differ)))
    for i in differ[:10]:
        print("  line %d:\n    %s\n    %s" % (i, old[i], new[i]))
    return 1 if differ or len(old) != len(new) else 0


if __name__ == "__main__":
    sys.exit(main())
