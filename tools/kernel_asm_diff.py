#!/usr/bin/env python3
"""Compare two device assembly files of the same HIP source function by function: which kernels' code differs.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize -Imcarray_amd/csrc -Iinclude --offload-device-only -S \\
          -o new.s mcarray_amd/csrc/kernels_stream.hip        (the same for the parent's file: old.s)
    python tools/kernel_asm_diff.py old.s new.s

Comments and .loc lines are dropped and the function index in basic-block labels is normalised, so a source edit that moves lines or
reorders functions but changes no instruction compares equal.  Prints the number of functions,
the names of those whose bodies differ, and every kernel whose registers, scratch or workgroup bound differ.  Exit status 1 if a body differs.
(tools/compare_builds.py compares what two builds COMPUTE on the GPU; this compares what they ARE, and needs none.)"""
import re
import sys


def functions(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = [ln.split(";")[0].rstrip() for ln in m.group(2).split("\n") if not ln.strip().startswith((";", ".loc"))]
        # basic-block labels carry the function's index in the file (.LBB2_7), which moves when the order of instantiation does
        out[m.group(1)] = re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(lines))
    return out


def metadata(path):
    text = open(path).read()
    text = text[text.index("amdhsa.kernels"):]
    out = {}
    for blk in text.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in
                     ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")
                     if re.search(r"\." + k + r":\s+(\d+)", blk)}
    return out


def main():
    old, new = sys.argv[1:3]
    a, b = functions(old), functions(new)
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("%d / %d functions, %d differ" % (len(a), len(b), len(differ)))
    for k in differ:
        print("  body differs:", k)
    ma, mb = metadata(old), metadata(new)
    for k in sorted(set(ma) | set(mb)):
        if ma.get(k) != mb.get(k):
            print("  metadata:", k, ma.get(k), "->", mb.get(k))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
