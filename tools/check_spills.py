"""Register lint of the built library: no MVDR solve kernel, nor the post-filter behind it, may spill to scratch.

The k_mvdr_solve / k_mvdr_solve_t instantiations for 13 ... 16 microphones sit a register or two under
the 256 that __launch_bounds__(256, 2) allows, so another compiler version may start to spill them without a word;
a spilled column loop costs more than the sharing gains.  This script reads the kernel metadata of every gfx950 code object
inside mcarray_amd/libmcarray_hip.so and lists the kernels whose name matches the pattern and whose .vgpr_spill_count or
.private_segment_fixed_size is not 0.  (.sgpr_spill_count is not in the rule: scalar registers spill into lanes of a vector
register, which the vector count already includes, not into memory.)
usage: python tools/check_spills.py [path/to/lib.so] [name pattern]     (exit code 3 when a kernel spills -- any other non-zero
code is a failure of the tooling itself; the Makefile runs it at the link)"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_spill_count", "private_segment_fixed_size")
# the solve kernels (the hand-written k_mvdr_solve<Q, FULL> and every k_mvdr_solve_t<...>); the post-filter; the estimated steering
# vectors: k_mvdr_rtf<Q> (two covariances in registers), k_mvdr_rtf_steering<Q> and the solve arm k_mvdr_solve_rtf_t<...>.  The arm has
# a pattern of its own: tests/test_mvdr_nulls_abi.py counts what the first one matches beside the weighted k_mvdr_solve_t.
# k_mvdr_estmask<Q>: the mask estimator, which is to stay without scratch as well.  k_mvdr_track*: the tracks of the look directions;
# k_mvdr_track_spectrum<Q> holds the two covariances of k_mvdr_rtf_steering<Q> and the association keeps its state in LDS.
# k_mvdr_trk2*: the tracks in azimuth and elevation; k_mvdr_trk2_vectors<Q> is that kernel's estimator on its own.
DEFAULT_PATTERNS = (r"k_mvdr_solve(?!_rtf)", r"k_mvdr_postfilter", r"k_mvdr_rtf|k_mvdr_solve_rtf", r"k_mvdr_estmask", r"k_mvdr_track", r"k_mvdr_trk2")
# the template arguments a mangled k_mvdr_solve_t name ends with: NULLS, REUSE, WEIGHT (0 none, 1 per frame, 2 per frame and bin), NOISE
SOLVE_T = re.compile(r"k_mvdr_solve_tI.*ELb(?P<NULLS>[01])ELb(?P<REUSE>[01])ELNS_10MvdrWeightE(?P<WEIGHT>[012])ELb(?P<NOISE>[01])EEEv")
KEY = re.compile(r"^(?:  - |    )\.(\w+):\s*(.*)$")       # a key of a kernel's own map (those of its arguments sit deeper)


def solve_t(ks, **want):
    """the k_mvdr_solve_t instantiations among ks whose NULLS / REUSE / WEIGHT / NOISE are those of want (ints)"""
    out = []
    for k in ks:
        m = SOLVE_T.search(k.get("name", ""))
        if m and all(int(m.group(f)) == v for f, v in want.items()):
            out.append(k)
    return out


def kernels(lib):
    """[{metadata key: text}, ...] over all kernels of all device code objects of lib."""
    out = []
    tmp = tempfile.mkdtemp(prefix="mca_spill_")
    try:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        objs = sorted(f for f in os.listdir(tmp) if "amdgcn" in f)
        if not objs:
            raise RuntimeError("no device code objects found in %s" % lib)
        for f in objs:
            text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=tmp, check=True, capture_output=True, text=True).stdout
            inside, cur = False, None
            for line in text.splitlines():
                if line.startswith("amdhsa.kernels:"):
                    inside = True
                elif inside and line[:1] not in (" ", ""):
                    inside, cur = False, None
                elif inside:
                    m = KEY.match(line)
                    if m and line.startswith("  - "):
                        cur = {}
                        out.append(cur)
                    if m and cur is not None:
                        cur[m.group(1)] = m.group(2).strip().strip("'\"")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcarray_amd", "libmcarray_hip.so")
    pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else "|".join(DEFAULT_PATTERNS))
    ks = [k for k in kernels(lib) if pat.search(k.get("name", ""))]
    if not ks or any(f not in k for k in ks for f in FIELDS + ("vgpr_count",)):
        raise RuntimeError("kernel metadata of %s not understood (%d kernels match)" % (lib, len(ks)))
    bad = [k for k in ks if any(int(k[f]) != 0 for f in FIELDS)]
    for k in bad:
        print("%s: %s" % (k["name"], ", ".join("%s %s" % (f, k[f]) for f in FIELDS)))
    print("%s: %d of %d kernels matching '%s' spill; most VGPRs: %d" % (lib, len(bad), len(ks), pat.pattern, max(int(k["vgpr_count"]) for k in ks)))
    sys.exit(3 if bad else 0)
