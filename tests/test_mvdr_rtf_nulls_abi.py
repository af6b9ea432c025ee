"""CPU: the switch that lets the RTF-steered MVDR calls honour the null gain (mca_hip_mvdr_set_rtf_nulls, mca_hip_mvdr_get_rtf_nulls)
is declared, bound, present in the built library and exposed through the Python and C++ classes, and the kernels behind it,
k_mvdr_solve_rtf_nulls_t<Q, S, S1, PF, NOISE>, are the 24 of DESIGN.md 4.10: no scratch, at most 256 VGPRs, their workgroup memory
all dynamic and sized by mvdr_nulls_lds_bytes at the launch."""
import ctypes as C
import inspect
import os
import re

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_set_rtf_nulls", "mca_hip_mvdr_get_rtf_nulls")
NAME = re.compile(r"k_mvdr_solve_rtf_nulls_tILi(?P<Q>\d)ELi(?P<S>\d)ELi(?P<S1>\d)ELb(?P<PF>[01])ELb(?P<NOISE>[01])EEEv")


def test_header_declares_and_binding_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert "int mca_hip_mvdr_set_rtf_nulls(mca_hip_mvdr_ctx *ctx, int enable);" in text
    assert "int mca_hip_mvdr_get_rtf_nulls(const mca_hip_mvdr_ctx *ctx, int *enable);" in text
    assert bound[NEW[0]] == (C.c_int, [C.c_void_p, C.c_int]) and bound[NEW[1]][0] is C.c_int and len(bound[NEW[1]][1]) == 2
    # the switch is no part of the RTF configuration
    assert [f[0] for f in _lib.MvdrRtfConfig._fields_] == ["struct_size", "enable", "target_alpha", "iterations", "ref_mic", "min_share"]
    # the normative text names what the issue asks it to
    for phrase in ("does not depend on the scale of d_r", "w = g0 / M per direction", "state blobs neither carry nor check it"):
        assert phrase in raw, phrase


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    e = C.c_int(7)
    assert lib.mca_hip_mvdr_set_rtf_nulls(None, 1) == -1
    assert lib.mca_hip_mvdr_get_rtf_nulls(None, C.byref(e)) == -1 and e.value == 7


def test_python_and_cxx_classes_carry_the_switch():
    p = inspect.signature(api.MvdrBeamformer.__init__).parameters
    assert list(p)[-2:] == ["null_gain", "rtf_nulls"] and p["rtf_nulls"].default is False
    assert inspect.signature(api.MvdrBeamformer.set_rtf_nulls).parameters["enable"].default is True
    assert callable(api.MvdrBeamformer.get_rtf_nulls)
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("void setRtfNulls(bool enable)", "bool getRtfNulls() const"):
        assert decl in text, decl


def _spills():
    import importlib.util
    import shutil
    assert shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf"), "llvm-readelf of the ROCm toolchain is needed to read the kernels' register use"
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lds_bytes(Q, S, S1):
    """mvdr_nulls_lds_bytes of mca_internal.h, whose text the test below holds to this"""
    return 256 * (8 * Q * S + (12 * S if S1 < S else 0))


def test_rtf_nulls_kernels_of_the_build():
    mod = _spills()
    every = mod.kernels(_lib.LIB_PATH)
    ks = [k for k in every if "k_mvdr_solve_rtf_nulls_tI" in k.get("name", "")]
    assert len(ks) == 24, [k["name"] for k in ks]
    seen = set()
    for k in ks:
        m = NAME.search(k["name"])
        assert m, k["name"]
        Q, S, S1, PF, NOISE = (int(m.group(f)) for f in ("Q", "S", "S1", "PF", "NOISE"))
        seen.add((Q, S, NOISE))
        # the form of the CELL nulls row (mvdr_solve_form): two passes of two at Q = S = 4, no load a frame ahead at Q = 4, S >= 3
        assert S1 == (2 if (Q, S) == (4, 4) else S) and PF == (0 if Q == 4 and S >= 3 else 1), k["name"]
        assert not any(int(k[f]) for f in mod.FIELDS), (k["name"], [k[f] for f in mod.FIELDS])
        assert int(k["vgpr_count"]) <= 256, k["name"]
        # all of its workgroup memory is the dynamic LDS of the launch: mvdr_nulls_lds_bytes, under the 64 KiB a launch may ask
        # for without an attribute, and two workgroups of it fit the 160 KiB of a CU beside the 256 VGPRs of __launch_bounds__(256, 2)
        assert int(k.get("group_segment_fixed_size", 0)) == 0, k["name"]
        assert 0 < _lds_bytes(Q, S, S1) <= 64 * 1024, k["name"]
        assert any(re.search(p, k["name"]) for p in mod.DEFAULT_PATTERNS), k["name"]      # the lint at the link covers it
        print("Q %d S %d S1 %d PF %d NOISE %d: %3d VGPRs, %5d bytes of LDS" % (Q, S, S1, PF, NOISE, int(k["vgpr_count"]), _lds_bytes(Q, S, S1)))
    assert seen == {(Q, S, n) for Q in (1, 2, 3, 4) for S in (2, 3, 4) for n in (0, 1)}
    assert max(_lds_bytes(Q, S, 2 if (Q, S) == (4, 4) else S) for Q in (1, 2, 3, 4) for S in (2, 3, 4)) == 44 * 1024
    # the formula above is the header's, and the launch passes what the lookup returned
    text = open(os.path.join(ROOT, "mcarray_amd", "csrc", "mca_internal.h")).read()
    assert "inline int mvdr_nulls_lds_bytes(int Q, int S, int S1) { return 256 * (8 * Q * S + (S1 < S ? 12 * S : 0)); }" in text
    solve = open(os.path.join(ROOT, "mcarray_amd", "csrc", "mvdr_solve.h")).read()
    lookup = solve[solve.index("const void *mvdr_solve_rtf_nulls_kernel_of"):]
    assert "*lds_bytes = mvdr_nulls_lds_bytes(RQ, RS, f.S1);" in lookup and "mvdr_solve_form(RQ, false, RS, true, MvdrWeight::CELL, NOISE)" in lookup
    apisrc = open(os.path.join(ROOT, "mcarray_amd", "csrc", "api_mvdr.hip")).read()
    assert "mvdr_solve_rtf_nulls_kernel_of<true>(Q, n_sources, &lds)" in apisrc and "mvdr_solve_rtf_nulls_kernel_of<false>(Q, n_sources, &lds)" in apisrc
    assert "kargs, (size_t)lds, st)" in apisrc


def test_other_solve_instantiations_are_untouched():
    """the counts the other ABI tests hold k_mvdr_solve_t and k_mvdr_solve_rtf_t to: the new name stays out of all of them"""
    mod = _spills()
    every = mod.kernels(_lib.LIB_PATH)
    assert len(mod.solve_t(every, WEIGHT=2)) == 88 and len(mod.solve_t(every, WEIGHT=2, NOISE=1)) == 44
    assert len(mod.solve_t(every, WEIGHT=1)) == 88 and len(mod.solve_t(every, WEIGHT=0)) == 36
    assert len([k for k in every if "k_mvdr_solve_rtf_tI" in k.get("name", "")]) == 64
    assert not [k for k in every if "k_mvdr_solve_rtf_nulls" in k.get("name", "") and re.search(mod.DEFAULT_PATTERNS[0], k["name"])]


def test_makefile_builds_the_two_translation_units_without_slp():
    mk = open(os.path.join(ROOT, "mcarray_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS := (.*)$", mk, flags=re.M).group(1).split()
    slp = re.search(r"^SLP_FILES := (.*)$", mk, flags=re.M).group(1).split()
    for o in ("kernels_mvdr_solve_rtf_nulls.o", "kernels_mvdr_solve_rtf_nulls_noise.o"):
        assert o in objs and o not in slp, o
