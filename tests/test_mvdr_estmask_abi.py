"""CPU: the interface of the mask estimator of the MVDR context (mca_hip_mvdr_set_mask_estimator, mca_hip_mvdr_get_mask_estimator,
mca_hip_mvdr_sources_frames_auto_*) is declared, bound, present in the built library and exposed through the Python and C++ classes,
and its kernel k_mvdr_estmask uses no scratch and at most 256 VGPRs, beside an unchanged set of k_mvdr_solve_t / k_mvdr_solve_rtf_t
instantiations."""
import ctypes as C
import inspect
import os
import re

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_set_mask_estimator", "mca_hip_mvdr_get_mask_estimator", "mca_hip_mvdr_sources_frames_auto_dev",
       "mca_hip_mvdr_sources_frames_auto_host")


def test_header_declares_and_binding_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # the argument lists are those of the masked calls with the mask argument exchanged for the two outputs
    for form in ("dev", "host"):
        m, a = bound["mca_hip_mvdr_sources_frames_masked_" + form], bound["mca_hip_mvdr_sources_frames_auto_" + form]
        assert len(a) == len(m) + 1
        decl = {kind: re.sub(r"\s+", " ", re.search(r"int mca_hip_mvdr_sources_frames_%s_%s\(([^)]*)\)" % (kind, form), text).group(1))
                for kind in ("masked", "auto")}
        sfx = "_dev" if form == "dev" else ""
        outs = "float *update_mask_out%s, float *target_mask_out%s, " % (sfx, sfx)
        assert decl["auto"].count(outs) == 1
        assert decl["auto"].replace(outs, "const float *update_mask%s, " % sfx) == decl["masked"], (decl["auto"], decl["masked"])
    assert "target_mask_out_dev [streams][n_sources][F][K]" in raw and "update_mask_out_dev [streams][F][K]" in raw
    assert "6 = k_mvdr_estmask" in raw and "0.2 / 0.4" in raw
    # the configuration struct of the header and of the binding agree
    fields = re.search(r"typedef struct \{([^}]*)\} mca_hip_mvdr_estmask_config;", text).group(1)
    names = [n for decl in re.findall(r"\w+\s+([^;]+);", fields) for n in re.findall(r"\w+", decl)]
    assert names == [f[0] for f in _lib.MvdrEstmaskConfig._fields_]
    assert names == ["struct_size", "enable", "bin_lo", "bin_hi", "coherence_lo", "coherence_hi", "n_protected"]
    assert C.sizeof(_lib.MvdrEstmaskConfig) == 40


def test_python_and_cxx_classes_estimate_the_masks():
    for name in ("process", "process_dev", "process_sources", "process_sources_dev"):
        p = inspect.signature(getattr(api.MvdrBeamformer, name)).parameters
        assert "estimate_masks" in p and p["estimate_masks"].default is False, name
        assert p["target_mask"].default is None and p["update_mask"].default is None and p["update"].default is None, name
        tail = ["estimate_masks", "masks_out"] if name.endswith("_dev") else ["estimate_masks"]       # behind the existing parameters
        assert list(p)[-len(tail):] == tail, name
    for name in ("set_mask_estimator", "get_mask_estimator"):
        assert callable(getattr(api.MvdrBeamformer, name)), name
    assert api.MvdrBeamformer.K_ESTMASK == 6 and api.MvdrBeamformer.K_RTF == 5
    d = inspect.signature(api.MvdrBeamformer.set_mask_estimator).parameters
    assert (d["enable"].default, d["bin_lo"].default, d["bin_hi"].default, d["coherence_lo"].default, d["coherence_hi"].default,
            d["n_protected"].default) == (True, 0, None, 0.0, 0.05, 0)
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("void setMaskEstimator(bool enable, int binLo = 0, int binHi = -1, double coherenceLo = 0.0, double coherenceHi = 0.05, int nProtected = 0)",
                 "void getMaskEstimator(bool &enable, int &binLo, int &binHi, double &coherenceLo, double &coherenceHi, int &nProtected) const",
                 "int processAuto(const std::vector<Tin *> &in, int nSamples, Tout *out, int outSize, float *updateMaskOut = nullptr, float *targetMaskOut = nullptr)",
                 "int processAuto(const std::vector<Tin *> &in, int nSamples, const std::vector<Tout *> &out, int outSize, float *updateMaskOut = nullptr, float *targetMaskOut = nullptr)"):
        assert decl in text, decl


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    buf = (C.c_float * 8)()
    cfg = _lib.MvdrEstmaskConfig()
    cfg.struct_size = C.sizeof(_lib.MvdrEstmaskConfig)
    assert lib.mca_hip_mvdr_set_mask_estimator(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_get_mask_estimator(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_sources_frames_auto_dev(None, buf, 8, 4, 1, 1, 1, buf, buf, buf, buf, buf, None) == -1
    assert lib.mca_hip_mvdr_sources_frames_auto_dev(None, buf, 8, 4, 1, 1, 1, buf, None, None, buf, buf, None) == -1
    assert lib.mca_hip_mvdr_sources_frames_auto_host(None, buf, 1, 1, 1, buf, buf, buf, buf, buf) == -1
    assert lib.mca_hip_mvdr_sources_frames_auto_host(None, buf, 1, 1, 1, buf, None, None, buf, buf) == -1


def _spills():
    import importlib.util
    import shutil
    # the library is built by the ROCm toolchain that ships the tool; without it the register guarantee would go unchecked
    assert shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf"), "llvm-readelf of the ROCm toolchain is needed to read the kernels' register use"
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_estmask_kernel_uses_no_scratch():
    mod = _spills()
    assert any(re.search(p, "k_mvdr_estmask") for p in mod.DEFAULT_PATTERNS)             # the lint at the link covers it
    every = mod.kernels(_lib.LIB_PATH)
    est = [k for k in every if "k_mvdr_estmaskI" in k.get("name", "")]
    assert len(est) == 4, [k["name"] for k in est]                                       # one per number of row slots
    for k in est:
        assert not any(int(k[f]) for f in mod.FIELDS), (k["name"], [k[f] for f in mod.FIELDS])
        assert int(k["vgpr_count"]) <= 256, k["name"]
        assert int(k.get("group_segment_fixed_size", 0)) == 0, k["name"]                 # no LDS
    counts = sorted(int(k["vgpr_count"]) for k in est)
    print("k_mvdr_estmask: VGPRs %s" % counts)
    assert counts == [30, 40, 52, 60], counts          # the row of DESIGN.md 4.9 (at most 64: eight waves per SIMD); a compiler that moves it moves the row


def test_solve_instantiations_are_untouched():
    """the counts the other ABI tests hold k_mvdr_solve_t and k_mvdr_solve_rtf_t to"""
    mod = _spills()
    every = mod.kernels(_lib.LIB_PATH)
    assert len(mod.solve_t(every, WEIGHT=2)) == 88 and len(mod.solve_t(every, WEIGHT=2, NOISE=1)) == 44
    assert len(mod.solve_t(every, WEIGHT=1)) == 88 and len(mod.solve_t(every, WEIGHT=0)) == 36
    assert len([k for k in every if "k_mvdr_solve_rtf_tI" in k.get("name", "")]) == 2 * 4 * 2 * 4
    assert len([k for k in every if re.search(r"k_mvdr_rtfI", k.get("name", ""))]) == 4
