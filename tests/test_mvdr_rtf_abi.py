"""CPU: the interface of the estimated steering vectors of the MVDR context (mca_hip_mvdr_set_rtf, mca_hip_mvdr_sources_frames_rtf_*,
mca_hip_mvdr_get_steering, mca_hip_mvdr_get_target_covariance) is declared, bound, present in the built library and exposed through
the Python and C++ classes, and its kernels -- k_mvdr_rtf, k_mvdr_rtf_steering and every k_mvdr_solve_rtf_t -- use no scratch and at most 256
VGPRs, beside an unchanged set of k_mvdr_solve_t instantiations."""
import ctypes as C
import inspect
import os
import re

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_set_rtf", "mca_hip_mvdr_get_rtf", "mca_hip_mvdr_set_rtf_workspace", "mca_hip_mvdr_sources_frames_rtf_dev", "mca_hip_mvdr_sources_frames_rtf_host",
       "mca_hip_mvdr_get_steering", "mca_hip_mvdr_get_target_covariance")


def test_header_declares_and_binding_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # the argument lists are those of the masked calls with the target mask behind the update mask
    for form in ("dev", "host"):
        m, r = bound["mca_hip_mvdr_sources_frames_masked_" + form], bound["mca_hip_mvdr_sources_frames_rtf_" + form]
        assert len(r) == len(m) + 1
        decl = {kind: re.sub(r"\s+", " ", re.search(r"int mca_hip_mvdr_sources_frames_%s_%s\(([^)]*)\)" % (kind, form), text).group(1))
                for kind in ("masked", "rtf")}
        tm = "const float *target_mask_dev, " if form == "dev" else "const float *target_mask, "
        assert decl["rtf"].replace(tm, "") == decl["masked"], (decl["rtf"], decl["masked"])
    assert "target_mask_dev [streams][n_sources][F][K]" in raw and "UNDER-COUNTS" in raw
    # the configuration struct of the header and of the binding agree
    fields = re.search(r"typedef struct \{([^}]*)\} mca_hip_mvdr_rtf_config;", text).group(1)
    assert re.findall(r"(\w+);", fields) == [f[0] for f in _lib.MvdrRtfConfig._fields_]
    assert C.sizeof(_lib.MvdrRtfConfig) == 32


def test_python_and_cxx_classes_take_the_target_mask():
    for name in ("process", "process_dev", "process_sources", "process_sources_dev"):
        p = inspect.signature(getattr(api.MvdrBeamformer, name)).parameters
        assert "target_mask" in p and p["target_mask"].default is None and p["update_mask"].default is None, name
    for name in ("set_rtf", "get_rtf", "set_rtf_workspace", "target_covariance", "steering"):
        assert callable(getattr(api.MvdrBeamformer, name)), name
    assert api.MvdrBeamformer.K_RTF == 5
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("void setRtf(bool enable, double targetAlpha = -1.0, int iterations = 2, int refMic = 0, double minShare = 0.05)",
                 "void steering(double doaRadians, std::vector<double> &d, std::vector<unsigned char> &estimated, int source = 0)",
                 "int processRtf(const std::vector<Tin *> &in, int nSamples, Tout *out, int outSize, const float *updateMask, const float *targetMask)",
                 "int processRtf(const std::vector<Tin *> &in, int nSamples, const std::vector<Tout *> &out, int outSize, const float *updateMask, const float *targetMask)"):
        assert decl in text, decl
    d = inspect.signature(api.MvdrBeamformer.set_rtf).parameters
    assert (d["iterations"].default, d["ref_mic"].default, d["min_share"].default, d["target_alpha"].default) == (2, 0, 0.05, None)


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    buf = (C.c_float * 8)()
    dbl = (C.c_double * 8)()
    cfg = _lib.MvdrRtfConfig()
    cfg.struct_size = C.sizeof(_lib.MvdrRtfConfig)
    assert lib.mca_hip_mvdr_set_rtf(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_get_rtf(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_set_rtf_workspace(None, 1 << 20) == -1
    assert lib.mca_hip_mvdr_sources_frames_rtf_dev(None, buf, 8, 4, 1, 1, 1, buf, buf, buf, buf, buf, None) == -1
    assert lib.mca_hip_mvdr_sources_frames_rtf_dev(None, buf, 8, 4, 1, 1, 1, buf, None, None, buf, buf, None) == -1
    assert lib.mca_hip_mvdr_sources_frames_rtf_host(None, buf, 1, 1, 1, buf, buf, buf, buf, buf) == -1
    assert lib.mca_hip_mvdr_get_steering(None, 0, 0, 0.0, dbl, None) == -1
    assert lib.mca_hip_mvdr_get_target_covariance(None, 0, 0, dbl, dbl) == -1


def _spills():
    import importlib.util
    import shutil
    # the library is built by the ROCm toolchain that ships the tool; without it the register guarantee would go unchecked
    assert shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf"), "llvm-readelf of the ROCm toolchain is needed to read the kernels' register use"
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rtf_kernels_use_no_scratch():
    mod = _spills()
    for name in ("k_mvdr_rtf", "k_mvdr_rtf_steering", "k_mvdr_solve_rtf_t"):
        assert any(re.search(p, name) for p in mod.DEFAULT_PATTERNS), name               # the lint at the link covers them
    every = mod.kernels(_lib.LIB_PATH)
    est = [k for k in every if re.search(r"k_mvdr_rtfI", k.get("name", ""))]
    steer = [k for k in every if "k_mvdr_rtf_steeringI" in k.get("name", "")]
    solve = [k for k in every if "k_mvdr_solve_rtf_tI" in k.get("name", "")]
    # one estimator per number of row slots; a solve per (Q, FULL, S), with and without the noise plane
    assert len(est) == 4 and len(steer) == 4 and len(solve) == 2 * 4 * 2 * 4, (len(est), len(steer), len(solve))
    for k in est + steer + solve:
        assert not any(int(k[f]) for f in mod.FIELDS), (k["name"], [k[f] for f in mod.FIELDS])
        assert int(k["vgpr_count"]) <= 256, k["name"]                                    # two workgroups of four waves per CU
    assert not any(mod.SOLVE_T.search(k["name"]) for k in solve)                         # they are not counted as k_mvdr_solve_t


def test_solve_t_instantiations_are_untouched():
    """the counts the other ABI tests hold k_mvdr_solve_t to, per weight kind"""
    mod = _spills()
    every = mod.kernels(_lib.LIB_PATH)
    assert len(mod.solve_t(every, WEIGHT=2)) == 88 and len(mod.solve_t(every, WEIGHT=2, NOISE=1)) == 44
    assert len(mod.solve_t(every, WEIGHT=1)) == 88 and len(mod.solve_t(every, WEIGHT=0)) == 36
