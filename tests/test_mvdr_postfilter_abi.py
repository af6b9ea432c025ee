"""CPU: the interface of the Wiener post-filter of the MVDR context (mca_hip_mvdr_set_postfilter / _get_postfilter) is declared,
bound and exposed through the Python and C++ classes, and its kernels -- k_mvdr_postfilter and every instantiation of the gated solve
that emits the noise plane -- use no scratch."""
import ctypes as C
import inspect
import os
import re

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_set_postfilter", "mca_hip_mvdr_get_postfilter")


def test_header_declares_and_binding_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # the struct of the header, field for field
    body = re.search(r"typedef struct \{([^}]*)\}\s*mca_hip_mvdr_postfilter_config;", text).group(1)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert decls == [["int", "struct_size"], ["int", "enable"], ["double", "smoothing"], ["double", "gain_floor"], ["double", "noise_scale"]]
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in decls] == list(_lib.MvdrPostfilterConfig._fields_)
    assert C.sizeof(_lib.MvdrPostfilterConfig) == 32
    assert api.MvdrBeamformer.K_POSTFILTER == 4
    assert "kernel_id 0 = analysis, 1 = solve, 2 = synthesis" in raw and "3 = spectrum" in raw and "4 = post-filter" in raw
    # a processing parameter, not configuration: the context's struct is the one it was
    assert [f for f, _ in _lib.MvdrConfig._fields_] == ["struct_size", "device", "sample_rate", "fft_size", "n_mics", "mic_xyz", "alpha",
                                                        "loading", "max_streams"]


def test_python_and_cxx_classes_have_the_postfilter():
    for name in ("set_postfilter", "get_postfilter"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    p = inspect.signature(api.MvdrBeamformer.set_postfilter).parameters
    assert list(p)[1:] == ["enable", "smoothing", "gain_floor", "noise_scale"]
    assert (p["enable"].default, p["smoothing"].default, p["gain_floor"].default, p["noise_scale"].default) == (True, 0.98, 0.1, 1.0)
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("void setPostFilter(bool enable, double smoothing = 0.98, double gainFloor = 0.1, double noiseScale = 1.0)",
                 "void getPostFilter(bool &enable, double &smoothing, double &gainFloor, double &noiseScale) const"):
        assert decl in text, decl


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    cfg = _lib.MvdrPostfilterConfig(C.sizeof(_lib.MvdrPostfilterConfig), 1, 0.98, 0.1, 1.0)
    assert lib.mca_hip_mvdr_set_postfilter(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_get_postfilter(None, C.byref(cfg)) == -1
    assert (cfg.enable, cfg.smoothing, cfg.gain_floor, cfg.noise_scale) == (1, 0.98, 0.1, 1.0)


def test_postfilter_kernels_use_no_scratch():
    import importlib.util
    import shutil
    import pytest
    if shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf") is None:
        pytest.skip("no llvm-readelf in this image")
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert any(re.search(p, "k_mvdr_postfilter") for p in mod.DEFAULT_PATTERNS)           # the lint at the link covers it
    assert any(re.search(p, "k_mvdr_solve_t") for p in mod.DEFAULT_PATTERNS)
    all_k = mod.kernels(_lib.LIB_PATH)
    pf = [k for k in all_k if "k_mvdr_postfilter" in k.get("name", "")]
    # the solve with a weight per frame: with and without the noise plane
    gated = mod.solve_t(all_k, WEIGHT=1)
    noise = mod.solve_t(all_k, WEIGHT=1, NOISE=1)
    assert len(pf) == 1 and len(gated) == 88 and len(noise) == 44, (len(pf), len(gated), len(noise))
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in pf + noise if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
    assert all(int(k["vgpr_count"]) <= 256 for k in noise)     # two workgroups of four waves per CU (__launch_bounds__(256, 2))
    assert int(pf[0]["vgpr_count"]) <= 64                      # memory-bound: every wave slot of a SIMD stays usable
