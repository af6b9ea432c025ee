"""CPU: the interface of the Capon spatial spectrum of the MVDR context (mca_hip_mvdr_spectrum_*) is declared, bound and exposed
through the Python and C++ classes, and its kernels use no scratch."""
import ctypes as C
import inspect
import os
import re

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_spectrum_configure", "mca_hip_mvdr_spectrum_get_grid", "mca_hip_mvdr_spectrum_dev", "mca_hip_mvdr_spectrum_host")


def test_header_declares_and_binding_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # the struct of the header, field for field, and the two weightings
    body = re.search(r"typedef struct \{([^}]*)\}\s*mca_hip_mvdr_spectrum_config;", text).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip()[len("int"):].split(",")]
    assert fields == [f for f, _ in _lib.MvdrSpectrumConfig._fields_] == ["struct_size", "n_angles", "bin_lo", "bin_hi", "weighting", "n_peaks"]
    assert C.sizeof(_lib.MvdrSpectrumConfig) == 24
    assert dict(re.findall(r"#define\s+\w+_MVDR_SPECTRUM_(\w+)\s+(\d+)\b", text)) == {"POWER": "0", "NORMALISED": "1"}
    assert (api.MvdrBeamformer.SPECTRUM_POWER, api.MvdrBeamformer.SPECTRUM_NORMALISED, api.MvdrBeamformer.K_SPECTRUM) == (0, 1, 3)
    # a processing parameter, not configuration: the context's struct is the one it was
    assert [f for f, _ in _lib.MvdrConfig._fields_] == ["struct_size", "device", "sample_rate", "fft_size", "n_mics", "mic_xyz", "alpha",
                                                        "loading", "max_streams"]
    assert "kernel_id 0 = analysis, 1 = solve, 2 = synthesis" in raw and "3 = spectrum" in raw


def test_python_and_cxx_classes_have_the_spectrum():
    for name in ("configure_spectrum", "spectrum_grid", "spectrum", "spectrum_dev"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    p = inspect.signature(api.MvdrBeamformer.configure_spectrum).parameters
    assert list(p)[1:] == ["n_angles", "bin_lo", "bin_hi", "weighting", "n_peaks"]
    assert (p["bin_lo"].default, p["bin_hi"].default, p["weighting"].default, p["n_peaks"].default) == (None, None, "normalised", 1)
    assert inspect.signature(api.MvdrBeamformer.spectrum).parameters["n_streams"].default is None
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("void configureSpectrum(int nAngles, int binLo, int binHi, int weighting", "std::vector<double> spectrumGrid() const",
                 "void spectrum(std::vector<double> &", "void peaks(std::vector<double> &doaRadians, std::vector<double> &values)"):
        assert decl in text, decl


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    cfg = _lib.MvdrSpectrumConfig(C.sizeof(_lib.MvdrSpectrumConfig), 61, 1, 100, 1, 1)
    buf = (C.c_float * 61)()
    assert lib.mca_hip_mvdr_spectrum_configure(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_spectrum_get_grid(None, buf) == -1
    assert lib.mca_hip_mvdr_spectrum_dev(None, 1, None, None, None, None) == -1
    assert lib.mca_hip_mvdr_spectrum_host(None, 1, buf, None, None) == -1


def test_spectrum_kernels_use_no_scratch():
    import importlib.util
    import shutil
    import pytest
    if shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf") is None:
        pytest.skip("no llvm-readelf in this image")
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = [k for k in mod.kernels(_lib.LIB_PATH) if "k_mvdr_spectrum" in k.get("name", "")]
    assert len(ks) == 5, len(ks)                        # Q = 1 ... 4 row slots and the pick kernel
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in ks if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
    assert all(int(k["vgpr_count"]) <= 128 for k in ks)  # two workgroups of four waves per CU with room to spare
