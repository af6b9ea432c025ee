"""CPU: the interface of the azimuth x elevation Capon map of the MVDR context (mca_hip_mvdr_map_*) and of the elevation per
look-direction slot (mca_hip_mvdr_set_elevations_*) is declared, bound and exposed through the Python and C++ classes; the new
kernels exist and use no scratch, nor do the analysis kernels.  (The refusals need a context: tests/test_gpu_mvdr_map.py and
tests/test_gpu_mvdr_elevations.py.)"""
import ctypes as C
import importlib.util
import inspect
import os
import re
import shutil

import pytest

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_map_configure", "mca_hip_mvdr_map_get_grid", "mca_hip_mvdr_map_dev", "mca_hip_mvdr_map_host",
       "mca_hip_mvdr_set_elevations_host", "mca_hip_mvdr_set_elevations_dev", "mca_hip_mvdr_get_elevations")
FIELDS = ["struct_size", "n_az", "n_el", "el_lo_rad", "el_hi_rad", "bin_lo", "bin_hi", "weighting", "n_peaks"]


def _spills():
    if shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf") is None:
        pytest.skip("no llvm-readelf in this image")
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_and_binding_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    body = re.search(r"typedef struct \{([^}]*)\}\s*mca_hip_mvdr_map_config;", text).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in _lib.MvdrMapConfig._fields_] == FIELDS
    assert C.sizeof(_lib.MvdrMapConfig) == 48 and _lib.MvdrMapConfig.el_lo_rad.offset == 16
    assert api.MvdrBeamformer.K_MAP == 8 and "8 = both kernels of a" in raw
    # a processing parameter, not configuration: the context's struct and the spectrum's are the ones they were
    assert [f for f, _ in _lib.MvdrConfig._fields_] == ["struct_size", "device", "sample_rate", "fft_size", "n_mics", "mic_xyz", "alpha",
                                                        "loading", "max_streams"]
    assert C.sizeof(_lib.MvdrSpectrumConfig) == 24


def test_python_and_cxx_classes_have_the_map():
    for name in ("map_configure", "map_grid", "map", "map_dev", "set_elevations", "set_elevations_dev", "get_elevations"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    p = inspect.signature(api.MvdrBeamformer.map_configure).parameters
    assert list(p)[1:] == ["n_az", "n_el", "el_lo_rad", "el_hi_rad", "bin_lo", "bin_hi", "weighting", "n_peaks"]
    assert (p["n_el"].default, p["el_lo_rad"].default, p["el_hi_rad"].default, p["weighting"].default, p["n_peaks"].default) == (1, None, None, "normalised", 1)
    assert inspect.signature(api.MvdrBeamformer.map).parameters["n_streams"].default is None
    assert list(inspect.signature(api.MvdrBeamformer.map_dev).parameters)[1:] == ["n_streams", "map", "peak_az", "peak_el", "peak_val", "stream"]
    assert list(inspect.signature(api.MvdrBeamformer.set_elevations).parameters)[1:] == ["elev_rad"]
    assert list(inspect.signature(api.MvdrBeamformer.set_elevations_dev).parameters)[1:] == ["n_streams", "elev_rad", "stream"]
    assert inspect.signature(api.MvdrBeamformer.get_elevations).parameters["n_streams"].default is None
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("void setElevations(const std::vector<double> &elevationsRadians)",
                 "void configureMap(int nAz, int nEl, double elLoRad, double elHiRad, int binLo, int binHi, int weighting",
                 "void mapGrid(std::vector<double> &azRadians, std::vector<double> &elRadians) const", "void map(std::vector<double> &values)",
                 "void mapPeaks(std::vector<double> &azRadians, std::vector<double> &elRadians, std::vector<double> &values)"):
        assert decl in text, decl


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    cfg = _lib.MvdrMapConfig(C.sizeof(_lib.MvdrMapConfig), 36, 7, -0.5, 1.0, 1, 100, 1, 1)
    buf = (C.c_float * 252)()
    assert lib.mca_hip_mvdr_map_configure(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_map_get_grid(None, buf, buf) == -1
    assert lib.mca_hip_mvdr_map_dev(None, 1, None, None, None, None, None) == -1
    assert lib.mca_hip_mvdr_map_host(None, 1, buf, None, None, None) == -1
    assert lib.mca_hip_mvdr_set_elevations_host(None, 1, buf) == -1
    assert lib.mca_hip_mvdr_set_elevations_dev(None, 1, None, None) == -1
    assert lib.mca_hip_mvdr_get_elevations(None, 1, buf) == -1


def test_map_kernels_exist_and_use_no_scratch():
    mod = _spills()
    every = mod.kernels(_lib.LIB_PATH)
    scan = [k for k in every if "k_mvdr_map_scan" in k.get("name", "")]
    pick = [k for k in every if "k_mvdr_map_pick" in k.get("name", "")]
    elev = [k for k in every if "k_mvdr_elevations" in k.get("name", "")]
    assert len(scan) == 4 and len(pick) == 1 and len(elev) == 1, [k["name"] for k in scan + pick + elev]   # Q = 1 ... 4 row slots, the pick kernel
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in scan + pick + elev if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
    # two workgroups of four waves per CU: at most 128 VGPRs, and two times the 68 KiB of 16 microphones fit the 160 KiB of a CU
    assert all(int(k["vgpr_count"]) <= 128 for k in scan + pick), [(k["name"], k["vgpr_count"]) for k in scan]
    assert 2 * 64 * (136 * 8 + 4) <= 160 * 1024
    assert int(pick[0]["group_segment_fixed_size"]) <= 16 * 1024
    # the names hold none of the substrings whose counts the other ABI tests pin
    for k in scan + pick + elev:
        assert not any(s in k["name"] for s in ("k_mvdr_spectrum", "k_mvdr_track", "k_mvdr_analyse", "k_mvdr_rtfI", "k_mvdr_estmaskI", "k_mvdr_postfilter", "k_mvdr_solve"))


def test_the_analysis_kernels_still_use_no_scratch():
    mod = _spills()
    ks = [k for k in mod.kernels(_lib.LIB_PATH) if "k_mvdr_analyse" in k.get("name", "")]
    assert len(ks) == 3, [k["name"] for k in ks]
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in ks if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
