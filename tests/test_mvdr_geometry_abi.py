"""CPU: the geometry setter of the MVDR context (mca_hip_mvdr_set_geometry / _get_geometry) is declared, bound and exposed through the
Python class and synth, the kernels it touches use no scratch, and the kernel counts the other ABI tests hold are unchanged."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from mcarray_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_set_geometry", "mca_hip_mvdr_get_geometry")


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
    body = re.search(r"typedef struct \{([^}]*)\}\s*mca_hip_mvdr_geometry_config;", text).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in _lib.MvdrGeometryConfig._fields_] == ["struct_size", "mode", "elevation_rad"]
    assert C.sizeof(_lib.MvdrGeometryConfig) == 16
    assert re.search(r"#define \w+_MVDR_GEOMETRY_LINEAR_X 0\b", text) and re.search(r"#define \w+_MVDR_GEOMETRY_XYZ 1\b", text)
    assert (api.MvdrBeamformer.GEOMETRY_LINEAR_X, api.MvdrBeamformer.GEOMETRY_XYZ) == (0, 1)
    # a setter, not configuration: the context's struct is the one it was
    assert [f for f, _ in _lib.MvdrConfig._fields_] == ["struct_size", "device", "sample_rate", "fft_size", "n_mics", "mic_xyz", "alpha",
                                                        "loading", "max_streams"]


def test_python_class_and_synth_have_the_geometry():
    for name in ("set_geometry", "get_geometry"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    p = inspect.signature(api.MvdrBeamformer.set_geometry).parameters
    assert list(p)[1:] == ["mode", "elevation_rad"] and p["elevation_rad"].default == 0.0
    p = inspect.signature(api.MvdrBeamformer.__init__).parameters
    assert p["geometry"].default == "linear_x" and p["elevation_rad"].default == 0.0
    assert list(p).index("elevation_rad") == list(p).index("geometry") + 1 > list(p).index("device")      # behind every argument a caller passes by position
    p = inspect.signature(synth.noise_source_stream_xyz).parameters
    assert list(p) == ["xyz", "azimuth", "fs", "n_samples", "seed", "sigma", "snr_db", "elevation"] and p["elevation"].default == 0.0
    assert list(inspect.signature(synth.delay_channels_xyz).parameters) == ["s", "xyz", "azimuth", "fs", "elevation"]
    u = synth.uca(6, 0.045)
    assert u.shape == (6, 3) and u.dtype == np.float64 and np.all(u[:, 2] == 0.0)
    assert np.allclose(np.hypot(u[:, 0], u[:, 1]), 0.045, atol=1e-15) and np.allclose(u[0], [0.045, 0.0, 0.0])


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    cfg = _lib.MvdrGeometryConfig(C.sizeof(_lib.MvdrGeometryConfig), 1, 0.0)
    assert lib.mca_hip_mvdr_set_geometry(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_get_geometry(None, C.byref(cfg)) == -1


def test_touched_kernels_use_no_scratch():
    mod = _spills()
    touched = ("k_mvdr_analyse", "k_mvdr_track_tables", "k_mvdr_track_pick", "k_mvdr_track_seed", "k_mvdr_spectrum_pick")
    ks = [k for k in mod.kernels(_lib.LIB_PATH) if any(t in k.get("name", "") for t in touched)]
    names = sorted(k["name"] for k in ks)
    assert len(ks) == 7, names                           # analyse, _1024, _512, track tables / pick / seed, spectrum pick
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in ks if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad


def test_the_counts_of_the_other_kernels_are_unchanged():
    mod = _spills()
    every = mod.kernels(_lib.LIB_PATH)
    names = [k.get("name", "") for k in every]
    assert sum("k_mvdr_spectrum" in n for n in names) == 5 and sum("k_mvdr_track" in n for n in names) == 8
    assert sum("k_mvdr_rtfI" in n for n in names) == 4 and sum("k_mvdr_estmaskI" in n for n in names) == 4
    assert sum("k_mvdr_postfilter" in n for n in names) == 1 and sum("k_mvdr_analyse" in n for n in names) == 3
    assert len(mod.solve_t(every, WEIGHT=2)) == 88 and len(mod.solve_t(every, WEIGHT=1)) == 88 and len(mod.solve_t(every, WEIGHT=0)) == 36
