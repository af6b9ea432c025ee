"""CPU: the interface of the tracks of the look directions of the MVDR context (mca_hip_mvdr_tracks_*) is declared, bound and exposed
through the Python class, its kernels use no scratch, and the kernel counts the other ABI tests hold are unchanged."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import shutil

import pytest

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_tracks_configure", "mca_hip_mvdr_tracks_get_config", "mca_hip_mvdr_tracks_seed_dev", "mca_hip_mvdr_tracks_seed_host",
       "mca_hip_mvdr_tracks_update_dev", "mca_hip_mvdr_tracks_update_host", "mca_hip_mvdr_tracks_associate_dev", "mca_hip_mvdr_tracks_fill_dev", "mca_hip_mvdr_tracks_fill_host",
       "mca_hip_mvdr_tracks_get")


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
    body = re.search(r"typedef struct \{([^}]*)\}\s*mca_hip_mvdr_tracks_config;", text).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in _lib.MvdrTracksConfig._fields_] == ["struct_size", "enable", "n_tracks", "n_own", "max_step_rad", "min_sep_rad", "hold"]
    assert C.sizeof(_lib.MvdrTracksConfig) == 40
    assert api.MvdrBeamformer.K_TRACKS == 7 and "7 = the track" in raw
    # a processing parameter, not configuration: the context's struct is the one it was
    assert [f for f, _ in _lib.MvdrConfig._fields_] == ["struct_size", "device", "sample_rate", "fft_size", "n_mics", "mic_xyz", "alpha",
                                                        "loading", "max_streams"]


def test_python_class_has_the_tracks():
    for name in ("configure_tracks", "get_tracks_config", "seed_tracks", "seed_tracks_dev", "update_tracks", "update_tracks_dev", "associate_tracks_dev",
                 "fill_tracks_dev", "tracks", "follow_tracks"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    p = inspect.signature(api.MvdrBeamformer.configure_tracks).parameters
    assert list(p)[1:] == ["n_tracks", "n_own", "max_step_rad", "min_sep_rad", "hold", "enable"]


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    cfg = _lib.MvdrTracksConfig(C.sizeof(_lib.MvdrTracksConfig), 1, 2, 0, 0.2, 0.1, 3)
    f = (C.c_float * 8)()
    i = (C.c_int * 8)()
    assert lib.mca_hip_mvdr_tracks_configure(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_tracks_get_config(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_tracks_seed_dev(None, 1, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_seed_host(None, 1, f) == -1
    assert lib.mca_hip_mvdr_tracks_update_dev(None, 1, None, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_update_host(None, 1, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_associate_dev(None, 1, None, 1, None, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_fill_dev(None, 1, 1, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_fill_host(None, 1, 1, f) == -1
    assert lib.mca_hip_mvdr_tracks_get(None, 1, f, i, i, i) == -1


def test_track_kernels_use_no_scratch():
    mod = _spills()
    ks = [k for k in mod.kernels(_lib.LIB_PATH) if "k_mvdr_track" in k.get("name", "")]
    names = sorted(k["name"] for k in ks)
    assert len(ks) == 8, names                           # tables, spectrum<Q = 1 ... 4>, pick, fill, seed
    assert sum("k_mvdr_track_spectrumI" in n for n in names) == 4
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in ks if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
    assert all(int(k["vgpr_count"]) <= 256 for k in ks)  # two workgroups of four waves per CU
    assert any(re.search(p, "k_mvdr_track_spectrum") for p in mod.DEFAULT_PATTERNS)      # the lint at the link covers them


def test_the_counts_of_the_other_kernels_are_unchanged():
    mod = _spills()
    names = [k.get("name", "") for k in mod.kernels(_lib.LIB_PATH)]
    assert sum("k_mvdr_spectrum" in n for n in names) == 5
    assert sum("k_mvdr_rtfI" in n for n in names) == 4 and sum("k_mvdr_rtf_steeringI" in n for n in names) == 4
    assert sum("k_mvdr_estmaskI" in n for n in names) == 4 and sum("k_mvdr_postfilter" in n for n in names) == 1
    # mvdr_rtf.h includes mvdr_solve.h and a second unit now includes both: the solve instantiations are the ones they were
    every = mod.kernels(_lib.LIB_PATH)
    assert len(mod.solve_t(every, WEIGHT=2)) == 88 and len(mod.solve_t(every, WEIGHT=2, NOISE=1)) == 44
    assert len(mod.solve_t(every, WEIGHT=1)) == 88 and len(mod.solve_t(every, WEIGHT=0)) == 36
    assert sum("k_mvdr_solve_rtf_tI" in n for n in names) == 2 * 4 * 2 * 4
    assert sum("k_mvdr_solve_rtf_nulls_tI" in n for n in names) == 24
