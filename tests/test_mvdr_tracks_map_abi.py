"""CPU: the interface of the map mode of the tracks of the MVDR context (mca_hip_mvdr_tracks_*_map) is declared, bound and exposed
through the Python and C++ classes, its kernels exist without scratch under names that hold none of the substrings the other ABI
tests count, and those counts are unchanged.  (The refusals need a context: tests/test_gpu_mvdr_tracks_map.py.)"""
import ctypes as C
import importlib.util
import inspect
import os
import re
import shutil

import pytest

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_tracks_set_map", "mca_hip_mvdr_tracks_get_map_config", "mca_hip_mvdr_tracks_seed_map_dev", "mca_hip_mvdr_tracks_seed_map_host",
       "mca_hip_mvdr_tracks_update_map_dev", "mca_hip_mvdr_tracks_update_map_host", "mca_hip_mvdr_tracks_associate_map_dev", "mca_hip_mvdr_tracks_get_map")
PINNED = ("k_mvdr_track", "k_mvdr_spectrum", "k_mvdr_map_scan", "k_mvdr_map_pick", "k_mvdr_elevations", "k_mvdr_analyse", "k_mvdr_rtfI",
          "k_mvdr_rtf_steeringI", "k_mvdr_estmaskI", "k_mvdr_postfilter", "k_mvdr_solve")


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
    body = re.search(r"typedef struct \{([^}]*)\}\s*mca_hip_mvdr_tracks_map_config;", text).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f for f, _ in _lib.MvdrTracksMapConfig._fields_] == ["struct_size", "enable", "max_step_el_rad", "min_sep_el_rad"]
    assert C.sizeof(_lib.MvdrTracksMapConfig) == 24 and _lib.MvdrTracksMapConfig.max_step_el_rad.offset == 8
    # the tracks' own struct is the one it was
    assert C.sizeof(_lib.MvdrTracksConfig) == 40
    assert [f for f, _ in _lib.MvdrTracksConfig._fields_] == ["struct_size", "enable", "n_tracks", "n_own", "max_step_rad", "min_sep_rad", "hold"]
    assert api.MvdrBeamformer.K_TRACKS_MAP == 9 and "9 = the kernels of the tracks' map mode" in raw
    assert "loses its meaning near eps = +-pi/2" in raw                   # the header says what the grid-angle distance cannot do


def test_python_and_cxx_classes_have_the_map_mode():
    for name in ("configure_tracks_map", "get_tracks_map_config", "seed_tracks_map", "seed_tracks_map_dev", "update_tracks_map", "update_tracks_map_dev",
                 "associate_tracks_map_dev", "tracks_map", "follow_tracks"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    assert list(inspect.signature(api.MvdrBeamformer.configure_tracks_map).parameters)[1:] == ["max_step_el_rad", "min_sep_el_rad", "enable"]
    assert inspect.signature(api.MvdrBeamformer.update_tracks_map).parameters["want_map"].default is False
    assert list(inspect.signature(api.MvdrBeamformer.associate_tracks_map_dev).parameters)[1:] == ["n_streams", "own_az", "own_el", "cand_az", "cand_el", "cand_val",
                                                                                                   "stream"]
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("void configureTracksMap(double maxStepElRadians, double minSepElRadians", "void seedTracksMap(const std::vector<double> &azRadians",
                 "void updateTracksMap()", "void tracksMap(std::vector<double> &azRadians, std::vector<double> &elRadians"):
        assert decl in text, decl


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    cfg = _lib.MvdrTracksMapConfig(C.sizeof(_lib.MvdrTracksMapConfig), 1, 0.2, 0.1)
    f = (C.c_float * 8)()
    i = (C.c_int * 8)()
    assert lib.mca_hip_mvdr_tracks_set_map(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_tracks_get_map_config(None, C.byref(cfg)) == -1
    assert lib.mca_hip_mvdr_tracks_seed_map_dev(None, 1, None, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_seed_map_host(None, 1, f, f) == -1
    assert lib.mca_hip_mvdr_tracks_update_map_dev(None, 1, None, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_update_map_host(None, 1, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_associate_map_dev(None, 1, None, None, 1, None, None, None, None) == -1
    assert lib.mca_hip_mvdr_tracks_get_map(None, 1, f, f, i, i, i) == -1


def test_trk2_kernels_exist_without_scratch_under_names_no_other_test_counts():
    mod = _spills()
    ks = [k for k in mod.kernels(_lib.LIB_PATH) if "k_mvdr_trk2" in k.get("name", "")]
    names = sorted(k["name"] for k in ks)
    assert len(ks) == 9, names                           # tables, vectors<Q = 1 ... 4>, scan, pick, fill, seed
    assert sum("k_mvdr_trk2_vectorsI" in n for n in names) == 4
    for part in ("tables", "scan", "pick", "fill", "seed"):
        assert sum("k_mvdr_trk2_" + part in n for n in names) == 1, part
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in ks if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
    assert all(int(k["vgpr_count"]) <= 256 for k in ks)  # two workgroups of four waves per CU
    scan = [k for k in ks if "k_mvdr_trk2_scan" in k["name"]][0]
    assert int(scan["vgpr_count"]) <= 128 and int(scan["group_segment_fixed_size"]) <= 16 * 1024
    assert any(re.search(p, "k_mvdr_trk2_vectors") for p in mod.DEFAULT_PATTERNS)        # the lint at the link covers them
    for n in names:
        assert not any(s in n for s in PINNED), n


def test_the_counts_of_the_other_kernels_are_unchanged():
    mod = _spills()
    every = mod.kernels(_lib.LIB_PATH)
    names = [k.get("name", "") for k in every]
    assert sum("k_mvdr_track" in n for n in names) == 8 and sum("k_mvdr_track_spectrumI" in n for n in names) == 4
    assert sum("k_mvdr_spectrum" in n for n in names) == 5 and sum("k_mvdr_analyse" in n for n in names) == 3
    assert sum("k_mvdr_map_scan" in n for n in names) == 4 and sum("k_mvdr_map_pick" in n for n in names) == 1 and sum("k_mvdr_elevations" in n for n in names) == 1
    assert sum("k_mvdr_rtfI" in n for n in names) == 4 and sum("k_mvdr_rtf_steeringI" in n for n in names) == 4
    assert sum("k_mvdr_estmaskI" in n for n in names) == 4 and sum("k_mvdr_postfilter" in n for n in names) == 1
    assert len(mod.solve_t(every, WEIGHT=2)) == 88 and len(mod.solve_t(every, WEIGHT=2, NOISE=1)) == 44
    assert len(mod.solve_t(every, WEIGHT=1)) == 88 and len(mod.solve_t(every, WEIGHT=0)) == 36
    assert sum("k_mvdr_solve_rtf_tI" in n for n in names) == 2 * 4 * 2 * 4
    assert sum("k_mvdr_solve_rtf_nulls_tI" in n for n in names) == 24
