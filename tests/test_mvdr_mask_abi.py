"""CPU: the interface of the time-frequency update masks of the MVDR context (mca_hip_mvdr_sources_frames_masked_*) is declared,
bound, present in the built library and exposed through the Python and C++ classes, and its kernels -- every instantiation of
k_mvdr_solve_t<..., WEIGHT = CELL, ...> -- use no scratch."""
import ctypes as C
import inspect
import os
import re

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_sources_frames_masked_dev", "mca_hip_mvdr_sources_frames_masked_host")


def test_header_declares_and_binding_binds_the_new_symbols():
    raw = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # the argument lists are those of the weighted calls
    for form in ("dev", "host"):
        assert bound["mca_hip_mvdr_sources_frames_masked_" + form] == bound["mca_hip_mvdr_sources_frames_weighted_" + form]
        decl = {kind: re.search(r"int mca_hip_mvdr_sources_frames_%s_%s\(([^)]*)\)" % (kind, form), text).group(1) for kind in ("masked", "weighted")}
        strip = lambda s: re.sub(r"\s+", " ", s).replace("update_mask", "update")
        assert strip(decl["masked"]) == strip(decl["weighted"])
    assert "update_mask_dev [streams][F][K]" in raw


def test_python_and_cxx_classes_take_the_mask():
    for name in ("process", "process_dev", "process_sources", "process_sources_dev"):
        p = inspect.signature(getattr(api.MvdrBeamformer, name)).parameters
        assert "update_mask" in p and p["update_mask"].default is None and p["update"].default is None, name
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    for decl in ("int framesCompletedBy(int nSamples) const",
                 "int process(const std::vector<Tin *> &in, int nSamples, Tout *out, int outSize, const float *updateMask = nullptr)",
                 "int process(const std::vector<Tin *> &in, int nSamples, const std::vector<Tout *> &out, int outSize, const float *updateMask = nullptr)"):
        assert decl in text, decl


def test_decisions_of_the_masking_modules_become_a_mask():
    """0 = enhance (the target's band) closes the cells, 1 and 2 (temporal / spatial mask) open them; a bin takes the band with the
    nearest centre; the bins outside the centres take the end bands"""
    import numpy as np
    N, K = 1024, 513
    cen = np.linspace(0.01, 0.45, 45) ** 1.3                   # ascending, unevenly spaced, cycles per sample
    dec = np.random.default_rng(0).integers(0, 3, size=(2, 5, 45)).astype(np.int32)
    m = api.update_mask_from_decisions(dec, cen, N)
    assert m.shape == (2, 5, K) and m.dtype == np.float32 and m.flags["C_CONTIGUOUS"]
    for k in (0, 1, 17, 100, 256, 400, 512):
        b = int(np.argmin(np.abs(cen - k / N)))
        assert np.array_equal(m[:, :, k], (dec[:, :, b] != 0).astype(np.float32)), k
    only = np.zeros((1, 45), dtype=np.int32)
    only[0, 20] = 2                                             # one masked band: its bins open, all others closed
    m = api.update_mask_from_decisions(only, cen, N)[0]
    lo, hi = 0.5 * (cen[19] + cen[20]) * N, 0.5 * (cen[20] + cen[21]) * N
    assert np.array_equal(np.flatnonzero(m), np.arange(int(np.floor(lo)) + 1, int(np.floor(hi)) + 1))
    assert not api.update_mask_from_decisions(np.zeros((3, 45), dtype=np.int32), cen, N).any()      # everything enhanced: learn nothing
    import pytest
    with pytest.raises(api.MCArrayHipError):
        api.update_mask_from_decisions(np.zeros((3, 44), dtype=np.int32), cen, N)


def test_null_context_is_refused_without_a_gpu():
    lib = _lib.load()
    buf = (C.c_float * 8)()
    assert lib.mca_hip_mvdr_sources_frames_masked_dev(None, buf, 8, 4, 1, 1, 1, buf, buf, buf, buf, None) == -1
    assert lib.mca_hip_mvdr_sources_frames_masked_host(None, buf, 1, 1, 1, buf, buf, buf, buf) == -1
    assert lib.mca_hip_mvdr_sources_frames_masked_dev(None, buf, 8, 4, 1, 1, 1, buf, None, buf, buf, None) == -1


def test_masked_kernels_use_no_scratch():
    import importlib.util
    import shutil
    # the library is built by the ROCm toolchain that ships the tool; without it the register guarantee would go unchecked
    assert shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf"), "llvm-readelf of the ROCm toolchain is needed to read the kernels' register use"
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert any(re.search(p, "k_mvdr_solve_t") for p in mod.DEFAULT_PATTERNS)             # the lint at the link covers them
    every = mod.kernels(_lib.LIB_PATH)
    masked = mod.solve_t(every, WEIGHT=2)
    # one per kernel with a weight per frame: with and without the noise plane, REUSE never under a mask
    noise = mod.solve_t(every, WEIGHT=2, NOISE=1)
    assert len(masked) == 88 and len(noise) == 44, (len(masked), len(noise))
    assert masked == mod.solve_t(every, WEIGHT=2, REUSE=0)
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in masked if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
    assert all(int(k["vgpr_count"]) <= 256 for k in masked)    # two workgroups of four waves per CU (__launch_bounds__(256, 2))
