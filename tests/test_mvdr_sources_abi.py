"""CPU: the interface of the multi-source MVDR call (mca_hip_mvdr_set_max_sources, mca_hip_mvdr_sources_frames_dev / _host) is
declared, bound and exposed, the create path still fails loudly without a GPU, and the premise that lets S look directions share
one covariance recursion and one factorisation holds in the oracle: the covariance does not depend on the look direction."""
import os
import re

import numpy as np
import pytest

from mcarray_amd import _lib, api, synth
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_set_max_sources", "mca_hip_mvdr_sources_frames_dev", "mca_hip_mvdr_sources_frames_host")


def test_header_declares_and_binding_binds_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in NEW:
        assert name in declared, name
        assert name in bound, name
    # the sources calls take the single-look calls' arguments plus n_sources
    assert len(bound["mca_hip_mvdr_sources_frames_dev"]) == len(bound["mca_hip_mvdr_frames_dev"]) + 1
    assert len(bound["mca_hip_mvdr_sources_frames_host"]) == len(bound["mca_hip_mvdr_frames_host"]) + 1
    # opt-in: the configuration struct is the one it was
    assert [f for f, _ in _lib.MvdrConfig._fields_] == ["struct_size", "device", "sample_rate", "fft_size", "n_mics", "mic_xyz", "alpha",
                                                        "loading", "max_streams"]


def test_python_class_has_the_sources_calls():
    import inspect
    for name in ("process_sources", "process_sources_dev", "set_max_sources"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    sig = inspect.signature(api.MvdrBeamformer.__init__)
    assert sig.parameters["max_sources"].default == 1


def test_create_with_sources_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(api.MCArrayHipError, match="no CPU fallback"):
        api.MvdrBeamformer(48000, synth.ULA8, 1024, max_sources=2)


def test_oracle_covariance_does_not_depend_on_the_look_direction():
    fs, N, F = 16000, 256, 12
    xs = synth.REEM_C
    n = (F + 1) * N // 2
    pcm = (synth.noise_source_stream(xs, 0.3, fs, n, 3) + synth.noise_source_stream(xs, -0.8, fs, n, 4)).astype(np.float64)
    rng = np.random.default_rng(0)
    a, b = po.MVDR(fs, N, xs), po.MVDR(fs, N, xs)
    oa = a.stream(pcm, rng.uniform(-1.3, 1.3, F), want_spec=True)
    ob = b.stream(pcm, rng.uniform(-1.3, 1.3, F), want_spec=True)
    assert np.array_equal(a.covariance(), b.covariance())
    assert not np.array_equal(oa["spec"], ob["spec"])


def test_no_mvdr_solve_kernel_spills():
    """the instantiations for 13 ... 16 microphones sit a register or two under the budget; none may go to
    scratch.  The lint reads the kernel metadata of the built library (no GPU needed)."""
    import importlib.util
    import shutil
    if shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf") is None:
        pytest.skip("no llvm-readelf in this image")
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    every = mod.kernels(_lib.LIB_PATH)
    single = [k for k in every if "k_mvdr_solveI" in k.get("name", "")]            # the hand-written k_mvdr_solve<Q, FULL>
    sources = mod.solve_t(every, WEIGHT=0, NULLS=0)                                # k_mvdr_solve_t without weights and nulls
    assert (len(single), len(sources)) == (8, 24), (len(single), len(sources))     # 8 single-look instantiations, 24 of several directions
    ks = single + sources
    assert all(int(k["vgpr_count"]) <= 256 for k in ks)
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in ks if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
