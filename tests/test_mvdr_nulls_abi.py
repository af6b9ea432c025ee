"""CPU: the interface of the soft nulls of the MVDR sources call (mca_hip_mvdr_set_null_gain / _get_null_gain) is declared, bound
and exposed, the create path still fails loudly without a GPU, and no instantiation of the new solve kernel goes to scratch."""
import inspect
import os
import re

import pytest

from mcarray_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_mvdr_set_null_gain", "mca_hip_mvdr_get_null_gain")


def test_header_declares_and_binding_binds_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_[a-z0-9_]+)\s*\(", text))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # a processing parameter, not configuration: the struct is the one it was
    assert [f for f, _ in _lib.MvdrConfig._fields_] == ["struct_size", "device", "sample_rate", "fft_size", "n_mics", "mic_xyz", "alpha",
                                                        "loading", "max_streams"]


def test_python_and_cxx_classes_have_the_gain():
    for name in ("set_null_gain", "get_null_gain"):
        assert callable(getattr(api.MvdrBeamformer, name, None)), name
    assert inspect.signature(api.MvdrBeamformer.__init__).parameters["null_gain"].default == 0.0
    text = open(os.path.join(ROOT, "include", "mcarray", "MvdrBeamformer.h")).read()
    assert "void setNullGain(double" in text and "double getNullGain() const" in text


def test_create_with_a_gain_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(api.MCArrayHipError, match="no CPU fallback"):
        api.MvdrBeamformer(48000, synth.ULA8, 1024, max_sources=2, null_gain=100.0)


def test_no_nulls_kernel_spills():
    """one instantiation per (row slots, look directions); those for 13 ... 16 microphones sit a few registers
    under the budget of two workgroups per CU.  The lint reads the kernel metadata of the built library (no GPU needed) and covers
    the new kernels by its default pattern."""
    import importlib.util
    import shutil
    if shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf") is None:
        pytest.skip("no llvm-readelf in this image")
    spec = importlib.util.spec_from_file_location("check_spills", os.path.join(ROOT, "tools", "check_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    every = mod.kernels(_lib.LIB_PATH)
    ks = mod.solve_t(every, WEIGHT=0, NULLS=1)          # k_mvdr_solve_t<..., NULLS = true, ...> without weights
    assert len(ks) == 12, len(ks)                       # Q = 1 ... 4 row slots x S = 2 ... 4 look directions
    assert all(int(k["vgpr_count"]) <= 256 for k in ks)
    bad = {k["name"]: [k[f] for f in mod.FIELDS] for k in ks if any(int(k[f]) for f in mod.FIELDS)}
    assert not bad, bad
    # the lint's default pattern covers them beside the 32 kernels without weights that it covered before
    default = re.compile(mod.DEFAULT_PATTERNS[0])
    assert all(default.search(k["name"]) for k in ks)
    assert sum(1 for k in every if default.search(k.get("name", "")) and not mod.solve_t([k], WEIGHT=1) and not mod.solve_t([k], WEIGHT=2)) == 44
