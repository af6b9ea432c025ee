"""CPU: FreqGCCBinauralLocalisation::setProbability at caller-given angles and the per-frame hook exist at every layer -- the
library exports the four C entry points, the C++ class overrides setProbability and SourceSeparationAndLocalisation has the
SignalVector& hook overload of the reference, and the Python API has the methods (the GPU runs are in
tests/test_gpu_gcc2_probability.py)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from mcarray_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mca_hip_gcc2_set_probability", "mca_hip_gcc2_set_probability_dev", "mca_hip_gcc2_process_frame",
       "mca_hip_gcc2_frame_set_probability")


def test_library_exports_the_gcc2_probability_entry_points():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in bound, name


CXX_CHECK = r"""
#include <type_traits>
#include <vector>
#include "mcarray/BinauralLocalisation.h"
#include "mcarray/SourceSeparationAndLocalisation.h"

// FreqGCCBinauralLocalisation overrides setProbability (BinauralLocalisation.h:192 of the reference)
static_assert(!std::is_same<decltype(&mca::FreqGCCBinauralLocalisation::setProbability),
                            decltype(&mca::SoundLocalisationImpl::setProbability)>::value, "");

void hook_calls(mca::FreqGCCBinauralLocalisation &g, mca::SourceSeparationAndLocalisation &s, mca::SignalVector &sf,
                std::vector<double *> &frames, std::vector<double *> &data)
{
    s.processParametrisation(sf, 1026, data, 512);          // the SignalVector& overload (SourceSeparationAndLocalisation.h:68)
    s.processParametrisation(frames, 1026, data, 512);
    g.processParametrisation(frames, 1026, data, 512);
    mca::SoundLocalisationImpl &impl = g;
    double doas[2] = {0.1, -0.2}, probs[2];
    impl.setProbability(doas, probs, 2);
}
"""


def test_cxx_api_has_the_override_and_the_signalvector_hook(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ in this image")
    src = tmp_path / "check.cpp"
    src.write_text(CXX_CHECK)
    r = subprocess.run([cxx, "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_python_api_has_the_methods():
    for m in ("gcc2_set_probability", "gcc2_set_probability_dev", "gcc2_process_frame", "gcc2_frame_set_probability",
              "gcc2_frames_dev"):
        assert callable(getattr(api.Context, m, None)), m
    for m in ("set_probability", "process_frame"):
        assert callable(getattr(api.FreqGCCBinauralLocalisation, m, None)), m
