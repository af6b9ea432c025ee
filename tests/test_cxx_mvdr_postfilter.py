"""Builds and runs the C++ test of mca::MvdrBeamformer::setPostFilter / getPostFilter (tests/cxx/test_mvdr_postfilter.cpp): gain
floor 1 reproduces an unfiltered run through both process() overloads, a filtered run lowers the power of an interferer alone, and
the getter round-trips."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cxx_postfilter_on_gpu(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_mvdr_postfilter"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_mvdr_postfilter.cpp"), "-o", str(exe), "-L" + lib_dir,
                           "-lmcarray_hip", "-Wl,-rpath," + lib_dir], timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
