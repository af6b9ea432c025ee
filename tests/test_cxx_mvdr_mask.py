"""Builds and runs the C++ test of mca::MvdrBeamformer::framesCompletedBy and the updateMask argument of both process() overloads
(tests/cxx/test_mvdr_mask.cpp): a mask of ones is the run without one, a mask of 0.5 is setUpdateWeight(0.5) and overrides another
weight, closed bins keep their covariance."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cxx_update_mask_on_gpu(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_mvdr_mask"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_mvdr_mask.cpp"), "-o", str(exe), "-L" + lib_dir,
                           "-lmcarray_hip", "-Wl,-rpath," + lib_dir], timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
