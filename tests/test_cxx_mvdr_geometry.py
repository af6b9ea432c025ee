"""Builds the C++ test of mca::MvdrBeamformer::setGeometry / getGeometry (tests/cxx/test_mvdr_geometry.cpp) against the header, and runs
it on the GPU: the round trip, a planar-array process() call equal to the C ABI's bytes, the refusals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "test_mvdr_geometry.cpp")


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    return cxx


def test_cxx_program_compiles_against_the_header(tmp_path):
    """plain C++11 with every warning: the declarations and the default argument"""
    subprocess.check_call([_cxx(), "-std=c++11", "-O0", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", SRC,
                           "-o", str(tmp_path / "test_mvdr_geometry.o")], timeout=300)


@pytest.mark.gpu
def test_cxx_geometry_on_gpu(tmp_path):
    exe = tmp_path / "test_mvdr_geometry"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([_cxx(), "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), SRC, "-o", str(exe), "-L" + lib_dir,
                           "-lmcarray_hip", "-Wl,-rpath," + lib_dir], timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
