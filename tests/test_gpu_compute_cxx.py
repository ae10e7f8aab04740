"""sift_cuda::Detector::compute on the GPU: tests/cpp/test_compute.cpp, built
against libsift_cuda.so the way tests/test_multi_cxx.py builds test_multi.cpp
(a host-only g++ compile), hands a synthetic frame's own keypoints back through
compute() and compares bytes with detectAndCompute."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_compute_round_trip(tmp_path):
    exe = tmp_path / "test_compute"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_compute.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compute ok" in r.stdout
