"""sift_cuda::Detector::detectAndCompute(image, mask) on the GPU: tests/cpp/test_mask.cpp, built against
libsift_cuda.so the way tests/test_gpu_compute_cxx.py builds test_compute.cpp (a host-only g++ compile), runs the two
host overloads and the device overload on a 256 x 256 synthetic frame against the unmasked result filtered in C++, and
checks that a mask of the wrong size throws."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_masked_detect(tmp_path):
    exe = tmp_path / "test_mask"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_mask.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mask ok" in r.stdout
