"""sift_cuda::matchKnn / matchKnnList on the GPU: tests/cpp/test_match_knn.cpp, built against libsift_cuda.so the way
tests/test_gpu_match_list_cxx.py builds test_match_list.cpp (a host-only g++ compile), matches two 256 x 256 frames and
compares the rows and the capped list with the k-NN rule computed in C++ from the descriptor rows read back."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_match_knn(tmp_path):
    exe = tmp_path / "test_match_knn"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_match_knn.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match knn ok" in r.stdout
