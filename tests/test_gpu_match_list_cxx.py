"""sift_cuda::matchList on the GPU: tests/cpp/test_match_list.cpp, built against libsift_cuda.so the way
tests/test_gpu_mask_cxx.py builds test_mask.cpp (a host-only g++ compile), matches two 256 x 256 frames with the cross
check and compares the list with the mutual test done in C++ on the C ABI's top-2 of both directions."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_match_list(tmp_path):
    exe = tmp_path / "test_match_list"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_match_list.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match list ok" in r.stdout
