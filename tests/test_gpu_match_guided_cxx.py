"""sift_cuda::matchListGuided / matchGuided on the GPU: tests/cpp/test_match_guided.cpp, built against libsift_cuda.so
the way tests/test_gpu_match_list_cxx.py builds its program (a host-only g++ compile), matches two uploaded sets inside
a window and compares both results with a brute force over the gate done in the program; a bad gate throws."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_match_guided(tmp_path):
    exe = tmp_path / "test_match_guided"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_match_guided.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match guided ok" in r.stdout
