"""sift_cuda::matchListEpipolar / matchEpipolar on the GPU: tests/cpp/test_match_epipolar.cpp, built against
libsift_cuda.so the way tests/test_gpu_match_guided_cxx.py builds its program (a host-only g++ compile, here with
-ffp-contract=off: the program's brute force is the float32 rule of include/sift_hip.h), matches two uploaded sets under
a fundamental matrix and compares both results with that brute force; a bad gate throws."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_match_epipolar(tmp_path):
    exe = tmp_path / "test_match_epipolar"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-pthread", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_match_epipolar.cpp"), "-o",
                    str(exe), "-L", LIB, "-lsift_cuda", "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match epipolar ok" in r.stdout
