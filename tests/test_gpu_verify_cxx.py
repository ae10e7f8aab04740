"""sift_cuda::verifyFundamental / Verifier on the GPU: tests/cpp/test_verify.cpp, built against libsift_cuda.so the way
tests/test_gpu_match_epipolar_cxx.py builds its program (a host-only g++ compile with -ffp-contract=off: the program's
reference is the float32 rule of include/sift_hip.h restated in tests/cpp/verify_rule.hh), verifies an uploaded match
list and compares F, the winner and the inlier records with that restatement byte for byte; a bad max_error throws."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_verify(tmp_path):
    exe = tmp_path / "test_verify"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-pthread", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_verify.cpp"), "-o",
                    str(exe), "-L", LIB, "-lsift_cuda", "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify ok" in r.stdout
