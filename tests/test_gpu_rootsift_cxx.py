"""sift_cuda::Detector::setRootSift and sift_cuda::rootSiftDevice / rootSiftHost on the GPU: tests/cpp/test_rootsift.cpp,
built against libsift_cuda.so the way tests/test_gpu_mask_cxx.py builds its program (a host-only g++ compile).  A root
detector's rows equal rootSiftDevice applied to a plain detector's copied rows on a 256 x 256 synthetic frame, and the
setter throws after the warm-up."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_rootsift(tmp_path):
    exe = tmp_path / "test_rootsift"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_rootsift.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rootsift ok" in r.stdout


def test_example_rootsift_flag():
    """extract_and_match_example --rootsift: the same frames and keypoint counts as the default run, matches that
    agree with the shift (exit status 0), through the synchronous and the pipelined loop alike."""
    tool = os.path.join(LIB, "extract_and_match_example")
    plain = subprocess.run([tool, "--frames", "3"], capture_output=True, text=True, timeout=120)
    root = subprocess.run([tool, "--frames", "3", "--rootsift"], capture_output=True, text=True, timeout=120)
    piped = subprocess.run([tool, "--frames", "3", "--rootsift", "--pipelined"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and root.returncode == 0 and piped.returncode == 0, root.stdout + root.stderr + piped.stderr
    kpts = lambda out: [line.split(",")[0] for line in out.splitlines() if line.startswith("frame")]  # noqa: E731  "frame f: n kpts"
    assert kpts(root.stdout) == kpts(plain.stdout) and len(kpts(root.stdout)) == 3
    assert piped.stdout == root.stdout
