"""sift_cuda::verifyHomography / Verifier::verifyHomography* / projectHomographyDevice on the GPU:
tests/cpp/test_homography.cpp, built against libsift_cuda.so the way tests/test_gpu_verify_cxx.py builds its program (a
host-only g++ compile), verifies the main case of tests/homography_cases.py and compares H, the winner, the inlier
records and the projected positions byte for byte with what the numpy mirror (sift_amd.cv.ransac_homography,
cv.project_homography) makes of it, dumped here into the test's directory; what the ABI refuses throws."""
import os
import subprocess

import numpy as np
import pytest

import homography_cases as hc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def test_cxx_homography(sift, tmp_path):
    from sift_amd import cv

    n_in, n_out, K = hc.MAIN
    m, q_xy, t_xy, _ = hc.case(n_in, n_out)
    ref = hc.reference(n_in, n_out, K)
    assert K == 512 and ref["hypothesis"] >= 0  # the program's VerifyParams
    rec = np.zeros(1, sift.HOMOGRAPHY_RESULT_DTYPE)
    rec["H"], rec["inliers"], rec["hypothesis"] = ref["H"], ref["inliers"], ref["hypothesis"]
    rec["matches"], rec["valid_hypotheses"] = ref["matches"], ref["valid_hypotheses"]
    for name, a in (("matches", m), ("q_xy", q_xy), ("t_xy", t_xy), ("ref", rec), ("list", ref["list"]),
                    ("proj", cv.project_homography(ref["H"], q_xy))):
        np.ascontiguousarray(a).tofile(tmp_path / (name + ".bin"))
    exe = tmp_path / "test_homography"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_homography.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "homography ok" in r.stdout
