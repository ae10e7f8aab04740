"""The gated k-NN C++ surface on the GPU: tests/cpp/test_match_knn_gated.cpp, built against libsift_cuda.so the way
tests/test_gpu_match_knn_cxx.py builds test_match_knn.cpp (a host-only g++ compile), run on arrays written here -- two
pairs of the shared case set with their positions, and what sift_amd.cv.guided_knn / epipolar_knn / knn_records expect
for the single-pair calls (pair 0) and the batched ones (both pairs)."""
import os
import subprocess

import numpy as np
import pytest

import knn_cases as kc
import knn_gated_cases as kg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
K = 5


def write_case(sift, d):
    from sift_amd import cv

    shapes = [kc.BIG, (70, 300)]
    tabs = {g: [] for g in kg.GATES}
    for p, (nq, nt) in enumerate(shapes):
        q, t = kc.sets(nq, nt)
        q_xy, t_xy = kg.positions(nq, nt)
        q.astype(np.float16).view(np.uint16).tofile(d / f"q{p}.bin")
        t.astype(np.float16).view(np.uint16).tofile(d / f"t{p}.bin")
        kg.with_stride(q_xy, 3).tofile(d / f"qxy{p}.bin")
        kg.with_stride(t_xy, 3).tofile(d / f"txy{p}.bin")
        for g in kg.GATES:
            tabs[g].append(kg.reference(g, nq, nt, K))
    cap = float(np.median(np.sqrt(tabs["window"][0][1][tabs["window"][0][0] >= 0])))
    np.float32([*shapes[0], *shapes[1], K, kg.RADIUS, kg.MAX_ERROR, cap, *kg.F.reshape(-1)]).tofile(d / "meta.bin")
    for g in kg.GATES:
        np.concatenate([x[0] for x in tabs[g]]).tofile(d / f"idx_{g}.bin")
        np.concatenate([x[1] for x in tabs[g]]).tofile(d / f"d2_{g}.bin")
        cv.knn_records(*tabs[g][0]).tofile(d / f"rows_{g}0.bin")
        lst = cv.knn_records(*tabs[g][0], max_distance=cap)
        assert 0 < len(lst) < (tabs[g][0][0] >= 0).sum()
        lst.tofile(d / f"list_{g}0.bin")
        cv.knn_records(*tabs[g][1], max_distance=cap, img_idx=1).tofile(d / f"blist_{g}1.bin")


def test_cxx_match_knn_gated(sift, tmp_path):
    write_case(sift, tmp_path)
    exe = tmp_path / "test_match_knn_gated"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_match_knn_gated.cpp"), "-o", str(exe), "-L", LIB,
                    "-lsift_cuda", "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match knn gated ok" in r.stdout
