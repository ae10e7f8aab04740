"""sift_cuda::matchListGuidedBatchedDevice / matchListEpipolarBatchedDevice / projectHomographyBatchedDevice on the GPU:
tests/cpp/test_match_guided_batched.cpp, built against libsift_cuda.so the way tests/test_gpu_verify_batched_cxx.py
builds its program.  This test writes two pairs of tests/guided_batched_cases.py's epipolar batch (two query blocks with
two splits, and the 33 x 31 pair) and a degenerate one to a file, and per gate the expected records by the numpy rule;
the program runs the C++ surface, the C ABI on a second matcher, and compares all three byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import epipolar_cases as ec
import guided_batched_cases as bc
import guided_cases as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
PICK = (4, 3, 9)  # 257 x 300, 33 x 31, and the pair whose record is all zero


def batch_bytes(pairs):
    out = [struct.pack("<iff", len(pairs), gc.RADIUS, ec.MAX_ERROR)]
    out += [struct.pack("<ii", len(p["q"]), len(p["t"])) for p in pairs]
    for p in pairs:
        out += [p["q"].astype(np.float16).tobytes(), p["t"].astype(np.float16).tobytes(),
                np.ascontiguousarray(p["q_xy"], np.float32).tobytes(), np.ascontiguousarray(p["t_xy"], np.float32).tobytes(),
                np.ascontiguousarray(p["F"], np.float32).tobytes()]
    return b"".join(out)


def expected_bytes(pairs, window):
    from sift_amd import cv

    out = []
    for i, p in enumerate(pairs):
        if window:
            fwd = cv.guided_top2(p["q"], p["t"], p["q_xy"], p["t_xy"], gc.RADIUS)
            rev = cv.guided_top2(p["t"], p["q"], p["t_xy"], p["q_xy"], gc.RADIUS)
        else:
            fwd, rev = p["fwd"], p["rev"]
        rec = cv.filter_matches(*fwd, *rev, img_idx=i)
        out += [struct.pack("<i", len(rec)), rec.tobytes()]
    return b"".join(out)


def test_cxx_match_guided_batched(tmp_path):
    exe = tmp_path / "test_match_guided_batched"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_match_guided_batched.cpp"), "-o", str(exe), "-L", LIB,
                    "-lsift_cuda", "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    pairs = [bc.epipolar_batch()[p] for p in PICK]
    assert not pairs[2]["usable"] and len(expected_bytes(pairs, False)) > 200
    (tmp_path / "batch.bin").write_bytes(batch_bytes(pairs))
    (tmp_path / "window.bin").write_bytes(expected_bytes(pairs, True))
    (tmp_path / "epipolar.bin").write_bytes(expected_bytes(pairs, False))
    r = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("batch.bin", "window.bin", "epipolar.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "guided batched ok: 3 pairs" in r.stdout
