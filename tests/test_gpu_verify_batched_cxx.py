"""sift_cuda::Verifier's batched forms on the GPU: tests/cpp/test_verify_batched.cpp, built against libsift_cuda.so
the way tests/test_gpu_verify_cxx.py builds its program.  This test writes tests/verify_batched_cases.py's MIXED batch
of both models to a file, and per model the expected bytes -- every pair's model, winner and inlier records by the numpy
rule with the seed + p --; the program uploads the batch, runs verifyBatchedHost / verifyHomographyBatchedHost (and the
device forms) and compares byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import verify_batched_cases as bc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")


def batch_bytes(model, batch):
    K, seed = bc.BATCHES[batch]
    pairs = bc.pairs(model, batch)
    out = [struct.pack("<iiIf", len(pairs), K, seed, bc.MAX_ERROR)]
    for p in pairs:
        empty = len(p["buf"]) == 0  # an empty pair carries no position rows
        out.append(struct.pack("<iiii", len(p["buf"]), p["count"], 0 if empty else len(p["q_xy"]),
                               0 if empty else len(p["t_xy"])))
    out.append(bc.matches(model, batch).tobytes())
    for p in pairs:
        if len(p["buf"]):
            out += [np.ascontiguousarray(p["q_xy"], np.float32).tobytes(), np.ascontiguousarray(p["t_xy"], np.float32).tobytes()]
    return b"".join(out)


def expected_bytes(model, batch):
    out = []
    for p in range(len(bc.pairs(model, batch))):
        ref = bc.reference(model, batch, p)
        out += [bc.model_of(model, ref).astype(np.float32).tobytes(), struct.pack("<ii", ref["hypothesis"], ref["inliers"]),
                ref["list"].tobytes()]
    return b"".join(out)


def test_cxx_verify_batched(tmp_path):
    exe = tmp_path / "test_verify_batched"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_verify_batched.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    (tmp_path / "batch.bin").write_bytes(b"".join(batch_bytes(m, "MIXED") for m in bc.MODELS))
    for m in bc.MODELS:
        (tmp_path / f"{m}.bin").write_bytes(expected_bytes(m, "MIXED"))
    r = subprocess.run([str(exe), str(tmp_path / "batch.bin")] + [str(tmp_path / f"{m}.bin") for m in bc.MODELS],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify batched ok: 5 + 5 pairs" in r.stdout
