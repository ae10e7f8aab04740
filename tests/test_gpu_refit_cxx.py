"""sift_cuda::Verifier's refit forms on the GPU: tests/cpp/test_refit.cpp, built against libsift_cuda.so the way
tests/test_gpu_verify_batched_cxx.py builds its program.  This test writes one list per model (tests/refit_cases.py's
MAIN shapes) to a file, and per model the bytes the Python surface returns for it -- which tests/test_gpu_refit.py holds
to the numpy rule --: the refined record, the accepted rounds, the inlier records and the mask.  The program runs
verifyFundamental / verifyHomography with refit rounds, verifyDevice -> refineDevice on device memory, and the host form,
and compares byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import refit_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
ROUNDS = 2


def python_bytes(sift, model):
    """(the program's input, the bytes Verifier.verify*_host -> refine*_host return) for the model's MAIN shape."""
    mod = rc.CASES[model]
    n_in, n_out, K = mod.MAIN
    m, q_xy, t_xy, _ = mod.case(n_in, n_out)
    dev = lambda a: sift.DeviceArray.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    dm, dq, dt = dev(m), dev(q_xy), dev(t_xy)
    v = sift.Verifier(len(m), K)
    args = (dm.value, 0, len(m), dq.value, len(q_xy), dt.value, len(t_xy))
    verify, refine = (v.verify_host, v.refine_host) if model == "fundamental" else \
        (v.verify_homography_host, v.refine_homography_host)
    r, _, mask = verify(*args, rc.MAX_ERROR, K, 0, 2, 2, True)
    r, recs, mask, accepted = refine(*args, r, mask, rc.MAX_ERROR, ROUNDS, 2, 2)
    ref = rc.refined(model, mod.MAIN, ROUNDS)
    assert r[rc.FIELD[model]].tobytes() == ref[rc.FIELD[model]].tobytes() and accepted == ref["accepted"]
    given = struct.pack("<iiiiif", len(m), len(q_xy), len(t_xy), K, ROUNDS, rc.MAX_ERROR) + m.tobytes() + \
        q_xy.tobytes() + t_xy.tobytes()
    want = r.tobytes() + struct.pack("<ii", accepted, len(recs)) + recs.tobytes() + mask.tobytes()
    return given, want


def test_cxx_refit(sift, tmp_path):
    exe = tmp_path / "test_refit"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_refit.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    given = b""
    for model in rc.MODELS:
        g, want = python_bytes(sift, model)
        given += g
        (tmp_path / f"{model}.bin").write_bytes(want)
    (tmp_path / "input.bin").write_bytes(given)
    r = subprocess.run([str(exe), str(tmp_path / "input.bin")] + [str(tmp_path / f"{m}.bin") for m in rc.MODELS],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refit cxx ok" in r.stdout
