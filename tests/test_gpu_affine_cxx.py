"""sift_cuda::verifyAffine / Verifier::verifyAffine* / refineAffine* on the GPU: tests/cpp/test_affine.cpp, built
against libsift_cuda.so the way tests/test_gpu_homography_cxx.py builds its program (a host-only g++ compile), runs the
main case of tests/affine_cases.py for either model with two refit rounds.  What its device forms left goes through
tests/test_gpu_affine.py's checker against the numpy mirror (sift_amd.cv.ransac_affine / refine_affine); the program
itself holds the host, one-shot and batched forms to the device forms, and checks that what the ABI refuses throws."""
import os
import subprocess

import numpy as np
import pytest

import affine_cases as ac
from test_gpu_affine import FILL, check_record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
ROUNDS = 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("affine_cxx") / "test_affine"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_affine.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    return exe


@pytest.mark.parametrize("similarity", ac.MODELS, ids=ac.MODEL_IDS)
def test_cxx_affine(sift, program, tmp_path, similarity):
    n_in, n_out, K = ac.MAIN
    m, q_xy, t_xy, _ = ac.case(n_in, n_out, similarity)
    for name, a in (("matches", m), ("q_xy", q_xy), ("t_xy", t_xy)):
        np.ascontiguousarray(a).tofile(tmp_path / (name + ".bin"))
    r = subprocess.run([str(program), str(tmp_path), str(int(similarity)), str(K), str(ROUNDS)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "affine ok" in r.stdout
    read = lambda name, dtype: np.fromfile(tmp_path / (name + ".bin"), dtype)  # noqa: E731
    verify, refine = ac.reference(n_in, n_out, K, similarity), ac.refined(n_in, n_out, K, similarity, 0, ROUNDS)
    for stage, ref in (("verify", verify), ("refine", refine)):
        got = dict(result=read(stage + "_result", sift.AFFINE_RESULT_DTYPE)[0], out=read(stage + "_out", sift.DMATCH_DTYPE),
                   out_count=int(read(stage + "_count", np.int32)[0]), mask=read(stage + "_mask", np.uint8))
        assert len(got["out"]) == len(m) == len(got["mask"])
        check_record(got, ref, len(m), m)
    assert int(read("refine_accepted", np.int32)[0]) == refine["accepted"] >= 1
    one = read("oneshot", sift.AFFINE_RESULT_DTYPE)[0]
    assert one["H"].tobytes() == refine["H"].tobytes() and one["hypothesis"] == refine["hypothesis"]
    assert read("oneshot_list", sift.DMATCH_DTYPE).tobytes() == refine["list"].tobytes()
    assert FILL == 0x5A  # the byte the program prefills its outputs with
