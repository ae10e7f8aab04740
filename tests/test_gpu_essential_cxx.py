"""sift_cuda::verifyEssential / Verifier::verifyEssential* on the GPU: tests/cpp/test_essential.cpp, built against
libsift_cuda.so the way tests/test_gpu_affine_cxx.py builds its program (a host-only g++ compile), runs the 300 + 60 list
of tests/essential_cases.py.  What its device form left goes through tests/test_gpu_essential.py's checker against the
numpy mirror (sift_amd.cv.ransac_essential), and the pose it chained behind it against sift_amd.cv.recover_pose; the
program itself holds the host, one-shot and batched forms to the device form, and checks that what the ABI refuses
throws."""
import os
import subprocess

import numpy as np
import pytest

import essential_cases as ec
import pose_cases as pc
from test_gpu_essential import FILL, check_record, mirror

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
K = 64


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("essential_cxx") / "test_essential"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_essential.cpp"), "-o", str(exe), "-L", LIB, "-lsift_cuda",
                    "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    return exe


def test_cxx_essential(sift, program, tmp_path):
    from sift_amd import cv

    s = ec.scene(ec.GPU_SEED)
    m = s["matches"]
    for name, a in (("matches", m), ("q_xy", s["q_xy"]), ("t_xy", s["t_xy"]), ("cams", np.stack([s["cam_q"], s["cam_t"]]))):
        np.ascontiguousarray(a).tofile(tmp_path / (name + ".bin"))
    r = subprocess.run([str(program), str(tmp_path), str(K)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "essential ok" in r.stdout
    read = lambda name, dtype: np.fromfile(tmp_path / (name + ".bin"), dtype)  # noqa: E731
    ref = mirror(ec.PLANTED, ec.UNRELATED, K)
    got = dict(result=read("verify_result", sift.VERIFY_RESULT_DTYPE)[0], out=read("verify_out", sift.DMATCH_DTYPE),
               out_count=int(read("verify_count", np.int32)[0]), mask=read("verify_mask", np.uint8))
    assert len(got["out"]) == len(m) == len(got["mask"])
    check_record(got, ref, m)
    want = cv.recover_pose(m, s["q_xy"], s["t_xy"], ref, ref["mask"], s["cam_q"], s["cam_t"])
    assert read("pose", np.uint8).tobytes() == pc.pose_bytes(want) and want["candidate"] >= 0
    assert FILL == 0x5A  # the byte the program prefills its outputs with
