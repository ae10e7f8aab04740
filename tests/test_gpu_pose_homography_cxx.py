"""sift_cuda::Verifier's plane pose forms and sift_cuda::recoverPoseHomography on the GPU:
tests/cpp/test_pose_homography.cpp, built against libsift_cuda.so the way tests/test_gpu_pose_cxx.py builds its program.
This test writes three scenes of tests/plane_pose_cases.py to a file -- a unique one with unrelated records marked, a
tied one, and one with an empty record --, and per scene the bytes the Python surface returns for it, which
tests/test_gpu_pose_homography.py holds to the numpy rule: the plane pose record, the four candidates, the in-front
mask, the points, and the in-front records.  The program runs recoverPoseHomographyHost, recoverPoseHomography,
recoverPoseHomographyDevice on device memory with mask_out on the mask, and the batched host form on the 3-pair batch,
and compares byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import plane_pose_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
SCENES = ((pc.UNIQUE_SEEDS[0], 300, 60, True), (pc.TIED_SEEDS[0], 300, 0, False), (pc.UNIQUE_SEEDS[2], 64, 1, False))


def python_bytes(sift, i, key):
    """(the program's input, the bytes Verifier.recover_pose_homography_host returns) for a scene; the last one's record
    is empty."""
    s = pc.scene(*key)
    m, q_xy, t_xy = s["matches"], s["q_xy"], s["t_xy"]
    dev = lambda a: sift.DeviceArray.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    dm, dq, dt = dev(m), dev(q_xy), dev(t_xy)
    rec = np.zeros(1, sift.HOMOGRAPHY_RESULT_DTYPE)
    rec["H"][0], rec["hypothesis"][0], rec["matches"][0] = s["H"], (-1 if i == len(SCENES) - 1 else 0), len(m)
    v = sift.Verifier(len(m), 1)
    pose, mask, points, recs, cands = v.recover_pose_homography_host(dm.value, 0, len(m), dq.value, len(q_xy), dt.value,
                                                                     len(t_xy), rec[0], s["mask"], s["cam_q"], s["cam_t"],
                                                                     q_stride=2, t_stride=2)
    ref = pc.reference(*key)
    if rec["hypothesis"][0] >= 0:
        assert pose.tobytes() == pc.plane_pose_bytes(ref) and ref["candidate"] >= 0
        assert cands.tobytes() == ref["candidates"].tobytes()
    else:
        assert pose["candidate"] == -1 and pose["fit"] == ref["fit"] and not mask.any()
        assert not cands.view(np.uint8).any()
    given = struct.pack("<iii", len(m), len(q_xy), len(t_xy)) + m.tobytes() + q_xy.tobytes() + t_xy.tobytes() + \
        rec.tobytes() + s["mask"].tobytes() + s["cam_q"].tobytes() + s["cam_t"].tobytes()
    want = pose.tobytes() + cands.tobytes() + mask.tobytes() + points.tobytes() + struct.pack("<i", len(recs)) + \
        recs.tobytes()
    return given, want


def test_cxx_pose_homography(sift, tmp_path):
    exe = tmp_path / "test_pose_homography"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_pose_homography.cpp"), "-o", str(exe), "-L", LIB,
                    "-lsift_cuda", "-lsift_hip", f"-Wl,-rpath,{LIB}"], check=True)
    given, want = struct.pack("<i", len(SCENES)), b""
    for i, key in enumerate(SCENES):
        g, w = python_bytes(sift, i, key)
        given += g
        want += w
    (tmp_path / "input.bin").write_bytes(given)
    (tmp_path / "want.bin").write_bytes(want)
    r = subprocess.run([str(exe), str(tmp_path / "input.bin"), str(tmp_path / "want.bin")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pose homography cxx ok" in r.stdout
