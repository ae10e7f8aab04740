"""Descriptors for caller-supplied keypoints (sift_hip_compute*, cv::Feature2D::compute):
what runs without a GPU.

* sift_hip_check_keypoints is host logic on a created, not warmed-up handle:
  the validity rules of include/sift_hip.h, one rejection per rule with the
  index of the offending keypoint.
* The Python / C++ surfaces exist and agree on the 24-byte keypoint record.
* Without a device, compute fails loudly (no CPU fallback).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
W, H, L = 96, 80, 3


def handle(sift, upscale):
    det = sift.Detector(sift.CudaSiftConfig(col_width=W, row_width=H, upscale=upscale, numFeatures=0))
    first = -1 if upscale else 0
    return det, first, first + det.nOctaves - 1


def kpt(sift, octave=0, layer=1, x=40.0, y=30.0, size=4.0, angle=10.0):
    k = np.zeros(1, sift.KPT_DTYPE)
    k["x"], k["y"], k["size"], k["angle"], k["response"] = x, y, size, angle, 0.05
    k["octave"] = (octave & 255) | (layer << 8) | (128 << 16)
    return k


@pytest.mark.parametrize("upscale", [False, True])
def test_check_keypoints_accepts_every_plane(sift, upscale):
    det, lo, hi = handle(sift, upscale)
    assert (lo, hi) == ((-1, 4) if upscale else (0, 3))
    good = np.concatenate([kpt(sift, o, layer) for o in range(lo, hi + 1) for layer in range(L + 3)]
                          + [kpt(sift, angle=0.0), kpt(sift, angle=360.0), kpt(sift, x=-2.0, y=-2.0)])
    assert det.check_keypoints(good) == -1
    assert det.check_keypoints(np.zeros(0, sift.KPT_DTYPE)) == -1


REJECTED = {
    "octave below the first": lambda s, lo, hi: kpt(s, octave=lo - 1),
    "octave above the last": lambda s, lo, hi: kpt(s, octave=hi + 1),
    "layer L+3": lambda s, lo, hi: kpt(s, layer=L + 3),
    "size 0": lambda s, lo, hi: kpt(s, size=0.0),
    "negative size": lambda s, lo, hi: kpt(s, size=-1.0),
    "NaN size": lambda s, lo, hi: kpt(s, size=np.nan),
    "infinite x": lambda s, lo, hi: kpt(s, x=np.inf),
    "angle -1": lambda s, lo, hi: kpt(s, angle=-1.0),
    "angle 360.5": lambda s, lo, hi: kpt(s, angle=360.5),
    "x = 2W+1": lambda s, lo, hi: kpt(s, x=2.0 * W + 1),
}


@pytest.mark.parametrize("upscale", [False, True])
@pytest.mark.parametrize("case", sorted(REJECTED))
def test_check_keypoints_rejects_with_index(sift, upscale, case):
    det, lo, hi = handle(sift, upscale)
    bad = REJECTED[case](sift, lo, hi)
    for pos in (0, 3, 6):  # first, middle, last of seven
        ks = np.concatenate([kpt(sift, x=10.0 + i) for i in range(7)])
        ks[pos] = bad[0]
        assert det.check_keypoints(ks) == pos, (case, pos)
    two = np.concatenate([kpt(sift), bad, kpt(sift), bad])
    assert det.check_keypoints(two) == 1  # the first bad one


@pytest.mark.parametrize("upscale", [False, True])
def test_check_keypoints_count_above_capacity(sift, upscale):
    det, _, _ = handle(sift, upscale)
    cap = det.capacities()["results"]
    ks = np.repeat(kpt(sift), cap + 1)
    assert det.check_keypoints(ks[:cap]) == -1
    with pytest.raises(sift.SiftHipError, match="capacity"):
        det.check_keypoints(ks)
    fb = ctypes.c_int(7)
    L_ = sift.lib()
    assert L_.sift_hip_check_keypoints(det.handle, ks.ctypes.data, cap + 1, ctypes.byref(fb)) == -1  # SIFT_HIP_ERR_INVALID
    assert L_.sift_hip_check_keypoints(det.handle, ks.ctypes.data, -1, ctypes.byref(fb)) == -1
    assert L_.sift_hip_check_keypoints(None, ks.ctypes.data, 1, ctypes.byref(fb)) == -1


def test_keypoint_record_layout_and_round_trip(sift, oracle):
    from sift_amd import cv

    assert sift.KPT_DTYPE.itemsize == 24
    assert sift.KPT_DTYPE == oracle.KPT_DTYPE
    assert [(n, sift.KPT_DTYPE.fields[n][1]) for n in sift.KPT_DTYPE.names] == \
        [(n, oracle.KPT_DTYPE.fields[n][1]) for n in oracle.KPT_DTYPE.names]
    ks = np.load(os.path.join(ROOT, "tests", "golden", "camera256.npz"))["default_kpts"]
    # a detector's host results of these keypoints: kpts3 {x, y, layer}, feats4 {(float)octave, size, response, angle}
    k3 = np.stack([ks["x"], ks["y"], ((ks["octave"] >> 8) & 255).astype(np.float32)], 1)
    f4 = np.stack([ks["octave"].astype(np.float32), ks["size"], ks["response"], ks["angle"]], 1)
    back = cv.keypoint_records(cv.keypoint_fields(k3, f4))
    assert back.dtype == sift.KPT_DTYPE and back.tobytes() == ks.astype(sift.KPT_DTYPE).tobytes()
    assert cv.keypoint_records(k3, f4).tobytes() == back.tobytes()
    assert callable(cv.from_cv_keypoints)


def test_surfaces_exist(sift):
    for name in ("compute", "computeDevice", "check_keypoints"):
        assert callable(getattr(sift.Detector, name))
    assert sift.SIFT_HIP_FLAG_BAD_KEYPOINT == 16
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::Detector::compute(" in out and "sift_cuda::Detector::computeDevice(" in out
    assert "abi=1" in sift.version()


def test_compute_without_gpu_fails_loudly(sift):
    n = ctypes.c_int(-1)
    rc = sift.lib().sift_hip_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible")
    det = sift.Detector(sift.CudaSiftConfig(col_width=64, row_width=64))
    with pytest.raises(sift.SiftHipError):
        det.compute(np.zeros((64, 64), np.float32), kpt(sift, x=20.0, y=20.0))


def test_compute_before_warmup_is_a_state_error(sift):
    """The C entry points refuse a handle that was never warmed up, before any device call."""
    det = sift.Detector(sift.CudaSiftConfig(col_width=64, row_width=64))
    k = kpt(sift, x=20.0, y=20.0)
    img = np.zeros((64, 64), np.float32)
    assert sift.lib().sift_hip_compute(det.handle, img.ctypes.data, 0, k.ctypes.data, 1) == -3  # SIFT_HIP_ERR_STATE
