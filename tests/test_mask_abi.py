"""Detection mask (sift_hip_detect_masked*, cv::SIFT's mask argument): what runs without a GPU.

* The three entry points are exported with the signatures include/sift_hip.h documents.
* sift_amd.cv.mask_keep is KeyPointsFilter::runByPixelsMask in float32: (int)(v + 0.5f).
* The Python surface checks a mask's dtype and shape before any device call.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")

SIGNATURES = """
#include "sift_hip.h"
int (*a)(sift_hip_t, const void*, size_t, int, const uint8_t*, size_t) = sift_hip_detect_masked;
int (*b)(sift_hip_t, const void*, size_t, int, const uint8_t*, size_t, void*) = sift_hip_detect_device_masked;
int (*c)(sift_hip_t, const void*, int, size_t, size_t, int, const uint8_t*, size_t, size_t, void*) =
    sift_hip_detect_batch_device_masked;
"""
NAMES = ("sift_hip_detect_masked", "sift_hip_detect_device_masked", "sift_hip_detect_batch_device_masked")


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in NAMES:
        assert name in exported, name
        assert getattr(sift.lib(), name).argtypes is not None
    src = tmp_path / "signatures.c"
    src.write_text(SIGNATURES)
    # a C compile of the header: a function pointer of another type is an error
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    L = sift.lib()
    assert len(L.sift_hip_detect_masked.argtypes) == 6
    assert len(L.sift_hip_detect_device_masked.argtypes) == 7
    assert len(L.sift_hip_detect_batch_device_masked.argtypes) == 10


def test_surfaces_exist(sift):
    import inspect

    from sift_amd import cv

    assert callable(cv.mask_keep)
    assert "mask" in inspect.signature(sift.Detector.detectAndCompute).parameters
    p = inspect.signature(sift.Detector.detectAndComputeDevice).parameters
    assert "mask_ptr" in p and "mask_stride" in p
    p = inspect.signature(sift.Detector.detectBatchDevice).parameters
    assert "masks_ptr" in p and "mask_stride" in p and "mask_frame_stride" in p
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::Detector::detectAndCompute(Image<float> const&, Image<unsigned char> const&)" in out
    assert "sift_cuda::Detector::detectAndCompute(Image<unsigned char> const&, Image<unsigned char> const&)" in out
    assert "sift_cuda::Detector::detectAndComputeDevice(void const*, unsigned long, bool, unsigned char const*" in out


def test_mask_keep_rounds_like_opencv():
    from sift_amd import cv

    mask = np.zeros((4, 6), np.uint8)
    mask[1, 3] = 255
    below = np.nextafter(np.float32(2.5), np.float32(0))
    assert below < np.float32(2.5)
    # x = 2.5 lands in column 3; the float just below it in column 2
    assert cv.mask_keep([2.5], [1.0], mask).tolist() == [True]
    assert cv.mask_keep([below], [1.0], mask).tolist() == [False]
    # the same rule for rows
    assert cv.mask_keep([3.0], [0.5], mask).tolist() == [True]
    # float32 add: (0.5 - 2^-25) + 0.5 rounds to 1.0f (row 1), where exact arithmetic would stay in row 0
    assert cv.mask_keep([3.0], [np.nextafter(np.float32(0.5), np.float32(0))], mask).tolist() == [True]
    assert cv.mask_keep([3.0], [0.25], mask).tolist() == [False]
    assert cv.mask_keep([3.0], [np.nextafter(np.float32(1.5), np.float32(0))], mask).tolist() == [True]
    assert cv.mask_keep([3.0], [1.5], mask).tolist() == [False]
    # float32 arithmetic: 2.5 - 2^-25 is 2.5 as a float (a float64 sum would land in column 2)
    assert cv.mask_keep(np.array([2.5 - 2.0 ** -25]), [1.0], mask).tolist() == [True]
    # a value of 1 keeps the keypoint; order and dtype of the answer
    mask[2, 0] = 1
    keep = cv.mask_keep(np.float32([0.2, 3.4, 5.0, 2.6]), np.float32([2.3, 1.49, 3.0, 0.6]), mask)
    assert keep.dtype == np.bool_ and keep.tolist() == [True, True, False, True]
    assert cv.mask_keep([], [], mask).shape == (0,)


def test_mask_keep_strided_view_and_argument_checks():
    from sift_amd import cv

    big = np.zeros((8, 12), np.uint8)
    big[2, 6] = 7
    big[2, 7] = 9  # outside the view below: a packed read of the view's memory would see it
    for view, (x, y) in ((big[:, :7], (6.0, 2.0)), (big[::2, ::2], (3.0, 1.0)), (big.T, (2.0, 6.0))):
        assert not view.flags["C_CONTIGUOUS"]
        assert cv.mask_keep([x, x - 1], [y, y], view).tolist() == [True, False]
    with pytest.raises(ValueError):
        cv.mask_keep([1.0], [1.0], np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        cv.mask_keep([1.0], [1.0], np.zeros(16, np.uint8))
    with pytest.raises(ValueError):
        cv.mask_keep([1.0, 2.0], [1.0], np.zeros((4, 4), np.uint8))


def test_python_mask_argument_checks_need_no_device(sift):
    """A bad mask is refused before the warm-up (the first device call)."""
    w, h = 64, 48
    det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h))
    img = np.zeros((h, w), np.float32)
    for bad, word in ((np.zeros((h, w), np.float32), "uint8"), (np.zeros((h, w), np.int8), "uint8"),
                      (np.zeros((h, w), bool), "uint8"), ([[0] * w] * h, "uint8"),
                      (np.zeros((w, h), np.uint8), "shape"), (np.zeros((h, w + 1), np.uint8), "shape"),
                      (np.zeros((h, w, 1), np.uint8), "shape"), (np.zeros(h * w, np.uint8), "shape")):
        with pytest.raises(sift.SiftHipError, match=word):
            det.detectAndCompute(img, bad)
    assert not det._ready
    # a strided view whose last axis is contiguous is passed as it is; other layouts are copied
    big = np.zeros((h, w + 5), np.uint8)
    assert det._host_mask(big[:, :w]).strides == (w + 5, 1)
    assert np.shares_memory(det._host_mask(big[:, :w]), big)
    t = np.zeros((w, h), np.uint8).T
    assert det._host_mask(t).strides == (w, 1)


def test_masked_call_before_warmup_is_a_state_error(sift):
    det = sift.Detector(sift.CudaSiftConfig(col_width=64, row_width=64))
    img, mask = np.zeros((64, 64), np.float32), np.zeros((64, 64), np.uint8)
    L = sift.lib()
    assert L.sift_hip_detect_masked(det.handle, img.ctypes.data, 0, 0, mask.ctypes.data, 0) == -3  # SIFT_HIP_ERR_STATE
    assert L.sift_hip_detect_device_masked(det.handle, img.ctypes.data, 0, 0, mask.ctypes.data, 0, None) == -3
    assert L.sift_hip_detect_masked(None, img.ctypes.data, 0, 0, mask.ctypes.data, 0) == -1  # SIFT_HIP_ERR_INVALID
