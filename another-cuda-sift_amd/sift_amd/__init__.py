"""Python mirror of the reference's SIFT interface over libsift_hip.so (C ABI).

Names follow /root/reference/sift_cuda/interface/Detector.hh:24-96 and
/root/reference/sift_cuda/types/CudaSiftConfig.hh:3-14 (including the
reference's field spellings), so host code and parity tests read like the
reference's own callers (/root/reference/tool/*.cc).

The compute path is the HIP library only: if libsift_hip.so is missing this
module raises ImportError-like errors on first use; there is no CPU fallback.

HIP runtime note: PyTorch wheels bundle their own libamdhip64.so.  A process that
uses both torch and this library must load torch's runtime BEFORE
libsift_hip.so, so that the library binds to the already-loaded runtime (one HIP
runtime per process; the other order leaves torch with "No HIP GPUs are
available").  `lib()` therefore imports torch first whenever torch is
installed, so the load order no longer depends on the caller's imports.
"""
from __future__ import annotations

import ctypes
import importlib.util
import os
import sys
import warnings
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.normpath(os.path.join(_HERE, "..", "lib"))
# SIFT_HIP_LIB: alternative build of the same library (kernel A/B experiments).
LIB_PATH = os.environ.get("SIFT_HIP_LIB") or os.path.join(LIB_DIR, "libsift_hip.so")

SIFT_HIP_OK = 0
SIFT_HIP_F32, SIFT_HIP_U8 = 0, 1  # pixel formats (include/sift_hip.h)
SIFT_HIP_DESC_FAST, SIFT_HIP_DESC_EXACT = 0, 1  # descriptor modes (sift_hip_set_descriptor_mode)
SIFT_HIP_NORM_L2, SIFT_HIP_NORM_ROOT = 0, 1  # descriptor norms (sift_hip_set_descriptor_norm)
SIFT_HIP_FLAG_BAD_KEYPOINT = 16  # overflow_flags() bit: computeDevice met an invalid keypoint
# sift_hip_keypoint (cv::KeyPoint minus class_id, 24 bytes): the records Detector.compute takes.
# octave is OpenCV's packed form (octave & 255 | layer << 8 | xi << 16).
KPT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
# sift_hip_dmatch (cv::DMatch's fields in its order, 16 bytes): the records of Matcher.match_list_*.
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
KNN_MAX = 8  # SIFT_HIP_KNN_MAX: the largest k of Matcher.match_knn_*
_lib = None


class SiftHipError(RuntimeError):
    pass


class SiftCapacityWarning(RuntimeWarning):
    """A per-frame capacity (candidates, refined, oriented, results) overflowed; see overflow_flags()."""


class SiftKeypointWarning(RuntimeWarning):
    """computeDevice met an invalid keypoint (overflow_flags() bit 16): its descriptor row is zero."""


class _Config(ctypes.Structure):
    _fields_ = [
        ("col_width", ctypes.c_int),
        ("row_width", ctypes.c_int),
        ("numFeatures", ctypes.c_int),
        ("numOctaveLayers", ctypes.c_int),
        ("contrastThreshould", ctypes.c_double),
        ("edgeThreshould", ctypes.c_double),
        ("sigma", ctypes.c_double),
        ("upscale", ctypes.c_int),
        ("numOctaves", ctypes.c_int),
        ("maxKeypoints", ctypes.c_int),
    ]


class _MatchGate(ctypes.Structure):
    """sift_hip_match_gate: device position rows (x, y first) of both sets and the window's half-size in pixels."""
    _fields_ = [
        ("query_xy", ctypes.c_void_p),
        ("query_stride", ctypes.c_int),
        ("train_xy", ctypes.c_void_p),
        ("train_stride", ctypes.c_int),
        ("radius", ctypes.c_float),
    ]


class _MatchEpipolarGate(ctypes.Structure):
    """sift_hip_match_epipolar_gate: the positions as _MatchGate, the pair's fundamental matrix (row-major,
    x_train^T F x_query = 0) and the band's half-width (Sampson distance, pixels)."""
    _fields_ = [
        ("query_xy", ctypes.c_void_p),
        ("query_stride", ctypes.c_int),
        ("train_xy", ctypes.c_void_p),
        ("train_stride", ctypes.c_int),
        ("radius", ctypes.c_float),
        ("F", ctypes.c_float * 9),
        ("max_error", ctypes.c_float),
    ]


def _epipolar_gate(q_xy_ptr: int, q_stride: int, t_xy_ptr: int, t_stride: int, radius: float, F,
                   max_error: float) -> _MatchEpipolarGate:
    f = np.asarray(F, np.float32).reshape(-1)
    if f.size != 9:
        raise ValueError("F must have 9 entries (3 x 3, row-major)")
    return _MatchEpipolarGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius,
                              (ctypes.c_float * 9)(*f.tolist()), max_error)


class _MatchPositions(ctypes.Structure):
    """sift_hip_match_positions: pair p's device position rows in a batched gated call."""
    _fields_ = [("query_xy", ctypes.c_void_p), ("train_xy", ctypes.c_void_p)]


class _ProjectSet(ctypes.Structure):
    """sift_hip_project_set: one set of sift_hip_project_homography_batched_device."""
    _fields_ = [("xy", ctypes.c_void_p), ("n", ctypes.c_int), ("out_xy", ctypes.c_void_p)]


class _MatchFilter(ctypes.Structure):
    _fields_ = [
        ("ratio", ctypes.c_float),
        ("ratio_on_squared", ctypes.c_int),
        ("ratio_both_ways", ctypes.c_int),
        ("max_distance", ctypes.c_float),
        ("cross_check", ctypes.c_int),
    ]


def _match_filter(ratio: float = 0.8, ratio_on_squared: bool = False, ratio_both_ways: bool = False,
                  max_distance: float = 0.0, cross_check: bool = True) -> _MatchFilter:
    """sift_hip_match_filter with sift_hip_default_match_filter's defaults."""
    return _MatchFilter(ratio, int(bool(ratio_on_squared)), int(bool(ratio_both_ways)), max_distance,
                        int(bool(cross_check)))


class _VerifyParams(ctypes.Structure):
    """sift_hip_verify_params: the hypothesis budget K, the sampler's seed and the inlier threshold (Sampson distance,
    pixels)."""
    _fields_ = [
        ("hypotheses", ctypes.c_int),
        ("seed", ctypes.c_uint),
        ("max_error", ctypes.c_float),
    ]


class _VerifyResult(ctypes.Structure):
    """sift_hip_verify_result: the winning hypothesis' F (row-major), its inlier count and index (-1: none), the number
    of matches that counted and the number of hypotheses that were solved."""
    _fields_ = [
        ("F", ctypes.c_float * 9),
        ("inliers", ctypes.c_int),
        ("hypothesis", ctypes.c_int),
        ("matches", ctypes.c_int),
        ("valid_hypotheses", ctypes.c_int),
    ]


VERIFY_RESULT_DTYPE = np.dtype([("F", "<f4", (9,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("matches", "<i4"),
                                ("valid_hypotheses", "<i4")])
assert VERIFY_RESULT_DTYPE.itemsize == ctypes.sizeof(_VerifyResult)


class _VerifyPair(ctypes.Structure):
    """sift_hip_verify_pair: one pair of a batched verify call -- its device position rows and their counts, and cap,
    its number of rows in the call's matches, out and mask arrays (its rows start at the sum of the caps before it)."""
    _fields_ = [
        ("query_xy", ctypes.c_void_p),
        ("train_xy", ctypes.c_void_p),
        ("nq", ctypes.c_int),
        ("nt", ctypes.c_int),
        ("cap", ctypes.c_int),
    ]


assert ctypes.sizeof(_VerifyPair) == 32


class _HomographyResult(ctypes.Structure):
    """sift_hip_homography_result: the winning hypothesis' H (row-major, x_train ~ H x_query), its inlier count and
    index (-1: none), the number of matches that counted and the number of valid hypotheses."""
    _fields_ = [
        ("H", ctypes.c_float * 9),
        ("inliers", ctypes.c_int),
        ("hypothesis", ctypes.c_int),
        ("matches", ctypes.c_int),
        ("valid_hypotheses", ctypes.c_int),
    ]


HOMOGRAPHY_RESULT_DTYPE = np.dtype([("H", "<f4", (9,)), ("inliers", "<i4"), ("hypothesis", "<i4"), ("matches", "<i4"),
                                    ("valid_hypotheses", "<i4")])
assert HOMOGRAPHY_RESULT_DTYPE.itemsize == ctypes.sizeof(_HomographyResult)
# sift_hip_affine_result is the homography's record: H holds {a, b, tx, c, d, ty, 0, 0, 1}.
AFFINE_RESULT_DTYPE = HOMOGRAPHY_RESULT_DTYPE
MODEL_AFFINE, MODEL_SIMILARITY = 0, 1  # SIFT_HIP_MODEL_*


class _Camera(ctypes.Structure):
    """sift_hip_camera: a skew-free pinhole camera."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float)]


class _PoseParams(ctypes.Structure):
    """sift_hip_pose_params: the far bound on both depths, in baselines, and the cosine below which a record in front
    counts as one with parallax."""
    _fields_ = [("max_depth", ctypes.c_float), ("max_cos_parallax", ctypes.c_float)]


POSE_RESULT_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("in_front", "<i4"), ("with_parallax", "<i4"),
                              ("counts", "<i4", (4,)), ("candidate", "<i4"), ("fit", "<i4")])
assert POSE_RESULT_DTYPE.itemsize == 80
# sift_hip_plane_pose_result: a pose record as it lies, then the winner's plane; sift_hip_plane_candidate: one of the
# four (R, t, n, distance) of a homography's decomposition.
PLANE_POSE_RESULT_DTYPE = np.dtype(POSE_RESULT_DTYPE.descr + [("normal", "<f4", (3,)), ("distance", "<f4")])
PLANE_CANDIDATE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("normal", "<f4", (3,)), ("distance", "<f4")])
assert PLANE_POSE_RESULT_DTYPE.itemsize == 96 and PLANE_CANDIDATE_DTYPE.itemsize == 64


def _cameras(cams, P: int):
    """A ctypes array of P sift_hip_camera from (fx, fy, cx, cy) rows; None when there are none."""
    a = np.asarray(cams, np.float32).reshape(-1, 4)
    if len(a) != P:
        raise ValueError("one (fx, fy, cx, cy) camera per pair and side")
    return (_Camera * max(P, 1))(*[_Camera(*[float(x) for x in r]) for r in a])


def lib() -> ctypes.CDLL:
    """Load libsift_hip.so (once).  Fails loudly when the build is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SiftHipError(f"{LIB_PATH} not found: build it with `make` (or __graft_entry__.build())")
    # torch's bundled HIP runtime first (module docstring), so one HIP runtime
    # serves both; importing torch does not touch the GPU.  Only when torch is
    # installed, and a broken torch install (OSError / RuntimeError from its
    # bundled libraries) must not stop callers that never use torch.
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        try:
            import torch  # noqa: F401
        except Exception as e:  # noqa: BLE001
            print(f"sift_amd: torch import failed ({e!r}); loading {LIB_PATH} on its own", file=sys.stderr)
    L = ctypes.CDLL(LIB_PATH)
    vp, ip, i, f, d, sz = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    sigs = {
        "sift_hip_default_config": (None, [ctypes.POINTER(_Config), i, i]),
        "sift_hip_version": (ctypes.c_char_p, []),
        "sift_hip_last_error": (ctypes.c_char_p, []),
        "sift_hip_create": (i, [ctypes.POINTER(_Config), i, ctypes.POINTER(vp)]),
        "sift_hip_destroy": (i, [vp]),
        "sift_hip_warmup": (i, [vp]),
        "sift_hip_num_octaves": (i, [vp, ip]),
        "sift_hip_octave_dims": (i, [vp, i, ip, ip, ip]),
        "sift_hip_detect": (i, [vp, vp, sz]),
        "sift_hip_detect_device": (i, [vp, vp, sz, vp]),
        "sift_hip_detect_u8": (i, [vp, vp, sz]),
        "sift_hip_detect_device_fmt": (i, [vp, vp, sz, i, vp]),
        "sift_hip_detect_masked": (i, [vp, vp, sz, i, vp, sz]),
        "sift_hip_detect_device_masked": (i, [vp, vp, sz, i, vp, sz, vp]),
        "sift_hip_detect_batch_device_masked": (i, [vp, vp, i, sz, sz, i, vp, sz, sz, vp]),
        "sift_hip_check_keypoints": (i, [vp, vp, i, ip]),
        "sift_hip_compute": (i, [vp, vp, sz, vp, i]),
        "sift_hip_compute_u8": (i, [vp, vp, sz, vp, i]),
        "sift_hip_compute_device": (i, [vp, vp, sz, i, vp, i, vp]),
        "sift_hip_submit": (i, [vp, vp, sz, i, ctypes.POINTER(ctypes.c_longlong)]),
        "sift_hip_wait": (i, [vp, ctypes.c_longlong]),
        "sift_hip_submit_device": (i, [vp, vp, sz, i, vp, ctypes.POINTER(ctypes.c_longlong)]),
        "sift_hip_set_lanes": (i, [vp, i]),
        "sift_hip_lanes": (i, [vp, ip, ip]),
        "sift_hip_set_micro_batch": (i, [vp, i]),
        "sift_hip_micro_batch": (i, [vp, ip]),
        "sift_hip_set_auto_micro_batch": (i, [vp, i]),
        "sift_hip_auto_micro_batch": (i, [vp, ip]),
        "sift_hip_sync": (i, [vp]),
        "sift_hip_set_batch": (i, [vp, i]),
        "sift_hip_batch_capacity": (i, [vp, ip]),
        "sift_hip_set_descriptor_mode": (i, [vp, i]),
        "sift_hip_descriptor_mode": (i, [vp, ip]),
        "sift_hip_set_descriptor_norm": (i, [vp, i]),
        "sift_hip_descriptor_norm": (i, [vp, ip]),
        "sift_hip_rootsift_device": (i, [vp, i, vp, vp]),
        "sift_hip_rootsift_host": (i, [vp, i, vp]),
        "sift_hip_capacities": (i, [vp, ip, ip, ip, ip]),
        "sift_hip_detect_batch_device": (i, [vp, vp, i, sz, sz, i, vp]),
        "sift_hip_batch_frames": (i, [vp, ip]),
        "sift_hip_batch_results_device": (i, [vp, i, ip, ip, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]),
        "sift_hip_batch_copy_to_host": (i, [vp, i, vp, vp, vp, i, ip]),
        "sift_hip_num_keypoints": (i, [vp, ip]),
        "sift_hip_overflow_flags": (i, [vp, ip]),
        "sift_hip_results_device": (i, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ip, ip]),
        "sift_hip_copy_to_host": (i, [vp, vp, vp, vp, i]),
        "sift_hip_results_host": (i, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ip]),
        "sift_hip_copy_descriptors_device": (i, [vp, vp, i, vp]),
        "sift_hip_results_sidecar": (i, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]),
        "sift_hip_descriptors_written": (i, [vp]),
        "sift_hip_match_codes_batched": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, f, i, vp, vp, vp, vp]),
        "sift_hip_set_datagen": (i, [vp, ctypes.c_char_p]),
        "sift_hip_replay_stage": (i, [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]),
        "sift_hip_set_timing": (i, [vp, i]),
        "sift_hip_timing_count": (i, [vp, ip]),
        "sift_hip_timing_entry": (i, [vp, i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(d), ip, ctypes.POINTER(d)]),
        "sift_hip_timing_reset": (i, [vp]),
        "sift_hip_debug_gaussian": (i, [vp, i, i, vp]),
        "sift_hip_debug_candidates": (i, [vp, vp, i, ip]),
        "sift_hip_matcher_create": (i, [i, i, i, i, ctypes.POINTER(vp)]),
        "sift_hip_matcher_destroy": (i, [vp]),
        "sift_hip_matcher_set_sidecars": (i, [vp, i]),
        "sift_hip_match_device": (i, [vp, vp, i, vp, i, f, i, vp, vp, vp, vp]),
        "sift_hip_match_batched": (i, [vp, i, vp, vp, vp, vp, f, i, vp, vp, vp, vp]),
        "sift_hip_match_host": (i, [vp, vp, i, vp, i, f, i, vp]),
        "sift_hip_match_plan": (i, [i, i, i, ip, ip]),
        "sift_hip_default_match_filter": (None, [ctypes.POINTER(_MatchFilter)]),
        "sift_hip_match_list_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_list_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_list_codes_batched": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_MatchFilter),
                                                  vp, vp, vp]),
        "sift_hip_match_list_host": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchFilter), vp, i, ip]),
        "sift_hip_match_knn_device": (i, [vp, vp, i, vp, i, i, vp, vp, vp]),
        "sift_hip_match_knn_batched": (i, [vp, i, vp, vp, vp, vp, i, vp, vp, vp]),
        "sift_hip_match_knn_codes_batched": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp]),
        "sift_hip_match_knn_host": (i, [vp, vp, i, vp, i, i, vp, vp]),
        "sift_hip_match_knn_list_device": (i, [vp, vp, i, vp, i, i, f, vp, vp, vp]),
        "sift_hip_match_knn_list_batched": (i, [vp, i, vp, vp, vp, vp, i, f, vp, vp, vp]),
        "sift_hip_match_knn_list_host": (i, [vp, vp, i, vp, i, i, f, vp, i, ip]),
        "sift_hip_match_knn_plan": (i, [i, i, i, i, ip]),
        "sift_hip_match_guided_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchGate), f, i, vp, vp, vp, vp]),
        "sift_hip_match_guided_plan": (i, [i, i, ip]),
        "sift_hip_match_list_guided_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchGate),
                                                  ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_list_guided_host": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchGate),
                                                ctypes.POINTER(_MatchFilter), vp, i, ip]),
        "sift_hip_match_epipolar_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchEpipolarGate), f, i, vp, vp, vp,
                                               vp]),
        "sift_hip_match_list_epipolar_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchEpipolarGate),
                                                    ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_list_epipolar_host": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchEpipolarGate),
                                                  ctypes.POINTER(_MatchFilter), vp, i, ip]),
        "sift_hip_match_guided_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f, f, i, vp,
                                              vp, vp, vp]),
        "sift_hip_match_epipolar_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f, vp, i, f,
                                                f, i, vp, vp, vp, vp]),
        "sift_hip_match_list_guided_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f,
                                                   ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_list_epipolar_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f, vp,
                                                     i, f, ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_list_guided_codes_batched": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, vp,
                                                         ctypes.POINTER(_MatchPositions), i, i, f,
                                                         ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_list_epipolar_codes_batched": (i, [vp, vp, vp, i, vp, vp, vp, vp, vp, vp,
                                                           ctypes.POINTER(_MatchPositions), i, i, f, vp, i, f,
                                                           ctypes.POINTER(_MatchFilter), vp, vp, vp]),
        "sift_hip_match_knn_guided_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchGate), i, vp, vp, vp]),
        "sift_hip_match_knn_epipolar_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchEpipolarGate), i, vp, vp, vp]),
        "sift_hip_match_knn_guided_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f, i, vp,
                                                  vp, vp]),
        "sift_hip_match_knn_epipolar_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f, vp,
                                                    i, f, i, vp, vp, vp]),
        "sift_hip_match_knn_list_guided_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchGate), i, f, vp, vp, vp]),
        "sift_hip_match_knn_list_epipolar_device": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchEpipolarGate), i, f, vp,
                                                        vp, vp]),
        "sift_hip_match_knn_list_guided_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f,
                                                       i, f, vp, vp, vp]),
        "sift_hip_match_knn_list_epipolar_batched": (i, [vp, i, vp, vp, vp, vp, ctypes.POINTER(_MatchPositions), i, i, f,
                                                         vp, i, f, i, f, vp, vp, vp]),
        "sift_hip_match_knn_guided_host": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchGate), i, vp, vp]),
        "sift_hip_match_knn_epipolar_host": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchEpipolarGate), i, vp, vp]),
        "sift_hip_match_knn_list_guided_host": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchGate), i, f, vp, i, ip]),
        "sift_hip_match_knn_list_epipolar_host": (i, [vp, vp, i, vp, i, ctypes.POINTER(_MatchEpipolarGate), i, f, vp, i,
                                                      ip]),
        "sift_hip_project_homography_batched_device": (i, [vp, i, i, ctypes.POINTER(_ProjectSet), i, i, vp]),
        "sift_hip_default_verify_params": (None, [ctypes.POINTER(_VerifyParams)]),
        "sift_hip_verifier_create": (i, [i, i, i, ctypes.POINTER(vp)]),
        "sift_hip_verifier_destroy": (i, [vp]),
        "sift_hip_verify_fundamental_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, ctypes.POINTER(_VerifyParams), vp,
                                                   vp, vp, vp, vp]),
        "sift_hip_verify_fundamental_host": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, ctypes.POINTER(_VerifyParams),
                                                 ctypes.POINTER(_VerifyResult), vp, vp]),
        "sift_hip_score_fundamental_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, i, f, vp, vp]),
        "sift_hip_verify_hypotheses_host": (i, [vp, vp, vp, vp, i]),
        "sift_hip_verify_homography_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, ctypes.POINTER(_VerifyParams), vp,
                                                  vp, vp, vp, vp]),
        "sift_hip_verify_homography_host": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, ctypes.POINTER(_VerifyParams),
                                                ctypes.POINTER(_HomographyResult), vp, vp]),
        "sift_hip_score_homography_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, i, f, vp, vp]),
        "sift_hip_verify_homography_hypotheses_host": (i, [vp, vp, vp, vp, i]),
        "sift_hip_project_homography_device": (i, [vp, vp, i, i, vp, i, vp]),
        "sift_hip_verifier_create_batched": (i, [i, i, i, i, ctypes.POINTER(vp)]),
        "sift_hip_verify_fundamental_batched_device": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i,
                                                           ctypes.POINTER(_VerifyParams), vp, vp, vp, vp, vp]),
        "sift_hip_verify_fundamental_batched_host": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i,
                                                         ctypes.POINTER(_VerifyParams), vp, vp, vp]),
        "sift_hip_verify_homography_batched_device": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i,
                                                          ctypes.POINTER(_VerifyParams), vp, vp, vp, vp, vp]),
        "sift_hip_verify_homography_batched_host": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i,
                                                        ctypes.POINTER(_VerifyParams), vp, vp, vp]),
        "sift_hip_refine_fundamental_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, f, i, vp, vp, vp, vp, vp, vp]),
        "sift_hip_refine_fundamental_host": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, f, i, vp, vp, vp, ip, ip]),
        "sift_hip_refine_homography_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, f, i, vp, vp, vp, vp, vp, vp]),
        "sift_hip_refine_homography_host": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, f, i, vp, vp, vp, ip, ip]),
        "sift_hip_refine_fundamental_batched_device": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, f, i, vp, vp,
                                                           vp, vp, vp, vp]),
        "sift_hip_refine_fundamental_batched_host": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, f, i, vp, vp,
                                                         vp, vp, vp]),
        "sift_hip_refine_homography_batched_device": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, f, i, vp, vp,
                                                          vp, vp, vp, vp]),
        "sift_hip_refine_homography_batched_host": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, f, i, vp, vp,
                                                        vp, vp, vp]),
        "sift_hip_verifier_reserve_essential": (i, [vp, i]),
        "sift_hip_verify_essential_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, vp, ctypes.POINTER(_VerifyParams),
                                                 vp, vp, vp, vp, vp]),
        "sift_hip_verify_essential_host": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, vp, ctypes.POINTER(_VerifyParams),
                                               ctypes.POINTER(_VerifyResult), vp, vp]),
        "sift_hip_verify_essential_batched_device": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, vp, vp,
                                                         ctypes.POINTER(_VerifyParams), vp, vp, vp, vp, vp]),
        "sift_hip_verify_essential_batched_host": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, vp, vp,
                                                       ctypes.POINTER(_VerifyParams), vp, vp, vp]),
        "sift_hip_verify_essential_hypotheses_host": (i, [vp, vp, vp, vp, i]),
        "sift_hip_verify_affine_device": (i, [vp, i, vp, vp, i, vp, i, i, vp, i, i, ctypes.POINTER(_VerifyParams), vp,
                                              vp, vp, vp, vp]),
        "sift_hip_verify_affine_host": (i, [vp, i, vp, vp, i, vp, i, i, vp, i, i, ctypes.POINTER(_VerifyParams),
                                            ctypes.POINTER(_HomographyResult), vp, vp]),
        "sift_hip_score_affine_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, i, f, vp, vp]),
        "sift_hip_verify_affine_hypotheses_host": (i, [vp, i, vp, vp, vp, i]),
        "sift_hip_verify_affine_batched_device": (i, [vp, i, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i,
                                                      ctypes.POINTER(_VerifyParams), vp, vp, vp, vp, vp]),
        "sift_hip_verify_affine_batched_host": (i, [vp, i, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i,
                                                    ctypes.POINTER(_VerifyParams), vp, vp, vp]),
        "sift_hip_refine_affine_device": (i, [vp, i, vp, vp, i, vp, i, i, vp, i, i, f, i, vp, vp, vp, vp, vp, vp]),
        "sift_hip_refine_affine_host": (i, [vp, i, vp, vp, i, vp, i, i, vp, i, i, f, i, vp, vp, vp, ip, ip]),
        "sift_hip_refine_affine_batched_device": (i, [vp, i, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, f, i, vp, vp,
                                                      vp, vp, vp, vp]),
        "sift_hip_refine_affine_batched_host": (i, [vp, i, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, f, i, vp, vp,
                                                    vp, vp, vp]),
        "sift_hip_default_pose_params": (None, [ctypes.POINTER(_PoseParams)]),
        "sift_hip_recover_pose_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, vp, ctypes.POINTER(_Camera),
                                             ctypes.POINTER(_Camera), ctypes.POINTER(_PoseParams), vp, vp, vp, vp, vp, vp]),
        "sift_hip_recover_pose_host": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, vp, ctypes.POINTER(_Camera),
                                           ctypes.POINTER(_Camera), ctypes.POINTER(_PoseParams), vp, vp, vp, vp, ip]),
        "sift_hip_recover_pose_batched_device": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, vp, vp,
                                                     ctypes.POINTER(_Camera), ctypes.POINTER(_Camera),
                                                     ctypes.POINTER(_PoseParams), vp, vp, vp, vp, vp, vp]),
        "sift_hip_recover_pose_batched_host": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, vp, vp,
                                                   ctypes.POINTER(_Camera), ctypes.POINTER(_Camera),
                                                   ctypes.POINTER(_PoseParams), vp, vp, vp, vp, vp]),
        "sift_hip_recover_pose_homography_device": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, vp,
                                                        ctypes.POINTER(_Camera), ctypes.POINTER(_Camera),
                                                        ctypes.POINTER(_PoseParams), vp, vp, vp, vp, vp, vp, vp]),
        "sift_hip_recover_pose_homography_host": (i, [vp, vp, vp, i, vp, i, i, vp, i, i, vp, vp,
                                                      ctypes.POINTER(_Camera), ctypes.POINTER(_Camera),
                                                      ctypes.POINTER(_PoseParams), vp, vp, vp, vp, ip, vp]),
        "sift_hip_recover_pose_homography_batched_device": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, vp,
                                                                vp, ctypes.POINTER(_Camera), ctypes.POINTER(_Camera),
                                                                ctypes.POINTER(_PoseParams), vp, vp, vp, vp, vp, vp,
                                                                vp]),
        "sift_hip_recover_pose_homography_batched_host": (i, [vp, vp, vp, i, ctypes.POINTER(_VerifyPair), i, i, vp, vp,
                                                              ctypes.POINTER(_Camera), ctypes.POINTER(_Camera),
                                                              ctypes.POINTER(_PoseParams), vp, vp, vp, vp, vp, vp]),
        "sift_synth_frame": (i, [ctypes.c_uint, i, i, vp]),
        "sift_hip_device_count": (i, [ip]),
        "sift_hip_set_device": (i, [i]),
        "sift_hip_memcpy_d2d": (i, [vp, vp, sz, vp]),
        "sift_hip_comm_create": (i, [i, ip, ctypes.POINTER(vp)]),
        "sift_hip_comm_destroy": (i, [vp]),
        "sift_hip_comm_size": (i, [vp, ip]),
        "sift_hip_comm_allgather": (i, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), sz, ctypes.POINTER(vp)]),
        "sift_hip_malloc": (i, [ctypes.POINTER(vp), sz]),
        "sift_hip_free": (i, [vp]),
        "sift_hip_memcpy_h2d": (i, [vp, vp, sz]),
        "sift_hip_memcpy_d2h": (i, [vp, vp, sz]),
        "sift_hip_device_sync": (i, []),
    }
    for name, (res, args) in sigs.items():
        if os.environ.get("SIFT_HIP_LIB") and not hasattr(L, name):
            continue  # an older A/B build (tools/ab_build.sh) may predate an entry point
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != SIFT_HIP_OK:
        msg = lib().sift_hip_last_error().decode(errors="replace")
        raise SiftHipError(f"{what} failed ({rc}): {msg}")


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def version() -> str:
    """'abi=<n> arch=gfx950 hip=<ver> build=default' or 'build=ab <A/B macros>'."""
    return lib().sift_hip_version().decode()


def is_default_build() -> bool:
    """False for a library built with kernel A/B or instrumentation macros
    (tools/ab_variant.sh): bench.py and smoke() refuse to report from one."""
    return "build=default" in version()


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().sift_hip_device_count(ctypes.byref(n))
    return n.value


def synth_frame(index: int, width: int, height: int) -> np.ndarray:
    """Deterministic synthetic frame: float32 HxW, integers 0..255."""
    out = np.empty((height, width), np.float32)
    _check(lib().sift_synth_frame(index, width, height, _ptr(out)), "sift_synth_frame")
    return out


@dataclass
class CudaSiftConfig:
    """/root/reference/sift_cuda/types/CudaSiftConfig.hh:3-14 (+ numOctaves, maxKeypoints)."""

    col_width: int = 0
    row_width: int = 0
    numFeatures: int = 5000
    numOctaveLayers: int = 3
    contrastThreshould: float = 0.04
    edgeThreshould: float = 10.0
    sigma: float = 1.6
    upscale: bool = False
    numOctaves: int = 0
    maxKeypoints: int = 0

    def _abi(self) -> _Config:
        c = _Config()
        for name, _ in _Config._fields_:
            setattr(c, name, int(getattr(self, name)) if name == "upscale" else getattr(self, name))
        return c


class DeviceBuffer:
    """Non-owning device array view (stands in for thrust::device_vector).
    data() is for reading; a caller that writes into a detector's descriptor
    buffer takes mutable_data(), which drops the buffer's matcher sidecar
    (sift_hip_descriptors_written) so matches convert the written rows."""

    def __init__(self, ptr: int, size: int, descriptors: bool = False):
        self.ptr, self._size, self._desc = int(ptr or 0), int(size), descriptors

    def data(self) -> int:
        return self.ptr

    def mutable_data(self) -> int:
        if self._desc and self.ptr:
            _check(lib().sift_hip_descriptors_written(self.ptr), "descriptors_written")
        return self.ptr

    def size(self) -> int:
        return self._size


class Detector:
    """sift_cuda::Detector (Detector.hh:24-96) over the C ABI."""

    def __init__(self, config: CudaSiftConfig, device: int = -1, batch: int = 1, exact_descriptors: bool = False,
                 lanes: Optional[int] = None, micro_batch: int = 1, auto_micro_batch: Optional[int] = None,
                 root_sift: bool = False):
        """batch > 1: frame-batch handle (sift_hip_set_batch): detectBatchDevice runs up to `batch`
        frames per launch; the single-frame methods keep working (frame 0's arena).
        exact_descriptors: OpenCV's sequential float histogram (SIFT_HIP_DESC_EXACT), descriptors
        bit-identical to the oracle; default the fixed-point histogram (+-1 on a byte).
        lanes: compute lanes for frames in flight (sift_hip_set_lanes, 1..4, library default 2):
        frames submitted before the previous one completes run concurrently on another lane.
        micro_batch > 1: frames of submitDevice queue until that many run as one launch group on a
        lane (sift_hip_set_micro_batch; a wait on a queued frame launches the partial group).
        auto_micro_batch: automatic launch groups of up to that many frames once every lane is busy
        (sift_hip_set_auto_micro_batch; library default 8, 0 = off).
        root_sift: RootSIFT rows (SIFT_HIP_NORM_ROOT): every descriptor row the detector writes is
        cv.rootsift of the row it would have written, computed in the descriptor kernel; keypoints
        are unchanged.  Independent of exact_descriptors."""
        self.config = config
        self.batch = int(batch)
        self.exact_descriptors = bool(exact_descriptors)
        self.root_sift = bool(root_sift)
        self._h = ctypes.c_void_p()
        _check(lib().sift_hip_create(ctypes.byref(config._abi()), device, ctypes.byref(self._h)), "sift_hip_create")
        if self.batch != 1:
            _check(lib().sift_hip_set_batch(self._h, self.batch), "set_batch")
        if lanes is not None:
            _check(lib().sift_hip_set_lanes(self._h, int(lanes)), "set_lanes")
        if micro_batch != 1:
            _check(lib().sift_hip_set_micro_batch(self._h, int(micro_batch)), "set_micro_batch")
        if auto_micro_batch is not None:
            _check(lib().sift_hip_set_auto_micro_batch(self._h, int(auto_micro_batch)), "set_auto_micro_batch")
        if self.exact_descriptors:
            _check(lib().sift_hip_set_descriptor_mode(self._h, SIFT_HIP_DESC_EXACT), "set_descriptor_mode")
        if self.root_sift:
            _check(lib().sift_hip_set_descriptor_norm(self._h, SIFT_HIP_NORM_ROOT), "set_descriptor_norm")
        n = ctypes.c_int()
        lib().sift_hip_num_octaves(self._h, ctypes.byref(n))
        self.nOctaves = n.value
        self.total_size = 0
        self.prev_size = 0
        self.final_kpts = np.zeros((0, 3), np.float32)
        self.final_features = np.zeros((0, 4), np.float32)
        self.descriptors = np.zeros((0, 128), np.float16)
        self.device_kpts = self.device_features = self.device_descriptor = self.prev_descriptor = DeviceBuffer(0, 0)
        self._ready = False
        self._rb = None     # _refresh's ctypes holders
        self._views = None  # the pointers the result views were built from

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and h.value and _lib is not None:
            _lib.sift_hip_destroy(h)
            self._h = None

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def gpuWarmUpAndAllocate(self) -> bool:
        if not self._ready:
            _check(lib().sift_hip_warmup(self._h), "gpuWarmUpAndAllocate")
            self._ready = True
            self._refresh()
        return True

    def octave_dims(self, o: int):
        w, h, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().sift_hip_octave_dims(self._h, o, ctypes.byref(w), ctypes.byref(h), ctypes.byref(p)), "octave_dims")
        return w.value, h.value, p.value

    def _refresh(self) -> None:
        # Called after every frame: the ctypes holders are made once per
        # detector and the result views are rebuilt only when a pointer changed
        # (each ctypes call and object here is ~1 us of a ~0.23 ms frame).
        if self._rb is None:
            vals = [ctypes.c_void_p() for _ in range(4)] + [ctypes.c_int() for _ in range(4)]
            self._rb = (vals, [ctypes.byref(v) for v in vals])
        (k3, f4, d, pd, pc, cap, n, flags), refs = self._rb
        L = lib()
        _check(L.sift_hip_results_device(self._h, refs[0], refs[1], refs[2], refs[3], refs[4], refs[5]), "results")
        key = (k3.value, f4.value, d.value, pd.value, cap.value)
        if key != self._views:
            self._views = key
            self.device_kpts = DeviceBuffer(k3.value, cap.value)
            self.device_features = DeviceBuffer(f4.value, cap.value)
            self.device_descriptor = DeviceBuffer(d.value, cap.value * 128, descriptors=True)
            self.prev_descriptor = DeviceBuffer(pd.value, cap.value * 128, descriptors=True)
        self.prev_size = pc.value
        L.sift_hip_num_keypoints(self._h, refs[6])
        self.total_size = n.value
        L.sift_hip_overflow_flags(self._h, refs[7])
        self._warn_overflow(flags.value)

    def _warn_overflow(self, flags: Optional[int] = None) -> None:
        """A stage that hit its capacity clamps and sets a bit (keypoints the reference would keep are
        dropped): warned once per detector and flag (SiftCapacityWarning)."""
        if flags is None:
            flags = self.overflow_flags()
        new = flags & ~getattr(self, "_overflow_warned", 0)
        if new:
            self._overflow_warned = getattr(self, "_overflow_warned", 0) | flags
        if new & SIFT_HIP_FLAG_BAD_KEYPOINT:
            warnings.warn("computeDevice met an invalid keypoint (flag 16, check_keypoints names it); its descriptor "
                          "row is zero", SiftKeypointWarning, stacklevel=3)
        if new & 15:
            warnings.warn(f"capacity overflow (flags {flags:#x}: 1 candidates, 2 refined, 4 oriented, 8 results); "
                          f"keypoints were dropped -- raise CudaSiftConfig.maxKeypoints", SiftCapacityWarning, stacklevel=3)

    def _host_frame(self, image: np.ndarray):
        """(array, format): uint8 frames stay 8-bit (Image8U); anything else is float32 (Imagef)."""
        if image.dtype == np.uint8:
            img, fmt = np.ascontiguousarray(image), SIFT_HIP_U8
        else:
            img, fmt = np.ascontiguousarray(image, dtype=np.float32), SIFT_HIP_F32
        if img.shape != (self.config.row_width, self.config.col_width):
            raise SiftHipError(f"image shape {img.shape} != configured {(self.config.row_width, self.config.col_width)}")
        return img, fmt

    def _host_mask(self, mask) -> np.ndarray:
        """A detection mask as the C ABI takes it: a 2-D uint8 array of the frame's shape whose last axis is
        contiguous (a strided view is passed with its row stride, not copied).  Host-only check."""
        if not isinstance(mask, np.ndarray) or mask.dtype != np.uint8:
            raise SiftHipError(f"mask must be a uint8 numpy array, got {getattr(mask, 'dtype', type(mask))}")
        shape = (self.config.row_width, self.config.col_width)
        if mask.ndim != 2 or mask.shape != shape:
            raise SiftHipError(f"mask shape {mask.shape} != configured {shape}")
        if mask.strides[1] != 1 or mask.strides[0] < mask.shape[1]:
            mask = np.ascontiguousarray(mask)
        return mask

    def detectAndCompute(self, image: np.ndarray, mask: Optional[np.ndarray] = None) -> None:
        """Detector.cu:133-233.  `image`: (rows, cols) float32 0..255 (Imagef) or uint8 (Image8U).
        `mask` (cv::SIFT's mask argument; sift_hip_detect_masked): uint8 (rows, cols); a keypoint is dropped when
        mask[int(y + 0.5), int(x + 0.5)] == 0 in float32 (sift_amd.cv.mask_keep), after retainBest(numFeatures)
        as in OpenCV, and every result holds the kept rows only.  None: the unmasked call."""
        if mask is not None:
            m = self._host_mask(mask)
            self.gpuWarmUpAndAllocate()
            img, fmt = self._host_frame(image)
            _check(lib().sift_hip_detect_masked(self._h, _ptr(img), img.strides[0], fmt, _ptr(m), m.strides[0]),
                   "detectAndCompute")
            self._refresh()
            return
        self.gpuWarmUpAndAllocate()
        img, fmt = self._host_frame(image)
        if fmt == SIFT_HIP_U8:
            _check(lib().sift_hip_detect_u8(self._h, _ptr(img), img.strides[0]), "detectAndCompute")
        else:
            _check(lib().sift_hip_detect(self._h, _ptr(img), img.strides[0]), "detectAndCompute")
        self._refresh()

    # --- descriptors for the caller's own keypoints (cv::Feature2D::compute) ------
    @staticmethod
    def _kpt_records(kpts) -> np.ndarray:
        k = np.ascontiguousarray(kpts, dtype=KPT_DTYPE) if not isinstance(kpts, np.ndarray) or kpts.dtype != KPT_DTYPE \
            else np.ascontiguousarray(kpts)
        return k.reshape(-1)

    def check_keypoints(self, kpts) -> int:
        """Index of the first keypoint (KPT_DTYPE records) compute would refuse, or -1 (sift_hip_check_keypoints;
        host-only, valid before warm-up).  More keypoints than the result capacity raise SiftHipError."""
        k = self._kpt_records(kpts)
        bad = ctypes.c_int(-1)
        _check(lib().sift_hip_check_keypoints(self._h, _ptr(k) if len(k) else None, len(k), ctypes.byref(bad)),
               "check_keypoints")
        return bad.value

    def compute(self, image: np.ndarray, kpts) -> None:
        """Descriptors of the caller's keypoints on `image` (float32 or uint8, as detectAndCompute):
        sift_hip_compute / sift_hip_compute_u8.  `kpts`: KPT_DTYPE records (sift_amd.cv.keypoint_records /
        from_cv_keypoints build them).  Counts as a frame: total_size = len(kpts), rows in the caller's order,
        device_kpts / device_features hold the input, prev_descriptor the previous frame's rows.  An invalid
        keypoint or more than the result capacity raises SiftHipError and leaves the previous results current."""
        self.gpuWarmUpAndAllocate()
        img, fmt = self._host_frame(image)
        k = self._kpt_records(kpts)
        fn = lib().sift_hip_compute_u8 if fmt == SIFT_HIP_U8 else lib().sift_hip_compute
        _check(fn(self._h, _ptr(img), img.strides[0], _ptr(k) if len(k) else None, len(k)), "compute")
        self._refresh()

    def computeDevice(self, dev_ptr: int, row_stride_bytes: int, kpts_dev_ptr: int, n: int, stream: Optional[int] = None,
                      u8: bool = False, sync: bool = True) -> None:
        """The same for a device image and n device keypoints (24-byte KPT_DTYPE records), enqueued after `stream`
        (sift_hip_compute_device).  Device keypoints are validated on the GPU: an invalid one gets an all-zero row
        and sets overflow_flags() bit 16."""
        self.gpuWarmUpAndAllocate()
        fmt = SIFT_HIP_U8 if u8 else SIFT_HIP_F32
        _check(lib().sift_hip_compute_device(self._h, dev_ptr, row_stride_bytes, fmt, kpts_dev_ptr or None, n, stream),
               "computeDevice")
        if sync:
            self.sync()

    def submit(self, image: np.ndarray) -> int:
        """Pipelined input (sift_hip_submit): stage + upload + enqueue, no wait.  Returns the frame ticket."""
        self.gpuWarmUpAndAllocate()
        img, fmt = self._host_frame(image)
        t = ctypes.c_longlong()
        _check(lib().sift_hip_submit(self._h, _ptr(img), img.strides[0], fmt, ctypes.byref(t)), "submit")
        return t.value

    def submitDevice(self, dev_ptr: int, row_stride_bytes: int = 0, stream: Optional[int] = None, u8: bool = False) -> int:
        """Pipelined device input (sift_hip_submit_device): the frame at dev_ptr is enqueued on a free lane
        after `stream`; returns the ticket for wait().  The buffer must stay unchanged until wait(ticket)."""
        self.gpuWarmUpAndAllocate()
        t = ctypes.c_longlong()
        _check(lib().sift_hip_submit_device(self._h, dev_ptr, row_stride_bytes, SIFT_HIP_U8 if u8 else SIFT_HIP_F32,
                                            stream, ctypes.byref(t)), "submitDevice")
        return t.value

    def lanes(self) -> tuple:
        """(lane limit, lanes created so far)."""
        m, c = ctypes.c_int(), ctypes.c_int()
        _check(lib().sift_hip_lanes(self._h, ctypes.byref(m), ctypes.byref(c)), "lanes")
        return m.value, c.value

    def micro_batch(self) -> int:
        """Frames per submitDevice launch group (sift_hip_micro_batch)."""
        m = ctypes.c_int()
        _check(lib().sift_hip_micro_batch(self._h, ctypes.byref(m)), "micro_batch")
        return m.value

    def auto_micro_batch(self) -> int:
        """Largest automatic launch group (sift_hip_auto_micro_batch; 0: automatic groups off)."""
        m = ctypes.c_int()
        _check(lib().sift_hip_auto_micro_batch(self._h, ctypes.byref(m)), "auto_micro_batch")
        return m.value

    def wait(self, ticket: int) -> None:
        """Block until frame `ticket` is complete and expose its results (prev = frame ticket-1)."""
        _check(lib().sift_hip_wait(self._h, ticket), "wait")
        self._refresh()

    def detectAndComputeDevice(self, dev_ptr: int, row_stride_bytes: int, stream: Optional[int] = None, sync: bool = True,
                               u8: bool = False, mask_ptr: Optional[int] = None, mask_stride: int = 0) -> None:
        """mask_ptr: a device detection mask (col_width x row_width bytes, rows mask_stride bytes apart, 0 = packed),
        read in place -- unchanged until sync, like the image (sift_hip_detect_device_masked)."""
        self.gpuWarmUpAndAllocate()
        fmt = SIFT_HIP_U8 if u8 else SIFT_HIP_F32
        if mask_ptr:
            _check(lib().sift_hip_detect_device_masked(self._h, dev_ptr, row_stride_bytes, fmt, mask_ptr, mask_stride, stream),
                   "detectAndComputeDevice")
        else:
            _check(lib().sift_hip_detect_device_fmt(self._h, dev_ptr, row_stride_bytes, fmt, stream), "detectAndComputeDevice")
        if sync:
            self.sync()

    def sync(self) -> None:
        _check(lib().sift_hip_sync(self._h), "sync")
        self._refresh()

    # --- frame batches ----------------------------------------------------------
    def detectBatchDevice(self, dev_ptr: int, n: int, row_stride_bytes: int = 0, frame_stride_bytes: int = 0,
                          stream: Optional[int] = None, sync: bool = True, u8: bool = False,
                          masks_ptr: Optional[int] = None, mask_stride: int = 0, mask_frame_stride: int = 0) -> None:
        """n (<= batch) device frames at dev_ptr + i * frame_stride_bytes, one launch per stage for all.
        masks_ptr: n device detection masks, mask i at masks_ptr + i * mask_frame_stride (0 = mask_stride * rows),
        rows mask_stride bytes apart (0 = packed): sift_hip_detect_batch_device_masked."""
        self.gpuWarmUpAndAllocate()
        fmt = SIFT_HIP_U8 if u8 else SIFT_HIP_F32
        if masks_ptr:
            _check(lib().sift_hip_detect_batch_device_masked(self._h, dev_ptr, n, row_stride_bytes, frame_stride_bytes, fmt,
                                                             masks_ptr, mask_stride, mask_frame_stride, stream),
                   "detectBatchDevice")
        else:
            _check(lib().sift_hip_detect_batch_device(self._h, dev_ptr, n, row_stride_bytes, frame_stride_bytes, fmt, stream),
                   "detectBatchDevice")
        if sync:
            self.sync()

    def results_sidecar(self):
        """(codes, keys) device pointers of the current frame's matcher sidecar (sift_hip_results_sidecar):
        int8 codes v - 128 per descriptor row (128 B) and int32 key biases -(256 |c|^2 + (row & 255))."""
        c, k = ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().sift_hip_results_sidecar(self._h, ctypes.byref(c), ctypes.byref(k)), "results_sidecar")
        return c.value, k.value

    def batch_frames(self) -> int:
        n = ctypes.c_int()
        _check(lib().sift_hip_batch_frames(self._h, ctypes.byref(n)), "batch_frames")
        return n.value

    def batch_results(self, i: int):
        """(count, overflow flags, device kpts3 / feats4 / descriptor pointers) of frame i of the current batch."""
        c, o = ctypes.c_int(), ctypes.c_int()
        k3, f4, d = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().sift_hip_batch_results_device(self._h, i, ctypes.byref(c), ctypes.byref(o), ctypes.byref(k3),
                                                   ctypes.byref(f4), ctypes.byref(d)), "batch_results")
        return c.value, o.value, k3.value, f4.value, d.value

    def batch_copy_to_host(self, i: int, descriptor: bool = True):
        """Host copies (kpts3 (n,3), feats4 (n,4), descriptors (n,128) fp16 or None) of frame i of the current batch."""
        n = self.batch_results(i)[0]
        k3 = np.zeros((n, 3), np.float32)
        f4 = np.zeros((n, 4), np.float32)
        d = np.zeros((n, 128), np.uint16) if descriptor else None
        got = ctypes.c_int()
        _check(lib().sift_hip_batch_copy_to_host(self._h, i, _ptr(k3), _ptr(f4), _ptr(d) if d is not None else None, n,
                                                 ctypes.byref(got)), "batch_copy_to_host")
        return k3, f4, (d.view(np.float16) if d is not None else None)

    def copyToHost(self, descriptor: bool = True) -> None:
        """Detector.cu:606-634."""
        n = self.total_size
        k3 = np.empty((n, 3), np.float32)
        f4 = np.empty((n, 4), np.float32)
        d = np.empty((n, 128), np.uint16) if descriptor else None
        _check(lib().sift_hip_copy_to_host(self._h, _ptr(k3), _ptr(f4), _ptr(d) if d is not None else None, n), "copyToHost")
        self.final_kpts, self.final_features = k3, f4
        if d is not None:
            self.descriptors = d.view(np.float16)

    def results_host(self, descriptor: bool = True):
        """(kpts3 (n,3), feats4 (n,4), descriptors (n,128) fp16 or None) of the
        current frame as read-only views of the handle's pinned host results
        (sift_hip_results_host: no copy into Python memory).  They stay valid
        while the frame is the current or the previous one; copy what must
        outlive that."""
        k3, f4, d, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        _check(lib().sift_hip_results_host(self._h, ctypes.byref(k3), ctypes.byref(f4),
                                           ctypes.byref(d) if descriptor else None, ctypes.byref(n)), "results_host")

        def view(ptr, ctype, cols, dtype):
            if n.value == 0:
                return np.zeros((0, cols), dtype)
            a = np.ctypeslib.as_array((ctype * (n.value * cols)).from_address(ptr)).reshape(n.value, cols)
            a.flags.writeable = False
            return a

        kp = view(k3.value, ctypes.c_float, 3, np.float32)
        ft = view(f4.value, ctypes.c_float, 4, np.float32)
        ds = view(d.value, ctypes.c_uint16, 128, np.uint16).view(np.float16) if descriptor else None
        return kp, ft, ds

    def capacities(self) -> dict:
        """Per-frame buffer capacities (sift_hip_capacities; host-only)."""
        v = [ctypes.c_int() for _ in range(4)]
        _check(lib().sift_hip_capacities(self._h, *[ctypes.byref(x) for x in v]), "capacities")
        return dict(zip(("candidates", "refined", "oriented", "results"), (x.value for x in v)))

    def overflow_flags(self) -> int:
        v = ctypes.c_int()
        lib().sift_hip_overflow_flags(self._h, ctypes.byref(v))
        return v.value

    # --- parity/debug helpers -------------------------------------------------
    def debug_gaussian(self, octave: int, layer: int) -> np.ndarray:
        w, h, _ = self.octave_dims(octave)
        out = np.empty((h, w), np.float32)
        _check(lib().sift_hip_debug_gaussian(self._h, octave, layer, _ptr(out)), "debug_gaussian")
        return out

    def debug_candidates(self, cap: int = 1 << 20, return_count: bool = False):
        """The stored candidate rows (octave, layer, r, c): min(hits, candidate capacity, cap) of them.
        return_count=True: (rows, hits), hits counting every extremum met, stored or not (more than
        the capacity on overflow flag 1)."""
        q = np.zeros((cap, 4), np.int32)
        cnt = ctypes.c_int()
        _check(lib().sift_hip_debug_candidates(self._h, _ptr(q), cap, ctypes.byref(cnt)), "debug_candidates")
        rows = q[: min(cnt.value, cap, self.capacities()["candidates"])]
        return (rows, cnt.value) if return_count else rows

    def setDataGen(self, path: str) -> None:
        """Detector.hh:48-51: from now on every single-frame detect writes its stage
        dumps into `path` (sift_hip_set_datagen; "" switches them off)."""
        _check(lib().sift_hip_set_datagen(self._h, (path or "").encode()), "setDataGen")

    STAGES = ("pyramid", "extrema", "refine", "orientation", "order", "descriptor")

    def replayStage(self, dump_dir: str, stage: str, out_dir: str) -> None:
        """tool/perf.cu:43-100: run ONE pipeline stage on a setDataGen dump's
        recorded input (sift_hip_replay_stage); outputs go to out_dir in the
        dump's file formats.  The handle's current results are discarded."""
        self.gpuWarmUpAndAllocate()
        _check(lib().sift_hip_replay_stage(self._h, dump_dir.encode(), stage.encode(), out_dir.encode()),
               f"replayStage({stage})")
        self._refresh()

    # --- stage timing (roofline) ---------------------------------------------
    def set_timing(self, enable, blur_reps: int = 1) -> None:
        mode = (blur_reps if blur_reps > 1 else 1) if enable else 0
        _check(lib().sift_hip_set_timing(self._h, mode), "set_timing")

    def timing(self) -> dict:
        n = ctypes.c_int()
        lib().sift_hip_timing_count(self._h, ctypes.byref(n))
        out = {}
        for k in range(n.value):
            name, ms, nl, by = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
            _check(lib().sift_hip_timing_entry(self._h, k, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(nl), ctypes.byref(by)), "timing")
            out[name.value.decode()] = {"ms": ms.value, "launches": nl.value, "bytes": by.value}
        return out

    def timing_reset(self) -> None:
        lib().sift_hip_timing_reset(self._h)


class Matcher:
    """Brute-force L2 matcher (replaces Match.cu:8-177) with preallocated scratch."""

    @staticmethod
    def plan(max_query: int, max_train: int, pairs: int = 1) -> tuple:
        """(train splits per query block, waves per workgroup) a call of this
        shape launches with (sift_hip_match_plan; host-only)."""
        S, nw = ctypes.c_int(), ctypes.c_int()
        _check(lib().sift_hip_match_plan(max_query, max_train, pairs, ctypes.byref(S), ctypes.byref(nw)), "match_plan")
        return S.value, nw.value

    def __init__(self, max_query: int, max_train: int, max_pairs: int = 1, device: int = -1):
        self._m = ctypes.c_void_p()
        self.max_query, self.max_train, self.max_pairs = max_query, max_train, max_pairs
        _check(lib().sift_hip_matcher_create(device, max_query, max_train, max_pairs, ctypes.byref(self._m)), "matcher_create")

    def __del__(self):
        m = getattr(self, "_m", None)
        if m and m.value and _lib is not None:
            _lib.sift_hip_matcher_destroy(m)
            self._m = None

    def set_sidecars(self, enable: bool) -> None:
        """Single pairs of detector-produced buffers match their sidecar codes (default on; sift_hip_matcher_set_sidecars)."""
        _check(lib().sift_hip_matcher_set_sidecars(self._m, int(bool(enable))), "matcher_set_sidecars")

    def match_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, ratio: float = 0.8, ratio_on_squared: bool = False,
                     idx2_ptr: int = 0, d2_ptr: int = 0, match_ptr: int = 0, stream: Optional[int] = None) -> None:
        _check(lib().sift_hip_match_device(self._m, q_ptr, nq, t_ptr, nt, ratio, int(ratio_on_squared),
                                           idx2_ptr or None, d2_ptr or None, match_ptr or None, stream), "match_device")

    def match_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int], nts: Sequence[int],
                      ratio: float = 0.8, ratio_on_squared: bool = False, idx2_ptr: int = 0, d2_ptr: int = 0,
                      match_ptr: int = 0, stream: Optional[int] = None) -> None:
        P = len(q_ptrs)
        qa = (ctypes.c_void_p * P)(*q_ptrs)
        ta = (ctypes.c_void_p * P)(*t_ptrs)
        na = (ctypes.c_int * P)(*nqs)
        ma = (ctypes.c_int * P)(*nts)
        _check(lib().sift_hip_match_batched(self._m, P, qa, na, ta, ma, ratio, int(ratio_on_squared),
                                            idx2_ptr or None, d2_ptr or None, match_ptr or None, stream), "match_batched")

    def match_codes_batched(self, codes_ptr: int, keys_ptr: int, pairs: Sequence, ratio: float = 0.8,
                            ratio_on_squared: bool = False, idx2_ptr: int = 0, d2_ptr: int = 0, match_ptr: int = 0,
                            stream: Optional[int] = None) -> None:
        """Pairs (qrow0, qkey0, nq, trow0, tkey0, nt) of ready code sets -- int8 codes (128 B rows from code row
        qrow0 / trow0) and int32 key biases (from key index qkey0 / tkey0), e.g. every rank's sidecar all-gathered
        (multi.all_gather_codes / multi.code_pairs) -- in ONE launch, no conversion
        (sift_hip_match_codes_batched).  Outputs packed per pair as match_batched."""
        P = len(pairs)
        qr, qk, nq, tr, tk, nt = ((ctypes.c_int * P)(*[p[k] for p in pairs]) for k in range(6))
        _check(lib().sift_hip_match_codes_batched(self._m, codes_ptr, keys_ptr, P, qr, qk, nq, tr, tk, nt, ratio,
                                                  int(ratio_on_squared), idx2_ptr or None, d2_ptr or None,
                                                  match_ptr or None, stream), "match_codes_batched")

    def match_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, ratio: float = 0.8, ratio_on_squared: bool = True) -> np.ndarray:
        out = np.full(max(nq, 0), -1, np.int32)
        _check(lib().sift_hip_match_host(self._m, q_ptr, nq, t_ptr, nt, ratio, int(ratio_on_squared), _ptr(out)), "match_host")
        return out


    # --- match lists: match -> filter -> ordered compaction on the device (the rule: include/sift_hip.h, and in
    # numpy sift_amd.cv.filter_matches).  `filter` keywords: ratio=0.8, ratio_on_squared=False,
    # ratio_both_ways=False, max_distance=0 (off), cross_check=True.  The first list call of a matcher allocates its
    # scratch (not under stream capture).

    def match_list_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, out_ptr: int, count_ptr: int,
                          stream: Optional[int] = None, **filter) -> None:
        """DMATCH_DTYPE records of the kept queries, ascending queryIdx, at out_ptr (device, room for nq) and their
        number at count_ptr (device int32); enqueued on `stream` (sift_hip_match_list_device)."""
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_device(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(f), out_ptr or None,
                                                count_ptr or None, stream), "match_list_device")

    def match_list_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int], nts: Sequence[int],
                           out_ptr: int, counts_ptr: int, stream: Optional[int] = None, **filter) -> None:
        """P pairs: pair p's records at row sum(nqs[:p]) of out_ptr with imgIdx = p, its count at counts_ptr[p]
        (sift_hip_match_list_batched)."""
        P = len(q_ptrs)
        qa = (ctypes.c_void_p * P)(*q_ptrs)
        ta = (ctypes.c_void_p * P)(*t_ptrs)
        na = (ctypes.c_int * P)(*nqs)
        ma = (ctypes.c_int * P)(*nts)
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_batched(self._m, P, qa, na, ta, ma, ctypes.byref(f), out_ptr or None,
                                                 counts_ptr or None, stream), "match_list_batched")

    def match_list_codes_batched(self, codes_ptr: int, keys_ptr: int, pairs: Sequence, out_ptr: int, counts_ptr: int,
                                 stream: Optional[int] = None, **filter) -> None:
        """The same for pairs (qrow0, qkey0, nq, trow0, tkey0, nt) of ready code sets, as match_codes_batched takes
        them (sift_hip_match_list_codes_batched)."""
        P = len(pairs)
        qr, qk, nq, tr, tk, nt = ((ctypes.c_int * P)(*[p[k] for p in pairs]) for k in range(6))
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_codes_batched(self._m, codes_ptr, keys_ptr, P, qr, qk, nq, tr, tk, nt,
                                                       ctypes.byref(f), out_ptr or None, counts_ptr or None, stream),
               "match_list_codes_batched")

    def match_list_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, **filter) -> np.ndarray:
        """Synchronous; the kept records as a DMATCH_DTYPE array (sift_hip_match_list_host)."""
        out = np.zeros(max(nq, 0), DMATCH_DTYPE)
        f = _match_filter(**filter)
        n = ctypes.c_int(0)
        _check(lib().sift_hip_match_list_host(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(f), _ptr(out), len(out),
                                              ctypes.byref(n)), "match_list_host")
        return out[: n.value]

    # --- k nearest neighbours (k <= KNN_MAX) and capped radius lists (the rule: include/sift_hip.h, and in numpy
    # sift_amd.cv.knn / knn_records).  Tables are (nq, k) int32 indices (-1: none) and float32 squared distances
    # (FLT_MAX: none) in ascending (d2, train index) order.  The first k-NN call of a matcher allocates its scratch
    # (not under stream capture).

    @staticmethod
    def knn_plan(nq: int, nt: int, pairs: int = 1, k: int = KNN_MAX) -> int:
        """Train splits a k-NN call of this shape launches with (sift_hip_match_knn_plan; host-only)."""
        S = ctypes.c_int()
        _check(lib().sift_hip_match_knn_plan(nq, nt, pairs, k, ctypes.byref(S)), "match_knn_plan")
        return S.value

    def match_knn_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, k: int, idx_ptr: int = 0, d2_ptr: int = 0,
                         stream: Optional[int] = None) -> None:
        """The table of one pair at idx_ptr / d2_ptr (device, nq * k entries each; 0 skips one); enqueued on `stream`
        (sift_hip_match_knn_device)."""
        _check(lib().sift_hip_match_knn_device(self._m, q_ptr or None, nq, t_ptr or None, nt, k, idx_ptr or None,
                                               d2_ptr or None, stream), "match_knn_device")

    def match_knn_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int], nts: Sequence[int],
                          k: int, idx_ptr: int = 0, d2_ptr: int = 0, stream: Optional[int] = None) -> None:
        """P pairs in one launch: pair p's rows from row sum(nqs[:p]) (sift_hip_match_knn_batched)."""
        P = len(q_ptrs)
        qa = (ctypes.c_void_p * P)(*q_ptrs)
        ta = (ctypes.c_void_p * P)(*t_ptrs)
        na = (ctypes.c_int * P)(*nqs)
        ma = (ctypes.c_int * P)(*nts)
        _check(lib().sift_hip_match_knn_batched(self._m, P, qa, na, ta, ma, k, idx_ptr or None, d2_ptr or None, stream),
               "match_knn_batched")

    def match_knn_codes_batched(self, codes_ptr: int, keys_ptr: int, pairs: Sequence, k: int, idx_ptr: int = 0,
                                d2_ptr: int = 0, stream: Optional[int] = None) -> None:
        """The same for pairs (qrow0, qkey0, nq, trow0, tkey0, nt) of ready code sets, as match_codes_batched takes
        them (sift_hip_match_knn_codes_batched)."""
        P = len(pairs)
        qr, qk, nq, tr, tk, nt = ((ctypes.c_int * P)(*[p[j] for p in pairs]) for j in range(6))
        _check(lib().sift_hip_match_knn_codes_batched(self._m, codes_ptr, keys_ptr, P, qr, qk, nq, tr, tk, nt, k,
                                                      idx_ptr or None, d2_ptr or None, stream), "match_knn_codes_batched")

    def match_knn_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, k: int):
        """Synchronous; (idx int32 (nq, k), d2 float32 (nq, k)) (sift_hip_match_knn_host)."""
        shape = (max(nq, 0), max(k, 0))
        idx, d2 = np.full(shape, -1, np.int32), np.full(shape, np.finfo(np.float32).max, np.float32)
        _check(lib().sift_hip_match_knn_host(self._m, q_ptr or None, nq, t_ptr or None, nt, k, _ptr(idx), _ptr(d2)),
               "match_knn_host")
        return idx, d2

    def match_knn_list_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, k: int, out_ptr: int, count_ptr: int,
                              max_distance: float = 0.0, stream: Optional[int] = None) -> None:
        """DMATCH_DTYPE records of the neighbours within max_distance (<= 0: all), (queryIdx, rank) order, at out_ptr
        (device, room for nq * k) and their number at count_ptr (device int32) (sift_hip_match_knn_list_device)."""
        _check(lib().sift_hip_match_knn_list_device(self._m, q_ptr or None, nq, t_ptr or None, nt, k, max_distance,
                                                    out_ptr or None, count_ptr or None, stream), "match_knn_list_device")

    def match_knn_list_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                               nts: Sequence[int], k: int, out_ptr: int, counts_ptr: int, max_distance: float = 0.0,
                               stream: Optional[int] = None) -> None:
        """P pairs: pair p's records from row k * sum(nqs[:p]) of out_ptr with imgIdx = p, its count at counts_ptr[p]
        (sift_hip_match_knn_list_batched)."""
        P = len(q_ptrs)
        qa = (ctypes.c_void_p * P)(*q_ptrs)
        ta = (ctypes.c_void_p * P)(*t_ptrs)
        na = (ctypes.c_int * P)(*nqs)
        ma = (ctypes.c_int * P)(*nts)
        _check(lib().sift_hip_match_knn_list_batched(self._m, P, qa, na, ta, ma, k, max_distance, out_ptr or None,
                                                     counts_ptr or None, stream), "match_knn_list_batched")

    def match_knn_list_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, k: int, max_distance: float = 0.0) -> np.ndarray:
        """Synchronous; the kept records as a DMATCH_DTYPE array (sift_hip_match_knn_list_host)."""
        out = np.zeros(max(nq, 0) * max(k, 0), DMATCH_DTYPE)
        n = ctypes.c_int(0)
        _check(lib().sift_hip_match_knn_list_host(self._m, q_ptr or None, nq, t_ptr or None, nt, k, max_distance,
                                                  _ptr(out), len(out), ctypes.byref(n)), "match_knn_list_host")
        return out[: n.value]

    # --- guided matching: the same operations restricted to a search window (the rule: include/sift_hip.h, and in
    # numpy sift_amd.cv.gate_mask / guided_top2).  q_xy_ptr / t_xy_ptr: device float rows with x, y first (stride 3
    # passes a detector's device_kpts as it is); train row t is a candidate of query i when |tx - qx| <= radius and
    # |ty - qy| <= radius.  One pair per call.

    @staticmethod
    def guided_plan(nq: int, nt: int) -> int:
        """Train splits a guided call of this shape launches with (sift_hip_match_guided_plan; host-only)."""
        S = ctypes.c_int()
        _check(lib().sift_hip_match_guided_plan(nq, nt, ctypes.byref(S)), "match_guided_plan")
        return S.value

    def match_guided_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, radius: float,
                            q_stride: int = 3, t_stride: int = 3, ratio: float = 0.8, ratio_on_squared: bool = False,
                            idx2_ptr: int = 0, d2_ptr: int = 0, match_ptr: int = 0, stream: Optional[int] = None) -> None:
        """match_device over each query's candidates only (sift_hip_match_guided_device)."""
        g = _MatchGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius)
        _check(lib().sift_hip_match_guided_device(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(g), ratio,
                                                  int(ratio_on_squared), idx2_ptr or None, d2_ptr or None,
                                                  match_ptr or None, stream), "match_guided_device")

    def match_list_guided_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int,
                                 radius: float, out_ptr: int, count_ptr: int, q_stride: int = 3, t_stride: int = 3,
                                 stream: Optional[int] = None, **filter) -> None:
        """match_list_device with the guided top-2 of both directions (sift_hip_match_list_guided_device)."""
        g = _MatchGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius)
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_guided_device(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(g), ctypes.byref(f),
                                                       out_ptr or None, count_ptr or None, stream),
               "match_list_guided_device")

    def match_list_guided_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int,
                               radius: float, q_stride: int = 3, t_stride: int = 3, **filter) -> np.ndarray:
        """Synchronous; the kept records as a DMATCH_DTYPE array (sift_hip_match_list_guided_host)."""
        out = np.zeros(max(nq, 0), DMATCH_DTYPE)
        g = _MatchGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius)
        f = _match_filter(**filter)
        n = ctypes.c_int(0)
        _check(lib().sift_hip_match_list_guided_host(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(g), ctypes.byref(f),
                                                     _ptr(out), len(out), ctypes.byref(n)), "match_list_guided_host")
        return out[: n.value]

    # --- guided matching under a fundamental matrix: the same operations with the epipolar gate (the rule:
    # include/sift_hip.h, and in numpy sift_amd.cv.epipolar_mask / epipolar_top2).  F: 9 floats, row-major, with
    # x_train^T F x_query = 0; train row t is a candidate of query i when its Sampson distance is <= max_error and it
    # lies in the window `radius` (inf: none).  The launch shape is guided_plan's.

    def match_epipolar_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, F,
                              max_error: float, radius: float = float("inf"), q_stride: int = 3, t_stride: int = 3,
                              ratio: float = 0.8, ratio_on_squared: bool = False, idx2_ptr: int = 0, d2_ptr: int = 0,
                              match_ptr: int = 0, stream: Optional[int] = None) -> None:
        """match_device over each query's candidates only (sift_hip_match_epipolar_device)."""
        g = _epipolar_gate(q_xy_ptr, q_stride, t_xy_ptr, t_stride, radius, F, max_error)
        _check(lib().sift_hip_match_epipolar_device(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(g), ratio,
                                                    int(ratio_on_squared), idx2_ptr or None, d2_ptr or None,
                                                    match_ptr or None, stream), "match_epipolar_device")

    def match_list_epipolar_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, F,
                                   max_error: float, out_ptr: int, count_ptr: int, radius: float = float("inf"),
                                   q_stride: int = 3, t_stride: int = 3, stream: Optional[int] = None,
                                   **filter) -> None:
        """match_list_device with the epipolar top-2 of both directions (sift_hip_match_list_epipolar_device)."""
        g = _epipolar_gate(q_xy_ptr, q_stride, t_xy_ptr, t_stride, radius, F, max_error)
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_epipolar_device(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(g), ctypes.byref(f),
                                                         out_ptr or None, count_ptr or None, stream),
               "match_list_epipolar_device")

    def match_list_epipolar_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, F,
                                 max_error: float, radius: float = float("inf"), q_stride: int = 3, t_stride: int = 3,
                                 **filter) -> np.ndarray:
        """Synchronous; the kept records as a DMATCH_DTYPE array (sift_hip_match_list_epipolar_host)."""
        out = np.zeros(max(nq, 0), DMATCH_DTYPE)
        g = _epipolar_gate(q_xy_ptr, q_stride, t_xy_ptr, t_stride, radius, F, max_error)
        f = _match_filter(**filter)
        n = ctypes.c_int(0)
        _check(lib().sift_hip_match_list_epipolar_host(self._m, q_ptr, nq, t_ptr, nt, ctypes.byref(g), ctypes.byref(f),
                                                       _ptr(out), len(out), ctypes.byref(n)), "match_list_epipolar_host")
        return out[: n.value]

    # --- batched guided matching: both gates for all pairs of a batch in one pass (the rule: include/sift_hip.h).
    # positions: per pair (q_xy_ptr, nq, t_xy_ptr, nt) as multi.position_pairs returns them, or (q_xy_ptr, t_xy_ptr);
    # the strides and the radius are the call's.  Under the epipolar gate geometry_ptr is DEVICE memory: pair p's nine
    # floats at geometry_ptr + p * geometry_stride bytes -- with the default stride, 52, the VERIFY_RESULT_DTYPE
    # records of Verifier.verify_batched_device as they lie.  A pair whose record is not usable
    # (sift_amd.cv.geometry_usable: a non-finite entry, or all zero) has no candidates.  Outputs are laid out as
    # match_batched's / match_list_batched's.

    @staticmethod
    def _positions(positions: Sequence, P: int):
        if len(positions) != P:
            raise ValueError("one position pair per pair of sets")
        rec = [(p[0], p[2]) if len(p) == 4 else (p[0], p[1]) for p in positions]
        return (_MatchPositions * max(P, 1))(*[_MatchPositions(a or None, b or None) for a, b in rec])

    @staticmethod
    def _sets(q_ptrs, nqs, t_ptrs, nts):
        P = len(q_ptrs)
        return (P, (ctypes.c_void_p * P)(*q_ptrs), (ctypes.c_int * P)(*nqs), (ctypes.c_void_p * P)(*t_ptrs),
                (ctypes.c_int * P)(*nts))

    def match_guided_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int], nts: Sequence[int],
                             positions: Sequence, radius: float, q_stride: int = 3, t_stride: int = 3,
                             ratio: float = 0.8, ratio_on_squared: bool = False, idx2_ptr: int = 0, d2_ptr: int = 0,
                             match_ptr: int = 0, stream: Optional[int] = None) -> None:
        """match_batched under the window gate (sift_hip_match_guided_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        _check(lib().sift_hip_match_guided_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P), q_stride,
                                                   t_stride, radius, ratio, int(ratio_on_squared), idx2_ptr or None,
                                                   d2_ptr or None, match_ptr or None, stream), "match_guided_batched")

    def match_epipolar_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                               nts: Sequence[int], positions: Sequence, geometry_ptr: int, max_error: float,
                               radius: float = float("inf"), geometry_stride: int = 52, q_stride: int = 3,
                               t_stride: int = 3, ratio: float = 0.8, ratio_on_squared: bool = False, idx2_ptr: int = 0,
                               d2_ptr: int = 0, match_ptr: int = 0, stream: Optional[int] = None) -> None:
        """match_batched under the epipolar gate, F read on the device (sift_hip_match_epipolar_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        _check(lib().sift_hip_match_epipolar_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P), q_stride,
                                                     t_stride, radius, geometry_ptr or None, geometry_stride, max_error,
                                                     ratio, int(ratio_on_squared), idx2_ptr or None, d2_ptr or None,
                                                     match_ptr or None, stream), "match_epipolar_batched")

    def match_list_guided_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                                  nts: Sequence[int], positions: Sequence, radius: float, out_ptr: int, counts_ptr: int,
                                  q_stride: int = 3, t_stride: int = 3, stream: Optional[int] = None, **filter) -> None:
        """match_list_batched under the window gate (sift_hip_match_list_guided_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_guided_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P),
                                                        q_stride, t_stride, radius, ctypes.byref(f), out_ptr or None,
                                                        counts_ptr or None, stream), "match_list_guided_batched")

    def match_list_epipolar_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                                    nts: Sequence[int], positions: Sequence, geometry_ptr: int, max_error: float,
                                    out_ptr: int, counts_ptr: int, radius: float = float("inf"),
                                    geometry_stride: int = 52, q_stride: int = 3, t_stride: int = 3,
                                    stream: Optional[int] = None, **filter) -> None:
        """match_list_batched under the epipolar gate (sift_hip_match_list_epipolar_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_epipolar_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P),
                                                          q_stride, t_stride, radius, geometry_ptr or None,
                                                          geometry_stride, max_error, ctypes.byref(f), out_ptr or None,
                                                          counts_ptr or None, stream), "match_list_epipolar_batched")

    def match_list_guided_codes_batched(self, codes_ptr: int, keys_ptr: int, pairs: Sequence, positions: Sequence,
                                        radius: float, out_ptr: int, counts_ptr: int, q_stride: int = 3,
                                        t_stride: int = 3, stream: Optional[int] = None, **filter) -> None:
        """match_list_codes_batched under the window gate: pairs as multi.code_pairs, positions as
        multi.position_pairs return them (sift_hip_match_list_guided_codes_batched)."""
        P = len(pairs)
        qr, qk, nq, tr, tk, nt = ((ctypes.c_int * P)(*[p[k] for p in pairs]) for k in range(6))
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_guided_codes_batched(self._m, codes_ptr, keys_ptr, P, qr, qk, nq, tr, tk, nt,
                                                              self._positions(positions, P), q_stride, t_stride, radius,
                                                              ctypes.byref(f), out_ptr or None, counts_ptr or None,
                                                              stream), "match_list_guided_codes_batched")

    def match_list_epipolar_codes_batched(self, codes_ptr: int, keys_ptr: int, pairs: Sequence, positions: Sequence,
                                          geometry_ptr: int, max_error: float, out_ptr: int, counts_ptr: int,
                                          radius: float = float("inf"), geometry_stride: int = 52, q_stride: int = 3,
                                          t_stride: int = 3, stream: Optional[int] = None, **filter) -> None:
        """match_list_codes_batched under the epipolar gate (sift_hip_match_list_epipolar_codes_batched)."""
        P = len(pairs)
        qr, qk, nq, tr, tk, nt = ((ctypes.c_int * P)(*[p[k] for p in pairs]) for k in range(6))
        f = _match_filter(**filter)
        _check(lib().sift_hip_match_list_epipolar_codes_batched(self._m, codes_ptr, keys_ptr, P, qr, qk, nq, tr, tk, nt,
                                                                self._positions(positions, P), q_stride, t_stride,
                                                                radius, geometry_ptr or None, geometry_stride,
                                                                max_error, ctypes.byref(f), out_ptr or None,
                                                                counts_ptr or None, stream),
               "match_list_epipolar_codes_batched")

    # --- k nearest neighbours inside the two gates (the rule: include/sift_hip.h, "Gated k nearest neighbours"; in
    # numpy sift_amd.cv.guided_knn / epipolar_knn / mask_knn, the lists sift_amd.cv.knn_records of their tables).
    # Arguments as the gated top-2 calls above with k (and max_distance) in place of the ratio test; tables and lists
    # as match_knn_*.  The launch shape is knn_plan's.

    def match_knn_guided_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int,
                                radius: float, k: int, idx_ptr: int = 0, d2_ptr: int = 0, q_stride: int = 3,
                                t_stride: int = 3, stream: Optional[int] = None) -> None:
        """match_knn_device over each query's window candidates only (sift_hip_match_knn_guided_device)."""
        g = _MatchGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius)
        _check(lib().sift_hip_match_knn_guided_device(self._m, q_ptr or None, nq, t_ptr or None, nt, ctypes.byref(g), k,
                                                      idx_ptr or None, d2_ptr or None, stream), "match_knn_guided_device")

    def match_knn_epipolar_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, F,
                                  max_error: float, k: int, idx_ptr: int = 0, d2_ptr: int = 0,
                                  radius: float = float("inf"), q_stride: int = 3, t_stride: int = 3,
                                  stream: Optional[int] = None) -> None:
        """match_knn_device over each query's epipolar candidates only (sift_hip_match_knn_epipolar_device)."""
        g = _epipolar_gate(q_xy_ptr, q_stride, t_xy_ptr, t_stride, radius, F, max_error)
        _check(lib().sift_hip_match_knn_epipolar_device(self._m, q_ptr or None, nq, t_ptr or None, nt, ctypes.byref(g),
                                                        k, idx_ptr or None, d2_ptr or None, stream),
               "match_knn_epipolar_device")

    def match_knn_guided_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                                 nts: Sequence[int], positions: Sequence, radius: float, k: int, idx_ptr: int = 0,
                                 d2_ptr: int = 0, q_stride: int = 3, t_stride: int = 3,
                                 stream: Optional[int] = None) -> None:
        """match_knn_batched under the window gate (sift_hip_match_knn_guided_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        _check(lib().sift_hip_match_knn_guided_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P),
                                                       q_stride, t_stride, radius, k, idx_ptr or None, d2_ptr or None,
                                                       stream), "match_knn_guided_batched")

    def match_knn_epipolar_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                                   nts: Sequence[int], positions: Sequence, geometry_ptr: int, max_error: float, k: int,
                                   idx_ptr: int = 0, d2_ptr: int = 0, radius: float = float("inf"),
                                   geometry_stride: int = 52, q_stride: int = 3, t_stride: int = 3,
                                   stream: Optional[int] = None) -> None:
        """match_knn_batched under the epipolar gate, F read on the device (sift_hip_match_knn_epipolar_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        _check(lib().sift_hip_match_knn_epipolar_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P),
                                                         q_stride, t_stride, radius, geometry_ptr or None,
                                                         geometry_stride, max_error, k, idx_ptr or None, d2_ptr or None,
                                                         stream), "match_knn_epipolar_batched")

    def match_knn_list_guided_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int,
                                     radius: float, k: int, out_ptr: int, count_ptr: int, max_distance: float = 0.0,
                                     q_stride: int = 3, t_stride: int = 3, stream: Optional[int] = None) -> None:
        """match_knn_list_device under the window gate (sift_hip_match_knn_list_guided_device)."""
        g = _MatchGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius)
        _check(lib().sift_hip_match_knn_list_guided_device(self._m, q_ptr or None, nq, t_ptr or None, nt, ctypes.byref(g),
                                                           k, max_distance, out_ptr or None, count_ptr or None, stream),
               "match_knn_list_guided_device")

    def match_knn_list_epipolar_device(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, F,
                                       max_error: float, k: int, out_ptr: int, count_ptr: int,
                                       max_distance: float = 0.0, radius: float = float("inf"), q_stride: int = 3,
                                       t_stride: int = 3, stream: Optional[int] = None) -> None:
        """match_knn_list_device under the epipolar gate (sift_hip_match_knn_list_epipolar_device)."""
        g = _epipolar_gate(q_xy_ptr, q_stride, t_xy_ptr, t_stride, radius, F, max_error)
        _check(lib().sift_hip_match_knn_list_epipolar_device(self._m, q_ptr or None, nq, t_ptr or None, nt,
                                                             ctypes.byref(g), k, max_distance, out_ptr or None,
                                                             count_ptr or None, stream), "match_knn_list_epipolar_device")

    def match_knn_list_guided_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                                      nts: Sequence[int], positions: Sequence, radius: float, k: int, out_ptr: int,
                                      counts_ptr: int, max_distance: float = 0.0, q_stride: int = 3, t_stride: int = 3,
                                      stream: Optional[int] = None) -> None:
        """match_knn_list_batched under the window gate (sift_hip_match_knn_list_guided_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        _check(lib().sift_hip_match_knn_list_guided_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P),
                                                            q_stride, t_stride, radius, k, max_distance, out_ptr or None,
                                                            counts_ptr or None, stream), "match_knn_list_guided_batched")

    def match_knn_list_epipolar_batched(self, q_ptrs: Sequence[int], nqs: Sequence[int], t_ptrs: Sequence[int],
                                        nts: Sequence[int], positions: Sequence, geometry_ptr: int, max_error: float,
                                        k: int, out_ptr: int, counts_ptr: int, max_distance: float = 0.0,
                                        radius: float = float("inf"), geometry_stride: int = 52, q_stride: int = 3,
                                        t_stride: int = 3, stream: Optional[int] = None) -> None:
        """match_knn_list_batched under the epipolar gate (sift_hip_match_knn_list_epipolar_batched)."""
        P, qa, na, ta, ma = self._sets(q_ptrs, nqs, t_ptrs, nts)
        _check(lib().sift_hip_match_knn_list_epipolar_batched(self._m, P, qa, na, ta, ma, self._positions(positions, P),
                                                              q_stride, t_stride, radius, geometry_ptr or None,
                                                              geometry_stride, max_error, k, max_distance,
                                                              out_ptr or None, counts_ptr or None, stream),
               "match_knn_list_epipolar_batched")

    def match_knn_guided_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int,
                              radius: float, k: int, q_stride: int = 3, t_stride: int = 3):
        """Synchronous; (idx int32 (nq, k), d2 float32 (nq, k)) (sift_hip_match_knn_guided_host)."""
        idx = np.full((max(nq, 0), max(k, 0)), -1, np.int32)
        d2 = np.full((max(nq, 0), max(k, 0)), np.finfo(np.float32).max, np.float32)
        g = _MatchGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius)
        _check(lib().sift_hip_match_knn_guided_host(self._m, q_ptr or None, nq, t_ptr or None, nt, ctypes.byref(g), k,
                                                    _ptr(idx), _ptr(d2)), "match_knn_guided_host")
        return idx, d2

    def match_knn_epipolar_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, F,
                                max_error: float, k: int, radius: float = float("inf"), q_stride: int = 3,
                                t_stride: int = 3):
        """Synchronous; (idx int32 (nq, k), d2 float32 (nq, k)) (sift_hip_match_knn_epipolar_host)."""
        idx = np.full((max(nq, 0), max(k, 0)), -1, np.int32)
        d2 = np.full((max(nq, 0), max(k, 0)), np.finfo(np.float32).max, np.float32)
        g = _epipolar_gate(q_xy_ptr, q_stride, t_xy_ptr, t_stride, radius, F, max_error)
        _check(lib().sift_hip_match_knn_epipolar_host(self._m, q_ptr or None, nq, t_ptr or None, nt, ctypes.byref(g), k,
                                                      _ptr(idx), _ptr(d2)), "match_knn_epipolar_host")
        return idx, d2

    def match_knn_list_guided_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int,
                                   radius: float, k: int, max_distance: float = 0.0, q_stride: int = 3,
                                   t_stride: int = 3) -> np.ndarray:
        """Synchronous; the kept records as a DMATCH_DTYPE array (sift_hip_match_knn_list_guided_host)."""
        out = np.zeros(max(nq, 0) * max(k, 0), DMATCH_DTYPE)
        g = _MatchGate(q_xy_ptr or None, q_stride, t_xy_ptr or None, t_stride, radius)
        n = ctypes.c_int(0)
        _check(lib().sift_hip_match_knn_list_guided_host(self._m, q_ptr or None, nq, t_ptr or None, nt, ctypes.byref(g),
                                                         k, max_distance, _ptr(out), len(out), ctypes.byref(n)),
               "match_knn_list_guided_host")
        return out[: n.value]

    def match_knn_list_epipolar_host(self, q_ptr: int, nq: int, t_ptr: int, nt: int, q_xy_ptr: int, t_xy_ptr: int, F,
                                     max_error: float, k: int, max_distance: float = 0.0, radius: float = float("inf"),
                                     q_stride: int = 3, t_stride: int = 3) -> np.ndarray:
        """Synchronous; the kept records as a DMATCH_DTYPE array (sift_hip_match_knn_list_epipolar_host)."""
        out = np.zeros(max(nq, 0) * max(k, 0), DMATCH_DTYPE)
        g = _epipolar_gate(q_xy_ptr, q_stride, t_xy_ptr, t_stride, radius, F, max_error)
        n = ctypes.c_int(0)
        _check(lib().sift_hip_match_knn_list_epipolar_host(self._m, q_ptr or None, nq, t_ptr or None, nt,
                                                           ctypes.byref(g), k, max_distance, _ptr(out), len(out),
                                                           ctypes.byref(n)), "match_knn_list_epipolar_host")
        return out[: n.value]


_default_matcher: Optional[Matcher] = None


def matchList(des: "DeviceBuffer", num_des: int, src: "DeviceBuffer", num_src: int, **filter) -> np.ndarray:
    """The usable match list of des against src in one device operation: DMATCH_DTYPE records (queryIdx, trainIdx,
    imgIdx 0, L2 distance) of the rows that pass the filter -- by default Lowe's ratio 0.8 on distances and the cross
    check of cv::BFMatcher(NORM_L2, crossCheck=True) -- in ascending queryIdx.  `filter` keywords as
    Matcher.match_list_*; the rule is sift_amd.cv.filter_matches."""
    m = _list_matcher(num_des, num_src)
    if num_des <= 0 or num_src <= 0:
        return np.zeros(0, DMATCH_DTYPE)
    return m.match_list_host(des.data(), num_des, src.data(), num_src, **filter)


def _list_matcher(num_des: int, num_src: int) -> Matcher:
    global _default_matcher
    need = max(num_des, num_src, 1)  # the reverse direction swaps the roles: both limits hold both sets
    if (_default_matcher is None or need > min(_default_matcher.max_query, _default_matcher.max_train)
            or _default_matcher.max_pairs < 2):
        cap = max(need, _default_matcher.max_query if _default_matcher else 0,
                  _default_matcher.max_train if _default_matcher else 0)
        # two pairs: foreign buffers match both directions in one launch (detector buffers use their sidecars)
        _default_matcher = Matcher(cap, cap, max_pairs=2)
    return _default_matcher


def knnMatch(des: "DeviceBuffer", num_des: int, src: "DeviceBuffer", num_src: int, k: int):
    """cv::BFMatcher::knnMatch(des, src, k) as arrays: (idx int32 (num_des, k), d2 float32 (num_des, k)), the k
    nearest rows of src for every row of des in ascending (squared distance, index) order, -1 / FLT_MAX where src has
    fewer than k rows (1 <= k <= KNN_MAX; the rule is sift_amd.cv.knn)."""
    m = _list_matcher(num_des, num_src)
    return m.match_knn_host(des.data(), num_des, src.data(), num_src, k)


def matchKnnList(des: "DeviceBuffer", num_des: int, src: "DeviceBuffer", num_src: int, k: int,
                 max_distance: float = 0.0) -> np.ndarray:
    """cv::BFMatcher::radiusMatch capped at k per query: DMATCH_DTYPE records (queryIdx, trainIdx, imgIdx 0, L2
    distance) of the k nearest rows of src within max_distance (<= 0: no cap) of every row of des, in (queryIdx,
    rank) order -- the candidates a verifier chooses among (the rule is sift_amd.cv.knn_records)."""
    m = _list_matcher(num_des, num_src)
    return m.match_knn_list_host(des.data(), num_des, src.data(), num_src, k, max_distance)


def _xy_ptrs(des_xy, src_xy):
    return tuple(p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))


def knnMatchGuided(des: "DeviceBuffer", num_des: int, des_xy, src: "DeviceBuffer", num_src: int, src_xy, radius: float,
                   k: int, des_stride: int = 3, src_stride: int = 3):
    """knnMatch inside a search window -- cv::DescriptorMatcher::knnMatch(des, src, k, mask) with the window of
    matchListGuided as the mask: (idx, d2) as knnMatch returns them, the k nearest candidates of every row of des
    (the rule: sift_amd.cv.guided_knn).  des_xy / src_xy as matchListGuided."""
    m = _list_matcher(num_des, num_src)
    qxy, txy = _xy_ptrs(des_xy, src_xy)
    return m.match_knn_guided_host(des.data(), num_des, src.data(), num_src, qxy, txy, radius, k, des_stride, src_stride)


def knnMatchEpipolar(des: "DeviceBuffer", num_des: int, des_xy, src: "DeviceBuffer", num_src: int, src_xy, F,
                     max_error: float, k: int, radius: float = float("inf"), des_stride: int = 3, src_stride: int = 3):
    """knnMatch under a fundamental matrix: the k nearest rows of src inside the epipolar band of every row of des
    (F, max_error and radius as matchListEpipolar; the rule: sift_amd.cv.epipolar_knn)."""
    m = _list_matcher(num_des, num_src)
    qxy, txy = _xy_ptrs(des_xy, src_xy)
    return m.match_knn_epipolar_host(des.data(), num_des, src.data(), num_src, qxy, txy, F, max_error, k, radius,
                                     des_stride, src_stride)


def matchKnnListGuided(des: "DeviceBuffer", num_des: int, des_xy, src: "DeviceBuffer", num_src: int, src_xy,
                       radius: float, k: int, max_distance: float = 0.0, des_stride: int = 3,
                       src_stride: int = 3) -> np.ndarray:
    """matchKnnList inside a search window: the records of knnMatchGuided's table within max_distance (<= 0: no cap),
    in (queryIdx, rank) order (the rule: sift_amd.cv.knn_records of sift_amd.cv.guided_knn)."""
    m = _list_matcher(num_des, num_src)
    qxy, txy = _xy_ptrs(des_xy, src_xy)
    return m.match_knn_list_guided_host(des.data(), num_des, src.data(), num_src, qxy, txy, radius, k, max_distance,
                                        des_stride, src_stride)


def matchKnnListEpipolar(des: "DeviceBuffer", num_des: int, des_xy, src: "DeviceBuffer", num_src: int, src_xy, F,
                         max_error: float, k: int, max_distance: float = 0.0, radius: float = float("inf"),
                         des_stride: int = 3, src_stride: int = 3) -> np.ndarray:
    """matchKnnList under a fundamental matrix: the records of knnMatchEpipolar's table within max_distance."""
    m = _list_matcher(num_des, num_src)
    qxy, txy = _xy_ptrs(des_xy, src_xy)
    return m.match_knn_list_epipolar_host(des.data(), num_des, src.data(), num_src, qxy, txy, F, max_error, k,
                                          max_distance, radius, des_stride, src_stride)


def matchListGuided(des: "DeviceBuffer", num_des: int, des_xy, src: "DeviceBuffer", num_src: int, src_xy, radius: float,
                    des_stride: int = 3, src_stride: int = 3, **filter) -> np.ndarray:
    """matchList inside a search window: row t of src is a candidate of row i of des when both coordinates of their
    positions differ by at most `radius` pixels (the rule: sift_amd.cv.gate_mask), and the top-2 search of both
    directions, the ratio test and the cross check see candidates only.  des_xy / src_xy: DeviceBuffers or raw device
    pointers of float rows with x, y first -- det.device_kpts (stride 3) for a detector's current frame, the
    previous frame's positions or the caller's predictions for the other side.  `filter` keywords as matchList."""
    m = _list_matcher(num_des, num_src)
    if num_des <= 0 or num_src <= 0:
        return np.zeros(0, DMATCH_DTYPE)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    return m.match_list_guided_host(des.data(), num_des, src.data(), num_src, qxy, txy, radius, des_stride, src_stride,
                                    **filter)


def matchListEpipolar(des: "DeviceBuffer", num_des: int, des_xy, src: "DeviceBuffer", num_src: int, src_xy, F,
                      max_error: float, radius: float = float("inf"), des_stride: int = 3, src_stride: int = 3,
                      **filter) -> np.ndarray:
    """matchList under a fundamental matrix: row t of src is a candidate of row i of des when it lies within
    `max_error` pixels (Sampson distance) of i's epipolar line under F -- 9 floats, row-major, x_src^T F x_des = 0,
    what cv.findFundamentalMat(des_points, src_points) returns -- and inside the window `radius` when that is finite
    (the rule: sift_amd.cv.epipolar_mask).  The top-2 search of both directions, the ratio test and the cross check
    see candidates only.  des_xy / src_xy and the `filter` keywords as matchListGuided."""
    m = _list_matcher(num_des, num_src)
    if num_des <= 0 or num_src <= 0:
        return np.zeros(0, DMATCH_DTYPE)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    return m.match_list_epipolar_host(des.data(), num_des, src.data(), num_src, qxy, txy, F, max_error, radius,
                                      des_stride, src_stride, **filter)


class Verifier:
    """Two-view verification of a match list on the device: a fixed-budget RANSAC for the fundamental matrix or the
    homography (sift_hip_verifier_*; the rules: include/sift_hip.h, and in numpy sift_amd.cv.ransac_fundamental /
    ransac_homography).  Owns all scratch of its calls -- for lists of up to max_matches records and up to
    max_hypotheses hypotheses -- so a device call only launches kernels.  Calls on one verifier must be ordered."""

    def __init__(self, max_matches: int, max_hypotheses: int = 1024, max_pairs: int = 1, device: int = -1,
                 essential_samples: int = 0):
        """max_pairs > 1: a verifier for the batched calls (sift_hip_verifier_create_batched) of up to max_pairs pairs
        whose caps sum to at most max_matches (up to 64 x 65536).  essential_samples > 0: the scratch of the essential
        calls for up to that many samples (sift_hip_verifier_reserve_essential), ten model slots each."""
        self._v = ctypes.c_void_p()
        if max_pairs == 1:
            _check(lib().sift_hip_verifier_create(device, max_matches, max_hypotheses, ctypes.byref(self._v)),
                   "verifier_create")
        else:
            _check(lib().sift_hip_verifier_create_batched(device, max_matches, max_hypotheses, max_pairs,
                                                          ctypes.byref(self._v)), "verifier_create_batched")
        self.max_matches, self.max_hypotheses, self.max_pairs = max_matches, max_hypotheses, max_pairs
        self._hypotheses = 0
        self._h_hypotheses = 0
        self._a_hypotheses = 0
        self._e_hypotheses = 0
        self.essential_samples = 0
        if essential_samples:
            self.reserve_essential(essential_samples)

    def reserve_essential(self, max_samples: int) -> None:
        """sift_hip_verifier_reserve_essential: allocates, once, what essential calls of up to max_samples (1..4096)
        samples need for the verifier's max_pairs.  Not capturable; the essential calls after it are."""
        _check(lib().sift_hip_verifier_reserve_essential(self._v, max_samples), "verifier_reserve_essential")
        self.essential_samples = max_samples

    def __del__(self):
        v = getattr(self, "_v", None)
        if v is not None and v.value and _lib is not None:
            _lib.sift_hip_verifier_destroy(v)
            self._v = None

    # --- one pair (sift_hip_verify_*_device / _host, sift_hip_score_*_device): the two models' methods differ in the
    # entry point and the record type only.

    def _device(self, fn, what, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, out_ptr,
                out_count_ptr, mask_ptr, max_error, hypotheses, seed, q_stride, t_stride, stream):
        p = _VerifyParams(hypotheses, seed, max_error)
        _check(fn(self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None,
                  t_stride, nt, ctypes.byref(p), result_ptr or None, out_ptr or None, out_count_ptr or None,
                  mask_ptr or None, stream), what)

    def _host(self, fn, what, record, dtype, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, max_error, hypotheses, seed,
              q_stride, t_stride, full):
        p = _VerifyParams(hypotheses, seed, max_error)
        r = record()
        out = np.zeros(max(cap, 0), DMATCH_DTYPE)
        mask = np.zeros(max(cap, 0), np.uint8)
        _check(fn(self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None,
                  t_stride, nt, ctypes.byref(p), ctypes.byref(r), _ptr(out), _ptr(mask)), what)
        if full:
            return np.frombuffer(bytes(r), dtype)[0], out[: r.inliers], mask
        return np.array(getattr(r, dtype.names[0]), np.float32).reshape(3, 3), out[: r.inliers], r.hypothesis

    def _score(self, fn, what, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, M_ptr, K, max_error, counts_ptr,
               q_stride, t_stride, stream):
        _check(fn(self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None,
                  t_stride, nt, M_ptr or None, K, max_error, counts_ptr or None, stream), what)

    def verify_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int, nt: int,
                      result_ptr: int, out_ptr: int = 0, out_count_ptr: int = 0, mask_ptr: int = 0,
                      max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, q_stride: int = 3,
                      t_stride: int = 3, stream: Optional[int] = None) -> None:
        """Enqueue the operation (sift_hip_verify_fundamental_device); every pointer is device memory.  count_ptr: the
        device int holding the number of records (0: all `cap` count) -- e.g. match_list_device's count; result_ptr: a
        VERIFY_RESULT_DTYPE record; out_ptr (room for cap records), out_count_ptr and mask_ptr (cap bytes) may be 0."""
        self._device(lib().sift_hip_verify_fundamental_device, "verify_fundamental_device", matches_ptr, count_ptr, cap,
                     q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, out_ptr, out_count_ptr, mask_ptr, max_error, hypotheses, seed,
                     q_stride, t_stride, stream)
        self._hypotheses = hypotheses

    def verify_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int, nt: int,
                    max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, q_stride: int = 3,
                    t_stride: int = 3, full: bool = False):
        """Synchronous (sift_hip_verify_fundamental_host): (F 3 x 3 float32, the inlier records as a DMATCH_DTYPE array,
        the winning hypothesis or -1).  full: (the VERIFY_RESULT_DTYPE record, the records, the mask of cap bytes)."""
        got = self._host(lib().sift_hip_verify_fundamental_host, "verify_fundamental_host", _VerifyResult,
                         VERIFY_RESULT_DTYPE, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, max_error,
                         hypotheses, seed, q_stride, t_stride, full)
        self._hypotheses = hypotheses
        return got

    def score_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int, nt: int,
                     F_ptr: int, K: int, max_error: float, counts_ptr: int, q_stride: int = 3, t_stride: int = 3,
                     stream: Optional[int] = None) -> None:
        """The score alone on the caller's K hypotheses (device, K x 9 floats): counts (device, K ints)."""
        self._score(lib().sift_hip_score_fundamental_device, "score_fundamental_device", matches_ptr, count_ptr, cap,
                    q_xy_ptr, nq, t_xy_ptr, nt, F_ptr, K, max_error, counts_ptr, q_stride, t_stride, stream)

    def hypotheses(self):
        """What the last verify call drew, solved and counted: (samples (K, 8) int32, F (K, 9) float32, valid (K,) bool
        -- an invalid hypothesis has F all zero --, counts (K,) int32).  Synchronises the device."""
        K = self._hypotheses
        samples, F, counts = np.zeros((K, 8), np.int32), np.zeros((K, 9), np.float32), np.zeros(K, np.int32)
        _check(lib().sift_hip_verify_hypotheses_host(self._v, _ptr(samples), _ptr(F), _ptr(counts), K),
               "verify_hypotheses_host")
        return samples, F, F.any(1), counts

    def verify_homography_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                                 nt: int, result_ptr: int, out_ptr: int = 0, out_count_ptr: int = 0, mask_ptr: int = 0,
                                 max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, q_stride: int = 3,
                                 t_stride: int = 3, stream: Optional[int] = None) -> None:
        """verify_device for the homography (sift_hip_verify_homography_device), argument for argument; result_ptr: a
        HOMOGRAPHY_RESULT_DTYPE record, whose address is also the H project_homography_device takes; max_error: the
        transfer error in pixels."""
        self._device(lib().sift_hip_verify_homography_device, "verify_homography_device", matches_ptr, count_ptr, cap,
                     q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, out_ptr, out_count_ptr, mask_ptr, max_error, hypotheses, seed,
                     q_stride, t_stride, stream)
        self._h_hypotheses = hypotheses

    def verify_homography_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                               nt: int, max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, q_stride: int = 3,
                               t_stride: int = 3, full: bool = False):
        """Synchronous (sift_hip_verify_homography_host): (H 3 x 3 float32 of unit norm, the inlier records as a
        DMATCH_DTYPE array, the winning hypothesis or -1).  full: (the HOMOGRAPHY_RESULT_DTYPE record, the records, the
        mask of cap bytes)."""
        got = self._host(lib().sift_hip_verify_homography_host, "verify_homography_host", _HomographyResult,
                         HOMOGRAPHY_RESULT_DTYPE, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, max_error,
                         hypotheses, seed, q_stride, t_stride, full)
        self._h_hypotheses = hypotheses
        return got

    def score_homography_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                                nt: int, H_ptr: int, K: int, max_error: float, counts_ptr: int, q_stride: int = 3,
                                t_stride: int = 3, stream: Optional[int] = None) -> None:
        """The transfer-error score alone on the caller's K homographies (device, K x 9 floats): counts (device, K
        ints)."""
        self._score(lib().sift_hip_score_homography_device, "score_homography_device", matches_ptr, count_ptr, cap,
                    q_xy_ptr, nq, t_xy_ptr, nt, H_ptr, K, max_error, counts_ptr, q_stride, t_stride, stream)

    def homography_hypotheses(self):
        """What the last verify call drew, solved and counted, when it was a homography call: (samples (K, 4) int32, H
        (K, 9) float32, valid (K,) bool -- an invalid hypothesis has H all zero --, counts (K,) int32).  Synchronises
        the device."""
        K = self._h_hypotheses
        samples, H, counts = np.zeros((K, 4), np.int32), np.zeros((K, 9), np.float32), np.zeros(K, np.int32)
        _check(lib().sift_hip_verify_homography_hypotheses_host(self._v, _ptr(samples), _ptr(H), _ptr(counts), K),
               "verify_homography_hypotheses_host")
        return samples, H, H.any(1), counts

    # --- all pairs of a batch in one pass (sift_hip_verify_*_batched_*).  pairs: (q_xy_ptr, nq, t_xy_ptr, nt) -- as
    # sift_amd.multi.position_pairs returns them -- or (q_xy_ptr, nq, t_xy_ptr, nt, cap); cap, the pair's rows in the
    # matches, out and mask arrays, defaults to nq, which is Matcher.match_list_batched's layout.  Pair p's rows
    # start at the sum of the caps before it, and its outputs are the single call's with seed + p.

    @staticmethod
    def _pairs(pairs: Sequence):
        rec = [(p[0] or None, p[2] or None, p[1], p[3], p[4] if len(p) > 4 else p[1]) for p in pairs]
        return (_VerifyPair * max(len(rec), 1))(*[_VerifyPair(*r) for r in rec]), [r[4] for r in rec]

    def _batched_device(self, fn, what, matches_ptr, counts_ptr, pairs, results_ptr, out_ptr, out_counts_ptr, mask_ptr,
                        max_error, hypotheses, seed, q_stride, t_stride, stream):
        p = _VerifyParams(hypotheses, seed & 0xFFFFFFFF, max_error)
        table, _ = self._pairs(pairs)
        _check(fn(self._v, matches_ptr or None, counts_ptr or None, len(pairs), table, q_stride, t_stride, ctypes.byref(p),
                  results_ptr or None, out_ptr or None, out_counts_ptr or None, mask_ptr or None, stream), what)

    def verify_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int,
                              out_ptr: int = 0, out_counts_ptr: int = 0, mask_ptr: int = 0, max_error: float = 1.5,
                              hypotheses: int = 1024, seed: int = 0, q_stride: int = 3, t_stride: int = 3,
                              stream: Optional[int] = None) -> None:
        """Enqueue the fundamental-matrix verification of every pair (sift_hip_verify_fundamental_batched_device);
        every pointer is device memory.  counts_ptr: len(pairs) device ints (0: every pair counts its cap) -- e.g.
        match_list_batched's counts; results_ptr: len(pairs) VERIFY_RESULT_DTYPE records; out_ptr and mask_ptr (the
        caps' sum rows / bytes) and out_counts_ptr (len(pairs) ints) may be 0."""
        self._batched_device(lib().sift_hip_verify_fundamental_batched_device, "verify_fundamental_batched_device",
                             matches_ptr, counts_ptr, pairs, results_ptr, out_ptr, out_counts_ptr, mask_ptr, max_error,
                             hypotheses, seed, q_stride, t_stride, stream)

    def verify_homography_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int,
                                         out_ptr: int = 0, out_counts_ptr: int = 0, mask_ptr: int = 0,
                                         max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0,
                                         q_stride: int = 3, t_stride: int = 3, stream: Optional[int] = None) -> None:
        """verify_batched_device for the homography (sift_hip_verify_homography_batched_device); results_ptr:
        HOMOGRAPHY_RESULT_DTYPE records."""
        self._batched_device(lib().sift_hip_verify_homography_batched_device, "verify_homography_batched_device",
                             matches_ptr, counts_ptr, pairs, results_ptr, out_ptr, out_counts_ptr, mask_ptr, max_error,
                             hypotheses, seed, q_stride, t_stride, stream)

    def _batched_host(self, fn, what, dtype, matches_ptr, counts_ptr, pairs, max_error, hypotheses, seed, q_stride,
                      t_stride, full):
        p = _VerifyParams(hypotheses, seed & 0xFFFFFFFF, max_error)
        table, caps = self._pairs(pairs)
        rows = sum(c for c in caps if 0 <= c <= 65536)
        res = np.zeros(max(len(pairs), 1), dtype)
        out, mask = np.zeros(rows, DMATCH_DTYPE), np.zeros(rows, np.uint8)
        _check(fn(self._v, matches_ptr or None, counts_ptr or None, len(pairs), table, q_stride, t_stride, ctypes.byref(p),
                  _ptr(res), _ptr(out), _ptr(mask)), what)
        row0 = np.concatenate([[0], np.cumsum(caps)]).astype(int)
        model = dtype.names[0]
        got = []
        for i, r in enumerate(res[:len(pairs)]):
            recs = out[row0[i]: row0[i] + r["inliers"]].copy()
            if full:
                got.append((r.copy(), recs, mask[row0[i]: row0[i + 1]].copy()))
            else:
                got.append((r[model].reshape(3, 3).copy(), recs, int(r["hypothesis"])))
        return got

    def verify_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, max_error: float = 1.5,
                            hypotheses: int = 1024, seed: int = 0, q_stride: int = 3, t_stride: int = 3,
                            full: bool = False) -> list:
        """Synchronous (sift_hip_verify_fundamental_batched_host): per pair what verify_host returns -- (F, the inlier
        records, the winning hypothesis or -1), or with full (the VERIFY_RESULT_DTYPE record, the records, the pair's
        mask of cap bytes)."""
        return self._batched_host(lib().sift_hip_verify_fundamental_batched_host, "verify_fundamental_batched_host",
                                  VERIFY_RESULT_DTYPE, matches_ptr, counts_ptr, pairs, max_error, hypotheses, seed,
                                  q_stride, t_stride, full)

    def verify_homography_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, max_error: float = 1.5,
                                       hypotheses: int = 1024, seed: int = 0, q_stride: int = 3, t_stride: int = 3,
                                       full: bool = False) -> list:
        """verify_batched_host for the homography (sift_hip_verify_homography_batched_host)."""
        return self._batched_host(lib().sift_hip_verify_homography_batched_host, "verify_homography_batched_host",
                                  HOMOGRAPHY_RESULT_DTYPE, matches_ptr, counts_ptr, pairs, max_error, hypotheses, seed,
                                  q_stride, t_stride, full)

    # --- the refit of a verified model on its inliers (sift_hip_refine_*; the rule: include/sift_hip.h, in numpy
    # sift_amd.cv.refine_fundamental / refine_homography).  The list, count, cap and positions are the verify call's;
    # result(s) and mask are what it wrote, updated in place.

    def _refine_device(self, fn, what, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, mask_ptr,
                       out_ptr, out_count_ptr, accepted_ptr, max_error, rounds, q_stride, t_stride, stream):
        _check(fn(self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None,
                  t_stride, nt, max_error, rounds, result_ptr or None, mask_ptr or None, out_ptr or None,
                  out_count_ptr or None, accepted_ptr or None, stream), what)

    def refine_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int, nt: int,
                      result_ptr: int, mask_ptr: int, out_ptr: int = 0, out_count_ptr: int = 0, accepted_ptr: int = 0,
                      max_error: float = 1.5, rounds: int = 1, q_stride: int = 3, t_stride: int = 3,
                      stream: Optional[int] = None) -> None:
        """Enqueue `rounds` (1..8) refit rounds of the fundamental matrix (sift_hip_refine_fundamental_device); every
        pointer is device memory.  result_ptr and mask_ptr: the record and the mask of verify_device on the same list,
        updated in place; out_ptr (room for cap records), out_count_ptr and accepted_ptr (an int: the number of
        accepted rounds) may be 0."""
        self._refine_device(lib().sift_hip_refine_fundamental_device, "refine_fundamental_device", matches_ptr,
                            count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, mask_ptr, out_ptr, out_count_ptr,
                            accepted_ptr, max_error, rounds, q_stride, t_stride, stream)

    def refine_homography_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                                 nt: int, result_ptr: int, mask_ptr: int, out_ptr: int = 0, out_count_ptr: int = 0,
                                 accepted_ptr: int = 0, max_error: float = 1.5, rounds: int = 1, q_stride: int = 3,
                                 t_stride: int = 3, stream: Optional[int] = None) -> None:
        """refine_device for the homography (sift_hip_refine_homography_device)."""
        self._refine_device(lib().sift_hip_refine_homography_device, "refine_homography_device", matches_ptr, count_ptr,
                            cap, q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, mask_ptr, out_ptr, out_count_ptr, accepted_ptr,
                            max_error, rounds, q_stride, t_stride, stream)

    def _refine_host(self, fn, what, dtype, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result, mask,
                     max_error, rounds, q_stride, t_stride):
        res = np.array([result], dtype)  # copies: the caller's record and mask are not changed
        mask = np.array(np.asarray(mask, np.uint8).reshape(-1), np.uint8)
        if len(mask) != max(cap, 0):
            raise ValueError("one mask byte per row of the list (cap)")
        out = np.zeros(max(cap, 0), DMATCH_DTYPE)
        n_out, accepted = ctypes.c_int(0), ctypes.c_int(0)
        _check(fn(self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None,
                  t_stride, nt, max_error, rounds, _ptr(res), _ptr(mask) if cap > 0 else None, _ptr(out),
                  ctypes.byref(n_out), ctypes.byref(accepted)), what)
        return res[0], out[: n_out.value], mask, accepted.value

    def refine_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int, nt: int,
                    result, mask, max_error: float = 1.5, rounds: int = 1, q_stride: int = 3, t_stride: int = 3):
        """Synchronous (sift_hip_refine_fundamental_host): result (a VERIFY_RESULT_DTYPE record) and mask (cap bytes)
        are host values as verify_host(full=True) returns them; the list and positions are device memory.  Returns
        (the updated record, the inlier records, the updated mask, the number of accepted rounds)."""
        return self._refine_host(lib().sift_hip_refine_fundamental_host, "refine_fundamental_host", VERIFY_RESULT_DTYPE,
                                 matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result, mask, max_error, rounds,
                                 q_stride, t_stride)

    def refine_homography_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                               nt: int, result, mask, max_error: float = 1.5, rounds: int = 1, q_stride: int = 3,
                               t_stride: int = 3):
        """refine_host for the homography (sift_hip_refine_homography_host; a HOMOGRAPHY_RESULT_DTYPE record)."""
        return self._refine_host(lib().sift_hip_refine_homography_host, "refine_homography_host",
                                 HOMOGRAPHY_RESULT_DTYPE, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result,
                                 mask, max_error, rounds, q_stride, t_stride)

    def _refine_batched_device(self, fn, what, matches_ptr, counts_ptr, pairs, results_ptr, mask_ptr, out_ptr,
                               out_counts_ptr, accepted_ptr, max_error, rounds, q_stride, t_stride, stream):
        table, _ = self._pairs(pairs)
        _check(fn(self._v, matches_ptr or None, counts_ptr or None, len(pairs), table, q_stride, t_stride, max_error,
                  rounds, results_ptr or None, mask_ptr or None, out_ptr or None, out_counts_ptr or None,
                  accepted_ptr or None, stream), what)

    def refine_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int, mask_ptr: int,
                              out_ptr: int = 0, out_counts_ptr: int = 0, accepted_ptr: int = 0, max_error: float = 1.5,
                              rounds: int = 1, q_stride: int = 3, t_stride: int = 3,
                              stream: Optional[int] = None) -> None:
        """Enqueue the refit of every pair (sift_hip_refine_fundamental_batched_device) on what verify_batched_device
        wrote: results_ptr (len(pairs) records) and mask_ptr (the caps' sum bytes) are updated in place; out_ptr,
        out_counts_ptr and accepted_ptr (len(pairs) ints each) may be 0.  Pair p's bytes are the single call's."""
        self._refine_batched_device(lib().sift_hip_refine_fundamental_batched_device, "refine_fundamental_batched_device",
                                    matches_ptr, counts_ptr, pairs, results_ptr, mask_ptr, out_ptr, out_counts_ptr,
                                    accepted_ptr, max_error, rounds, q_stride, t_stride, stream)

    def refine_homography_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int,
                                         mask_ptr: int, out_ptr: int = 0, out_counts_ptr: int = 0, accepted_ptr: int = 0,
                                         max_error: float = 1.5, rounds: int = 1, q_stride: int = 3, t_stride: int = 3,
                                         stream: Optional[int] = None) -> None:
        """refine_batched_device for the homography (sift_hip_refine_homography_batched_device)."""
        self._refine_batched_device(lib().sift_hip_refine_homography_batched_device, "refine_homography_batched_device",
                                    matches_ptr, counts_ptr, pairs, results_ptr, mask_ptr, out_ptr, out_counts_ptr,
                                    accepted_ptr, max_error, rounds, q_stride, t_stride, stream)

    def _refine_batched_host(self, fn, what, dtype, matches_ptr, counts_ptr, pairs, verified, max_error, rounds, q_stride,
                             t_stride):
        table, caps = self._pairs(pairs)
        if len(verified) != len(pairs):
            raise ValueError("one verified (record, records, mask) per pair")
        row0 = np.concatenate([[0], np.cumsum([c if 0 <= c <= 65536 else 0 for c in caps])]).astype(int)
        res = np.array([v[0] for v in verified], dtype) if len(pairs) else np.zeros(1, dtype)
        mask = np.zeros(row0[-1], np.uint8)
        for i, v in enumerate(verified):
            mask[row0[i]: row0[i + 1]] = np.asarray(v[2], np.uint8).reshape(-1)
        out = np.zeros(row0[-1], DMATCH_DTYPE)
        n_out, accepted = np.zeros(max(len(pairs), 1), np.int32), np.zeros(max(len(pairs), 1), np.int32)
        _check(fn(self._v, matches_ptr or None, counts_ptr or None, len(pairs), table, q_stride, t_stride, max_error,
                  rounds, _ptr(res), _ptr(mask) if len(mask) else None, _ptr(out), _ptr(n_out), _ptr(accepted)), what)
        return [(res[i].copy(), out[row0[i]: row0[i] + n_out[i]].copy(), mask[row0[i]: row0[i + 1]].copy(),
                 int(accepted[i])) for i in range(len(pairs))]

    def refine_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, verified: Sequence,
                            max_error: float = 1.5, rounds: int = 1, q_stride: int = 3, t_stride: int = 3) -> list:
        """Synchronous (sift_hip_refine_fundamental_batched_host): verified is verify_batched_host(full=True)'s list of
        (record, records, mask); per pair what refine_host returns."""
        return self._refine_batched_host(lib().sift_hip_refine_fundamental_batched_host, "refine_fundamental_batched_host",
                                         VERIFY_RESULT_DTYPE, matches_ptr, counts_ptr, pairs, verified, max_error, rounds,
                                         q_stride, t_stride)

    def refine_homography_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, verified: Sequence,
                                       max_error: float = 1.5, rounds: int = 1, q_stride: int = 3,
                                       t_stride: int = 3) -> list:
        """refine_batched_host for the homography (sift_hip_refine_homography_batched_host)."""
        return self._refine_batched_host(lib().sift_hip_refine_homography_batched_host, "refine_homography_batched_host",
                                         HOMOGRAPHY_RESULT_DTYPE, matches_ptr, counts_ptr, pairs, verified, max_error,
                                         rounds, q_stride, t_stride)

    # --- the affine map and the similarity (sift_hip_verify_affine_* / sift_hip_refine_affine_*; the rule:
    # include/sift_hip.h, in numpy sift_amd.cv.ransac_affine / refine_affine).  The homography methods argument for
    # argument, with similarity choosing the 4-degree-of-freedom model (2-point samples) over the affine map (3-point
    # samples); the record is the homography's, H = {a, b, tx, c, d, ty, 0, 0, 1}, so project_homography_device and the
    # window-gated matchers take it as it lies.

    @staticmethod
    def _affine(fn, similarity):
        """fn with the model argument, which follows the handle, bound."""
        model = MODEL_SIMILARITY if similarity else MODEL_AFFINE
        return lambda v, *args: fn(v, model, *args)

    def verify_affine_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                             nt: int, result_ptr: int, out_ptr: int = 0, out_count_ptr: int = 0, mask_ptr: int = 0,
                             max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, q_stride: int = 3,
                             t_stride: int = 3, stream: Optional[int] = None, similarity: bool = False) -> None:
        """verify_homography_device for the affine map or the similarity (sift_hip_verify_affine_device); result_ptr:
        an AFFINE_RESULT_DTYPE record."""
        self._device(self._affine(lib().sift_hip_verify_affine_device, similarity), "verify_affine_device", matches_ptr,
                     count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, out_ptr, out_count_ptr, mask_ptr, max_error,
                     hypotheses, seed, q_stride, t_stride, stream)
        self._a_hypotheses = hypotheses

    def verify_affine_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                           nt: int, max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, q_stride: int = 3,
                           t_stride: int = 3, full: bool = False, similarity: bool = False):
        """Synchronous (sift_hip_verify_affine_host): (A 3 x 3 float32 with the last row 0 0 1, the inlier records as a
        DMATCH_DTYPE array, the winning hypothesis or -1).  full: (the AFFINE_RESULT_DTYPE record, the records, the
        mask of cap bytes)."""
        got = self._host(self._affine(lib().sift_hip_verify_affine_host, similarity), "verify_affine_host",
                         _HomographyResult, AFFINE_RESULT_DTYPE, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt,
                         max_error, hypotheses, seed, q_stride, t_stride, full)
        self._a_hypotheses = hypotheses
        return got

    def score_affine_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                            nt: int, A_ptr: int, K: int, max_error: float, counts_ptr: int, q_stride: int = 3,
                            t_stride: int = 3, stream: Optional[int] = None, similarity: bool = False) -> None:
        """The affine score alone on the caller's K models (device, K x 9 floats, the last row 0 0 1): counts (device,
        K ints).  The predicate is both models' own: similarity changes nothing."""
        self._score(lib().sift_hip_score_affine_device, "score_affine_device", matches_ptr, count_ptr, cap, q_xy_ptr, nq,
                    t_xy_ptr, nt, A_ptr, K, max_error, counts_ptr, q_stride, t_stride, stream)

    def affine_hypotheses(self, similarity: bool = False):
        """What the last verify call drew, solved and counted, when it was a call of this model: (samples (K, 3) --
        similarity: (K, 2) -- int32, A (K, 9) float32, valid (K,) bool -- an invalid hypothesis has A all zero --,
        counts (K,) int32).  Synchronises the device."""
        K, m = self._a_hypotheses, 2 if similarity else 3
        samples, A, counts = np.zeros((K, m), np.int32), np.zeros((K, 9), np.float32), np.zeros(K, np.int32)
        _check(lib().sift_hip_verify_affine_hypotheses_host(self._v, MODEL_SIMILARITY if similarity else MODEL_AFFINE,
                                                            _ptr(samples), _ptr(A), _ptr(counts), K),
               "verify_affine_hypotheses_host")
        return samples, A, A.any(1), counts

    def verify_affine_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int,
                                     out_ptr: int = 0, out_counts_ptr: int = 0, mask_ptr: int = 0,
                                     max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, q_stride: int = 3,
                                     t_stride: int = 3, stream: Optional[int] = None, similarity: bool = False) -> None:
        """verify_batched_device for the affine models (sift_hip_verify_affine_batched_device)."""
        self._batched_device(self._affine(lib().sift_hip_verify_affine_batched_device, similarity),
                             "verify_affine_batched_device", matches_ptr, counts_ptr, pairs, results_ptr, out_ptr,
                             out_counts_ptr, mask_ptr, max_error, hypotheses, seed, q_stride, t_stride, stream)

    def verify_affine_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, max_error: float = 1.5,
                                   hypotheses: int = 1024, seed: int = 0, q_stride: int = 3, t_stride: int = 3,
                                   full: bool = False, similarity: bool = False) -> list:
        """verify_batched_host for the affine models (sift_hip_verify_affine_batched_host)."""
        return self._batched_host(self._affine(lib().sift_hip_verify_affine_batched_host, similarity),
                                  "verify_affine_batched_host", AFFINE_RESULT_DTYPE, matches_ptr, counts_ptr, pairs,
                                  max_error, hypotheses, seed, q_stride, t_stride, full)

    def refine_affine_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                             nt: int, result_ptr: int, mask_ptr: int, out_ptr: int = 0, out_count_ptr: int = 0,
                             accepted_ptr: int = 0, max_error: float = 1.5, rounds: int = 1, q_stride: int = 3,
                             t_stride: int = 3, stream: Optional[int] = None, similarity: bool = False) -> None:
        """refine_device for the affine models (sift_hip_refine_affine_device)."""
        self._refine_device(self._affine(lib().sift_hip_refine_affine_device, similarity), "refine_affine_device",
                            matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result_ptr, mask_ptr, out_ptr,
                            out_count_ptr, accepted_ptr, max_error, rounds, q_stride, t_stride, stream)

    def refine_affine_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                           nt: int, result, mask, max_error: float = 1.5, rounds: int = 1, q_stride: int = 3,
                           t_stride: int = 3, similarity: bool = False):
        """refine_host for the affine models (sift_hip_refine_affine_host; an AFFINE_RESULT_DTYPE record)."""
        return self._refine_host(self._affine(lib().sift_hip_refine_affine_host, similarity), "refine_affine_host",
                                 AFFINE_RESULT_DTYPE, matches_ptr, count_ptr, cap, q_xy_ptr, nq, t_xy_ptr, nt, result,
                                 mask, max_error, rounds, q_stride, t_stride)

    def refine_affine_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int,
                                     mask_ptr: int, out_ptr: int = 0, out_counts_ptr: int = 0, accepted_ptr: int = 0,
                                     max_error: float = 1.5, rounds: int = 1, q_stride: int = 3, t_stride: int = 3,
                                     stream: Optional[int] = None, similarity: bool = False) -> None:
        """refine_batched_device for the affine models (sift_hip_refine_affine_batched_device)."""
        self._refine_batched_device(self._affine(lib().sift_hip_refine_affine_batched_device, similarity),
                                    "refine_affine_batched_device", matches_ptr, counts_ptr, pairs, results_ptr, mask_ptr,
                                    out_ptr, out_counts_ptr, accepted_ptr, max_error, rounds, q_stride, t_stride, stream)

    def refine_affine_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, verified: Sequence,
                                   max_error: float = 1.5, rounds: int = 1, q_stride: int = 3, t_stride: int = 3,
                                   similarity: bool = False) -> list:
        """refine_batched_host for the affine models (sift_hip_refine_affine_batched_host)."""
        return self._refine_batched_host(self._affine(lib().sift_hip_refine_affine_batched_host, similarity),
                                         "refine_affine_batched_host", AFFINE_RESULT_DTYPE, matches_ptr, counts_ptr, pairs,
                                         verified, max_error, rounds, q_stride, t_stride)

    # --- the essential matrix (sift_hip_verify_essential_*; the rule: include/sift_hip.h, "Essential-matrix
    # verification", in numpy sift_amd.cv.ransac_essential).  The fundamental methods argument for argument with the two
    # cameras (fx, fy, cx, cy) behind the positions; `hypotheses` counts 5-point samples, each owning ten model slots,
    # and is bound by the reservation (essential_samples), not by max_hypotheses.  The record is a VERIFY_RESULT_DTYPE
    # record whose F is the winner's pixel-space matrix: recover_pose_device, refine_device and the epipolar matchers
    # take it as it lies.

    def verify_essential_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                                nt: int, cam_q, cam_t, result_ptr: int, out_ptr: int = 0, out_count_ptr: int = 0,
                                mask_ptr: int = 0, max_error: float = 1.5, hypotheses: int = 256, seed: int = 0,
                                q_stride: int = 3, t_stride: int = 3, stream: Optional[int] = None) -> None:
        """verify_device for the essential matrix (sift_hip_verify_essential_device): `hypothesis` in the record is the
        winning slot 10 k + r, valid_hypotheses the number of valid slots; max_error stays in pixels."""
        p = _VerifyParams(hypotheses, seed, max_error)
        _check(lib().sift_hip_verify_essential_device(
            self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None,
            t_stride, nt, _cameras(cam_q, 1), _cameras(cam_t, 1), ctypes.byref(p), result_ptr or None, out_ptr or None,
            out_count_ptr or None, mask_ptr or None, stream), "verify_essential_device")
        self._e_hypotheses = hypotheses

    def verify_essential_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                              nt: int, cam_q, cam_t, max_error: float = 1.5, hypotheses: int = 256, seed: int = 0,
                              q_stride: int = 3, t_stride: int = 3, full: bool = False):
        """Synchronous (sift_hip_verify_essential_host): what verify_host returns -- (F 3 x 3 float32, the inlier
        records, the winning slot or -1), or with full (the VERIFY_RESULT_DTYPE record, the records, the mask)."""
        p = _VerifyParams(hypotheses, seed, max_error)
        r = _VerifyResult()
        out = np.zeros(max(cap, 0), DMATCH_DTYPE)
        mask = np.zeros(max(cap, 0), np.uint8)
        _check(lib().sift_hip_verify_essential_host(
            self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None,
            t_stride, nt, _cameras(cam_q, 1), _cameras(cam_t, 1), ctypes.byref(p), ctypes.byref(r), _ptr(out),
            _ptr(mask)), "verify_essential_host")
        self._e_hypotheses = hypotheses
        if full:
            return np.frombuffer(bytes(r), VERIFY_RESULT_DTYPE)[0], out[: r.inliers], mask
        return np.array(r.F, np.float32).reshape(3, 3), out[: r.inliers], r.hypothesis

    def essential_hypotheses(self):
        """What the last verify call drew, solved and counted, when it was an essential call of K samples: (samples
        (K, 5) int32, F (10 K, 9) float32, valid (10 K,) bool -- an invalid slot has F all zero --, counts (10 K,)
        int32).  Synchronises the device."""
        K = self._e_hypotheses
        samples, F, counts = np.zeros((K, 5), np.int32), np.zeros((10 * K, 9), np.float32), np.zeros(10 * K, np.int32)
        _check(lib().sift_hip_verify_essential_hypotheses_host(self._v, _ptr(samples), _ptr(F), _ptr(counts), K),
               "verify_essential_hypotheses_host")
        return samples, F, F.any(1), counts

    def verify_essential_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, cams_q, cams_t,
                                        results_ptr: int, out_ptr: int = 0, out_counts_ptr: int = 0, mask_ptr: int = 0,
                                        max_error: float = 1.5, hypotheses: int = 256, seed: int = 0, q_stride: int = 3,
                                        t_stride: int = 3, stream: Optional[int] = None) -> None:
        """verify_batched_device for the essential matrix (sift_hip_verify_essential_batched_device): one camera per
        pair and side."""
        p = _VerifyParams(hypotheses, seed & 0xFFFFFFFF, max_error)
        table, _ = self._pairs(pairs)
        P = len(pairs)
        _check(lib().sift_hip_verify_essential_batched_device(
            self._v, matches_ptr or None, counts_ptr or None, P, table, q_stride, t_stride, _cameras(cams_q, P),
            _cameras(cams_t, P), ctypes.byref(p), results_ptr or None, out_ptr or None, out_counts_ptr or None,
            mask_ptr or None, stream), "verify_essential_batched_device")

    def verify_essential_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, cams_q, cams_t,
                                      max_error: float = 1.5, hypotheses: int = 256, seed: int = 0, q_stride: int = 3,
                                      t_stride: int = 3, full: bool = False) -> list:
        """verify_batched_host for the essential matrix (sift_hip_verify_essential_batched_host)."""
        P = len(pairs)
        cq, ct = _cameras(cams_q, P), _cameras(cams_t, P)

        def fn(v, matches, counts, n, table, qs, ts, params, res, out, mask):
            return lib().sift_hip_verify_essential_batched_host(v, matches, counts, n, table, qs, ts, cq, ct, params, res,
                                                                out, mask)

        return self._batched_host(fn, "verify_essential_batched_host", VERIFY_RESULT_DTYPE, matches_ptr, counts_ptr,
                                  pairs, max_error, hypotheses, seed, q_stride, t_stride, full)

    # --- the relative pose from a verified fundamental matrix (sift_hip_recover_pose_*; the rule: include/sift_hip.h,
    # in numpy sift_amd.cv.recover_pose).  The list, count, cap and positions are the verify call's; result(s) and mask
    # are what it (or a refine call) wrote and are only read.  A camera is (fx, fy, cx, cy).

    def recover_pose_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int,
                            nt: int, result_ptr: int, mask_ptr: int, cam_q, cam_t, pose_ptr: int, mask_out_ptr: int = 0,
                            points_ptr: int = 0, out_ptr: int = 0, out_count_ptr: int = 0, max_depth: float = 50.0,
                            max_cos_parallax: float = 0.99998, q_stride: int = 3, t_stride: int = 3,
                            stream: Optional[int] = None) -> None:
        """Enqueue the pose of the pair (sift_hip_recover_pose_device); every pointer is device memory.  pose_ptr: a
        POSE_RESULT_DTYPE record; mask_out_ptr (cap bytes, may be mask_ptr), points_ptr (cap x 3 floats), out_ptr (room
        for cap records) and out_count_ptr may be 0."""
        p = _PoseParams(max_depth, max_cos_parallax)
        _check(lib().sift_hip_recover_pose_device(
            self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None, t_stride,
            nt, result_ptr or None, mask_ptr or None, _cameras(cam_q, 1), _cameras(cam_t, 1), ctypes.byref(p),
            pose_ptr or None, mask_out_ptr or None, points_ptr or None, out_ptr or None, out_count_ptr or None, stream),
            "recover_pose_device")

    def recover_pose_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int, t_xy_ptr: int, nt: int,
                          result, mask, cam_q, cam_t, max_depth: float = 50.0, max_cos_parallax: float = 0.99998,
                          q_stride: int = 3, t_stride: int = 3):
        """Synchronous (sift_hip_recover_pose_host): result (a VERIFY_RESULT_DTYPE record) and mask (cap bytes) are host
        values as verify_host(full=True) or refine_host return them; the list and positions are device memory.  Returns
        (the POSE_RESULT_DTYPE record, the in-front mask of cap bytes, the points (cap, 3) float32 -- rows past the
        list's count stay NaN --, the in-front records)."""
        res = np.array([result], VERIFY_RESULT_DTYPE)
        mask = np.array(np.asarray(mask, np.uint8).reshape(-1), np.uint8)
        if len(mask) != max(cap, 0):
            raise ValueError("one mask byte per row of the list (cap)")
        p = _PoseParams(max_depth, max_cos_parallax)
        pose = np.zeros(1, POSE_RESULT_DTYPE)
        mask_out = np.zeros(max(cap, 0), np.uint8)
        points = np.full((max(cap, 0), 3), np.nan, np.float32)
        out = np.zeros(max(cap, 0), DMATCH_DTYPE)
        n_out = ctypes.c_int(0)
        _check(lib().sift_hip_recover_pose_host(
            self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None, t_stride,
            nt, _ptr(res), _ptr(mask) if cap > 0 else None, _cameras(cam_q, 1), _cameras(cam_t, 1), ctypes.byref(p),
            _ptr(pose), _ptr(mask_out), _ptr(points), _ptr(out), ctypes.byref(n_out)), "recover_pose_host")
        return pose[0], mask_out, points, out[: n_out.value]

    def recover_pose_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int,
                                    mask_ptr: int, cams_q, cams_t, poses_ptr: int, mask_out_ptr: int = 0,
                                    points_ptr: int = 0, out_ptr: int = 0, out_counts_ptr: int = 0, max_depth: float = 50.0,
                                    max_cos_parallax: float = 0.99998, q_stride: int = 3, t_stride: int = 3,
                                    stream: Optional[int] = None) -> None:
        """Enqueue the pose of every pair (sift_hip_recover_pose_batched_device) on what verify_batched_device and
        refine_batched_device wrote: results_ptr (len(pairs) records) and mask_ptr (the caps' sum bytes) are read;
        cams_q / cams_t: len(pairs) cameras each; poses_ptr: len(pairs) POSE_RESULT_DTYPE records.  Pair p's bytes are
        the single call's."""
        p = _PoseParams(max_depth, max_cos_parallax)
        table, _ = self._pairs(pairs)
        P = len(pairs)
        _check(lib().sift_hip_recover_pose_batched_device(
            self._v, matches_ptr or None, counts_ptr or None, P, table, q_stride, t_stride, results_ptr or None,
            mask_ptr or None, _cameras(cams_q, P), _cameras(cams_t, P), ctypes.byref(p), poses_ptr or None,
            mask_out_ptr or None, points_ptr or None, out_ptr or None, out_counts_ptr or None, stream),
            "recover_pose_batched_device")

    def recover_pose_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, verified: Sequence, cams_q,
                                  cams_t, max_depth: float = 50.0, max_cos_parallax: float = 0.99998, q_stride: int = 3,
                                  t_stride: int = 3) -> list:
        """Synchronous (sift_hip_recover_pose_batched_host): verified holds per pair a tuple with the VERIFY_RESULT_DTYPE
        record first and the mask (cap bytes) last -- (record, mask), or verify_batched_host(full=True)'s (record,
        records, mask); per pair what recover_pose_host returns."""
        table, caps = self._pairs(pairs)
        P = len(pairs)
        if len(verified) != P:
            raise ValueError("one verified (record, ..., mask) per pair")
        row0 = np.concatenate([[0], np.cumsum([c if 0 <= c <= 65536 else 0 for c in caps])]).astype(int)
        res = np.array([v[0] for v in verified], VERIFY_RESULT_DTYPE) if P else np.zeros(1, VERIFY_RESULT_DTYPE)
        mask = np.zeros(row0[-1], np.uint8)
        for i, v in enumerate(verified):
            mask[row0[i]: row0[i + 1]] = np.asarray(v[-1], np.uint8).reshape(-1)
        p = _PoseParams(max_depth, max_cos_parallax)
        poses = np.zeros(max(P, 1), POSE_RESULT_DTYPE)
        mask_out = np.zeros(row0[-1], np.uint8)
        points = np.full((row0[-1], 3), np.nan, np.float32)
        out = np.zeros(row0[-1], DMATCH_DTYPE)
        n_out = np.zeros(max(P, 1), np.int32)
        _check(lib().sift_hip_recover_pose_batched_host(
            self._v, matches_ptr or None, counts_ptr or None, P, table, q_stride, t_stride, _ptr(res),
            _ptr(mask) if len(mask) else None, _cameras(cams_q, P), _cameras(cams_t, P), ctypes.byref(p), _ptr(poses),
            _ptr(mask_out), _ptr(points), _ptr(out), _ptr(n_out)), "recover_pose_batched_host")
        return [(poses[i].copy(), mask_out[row0[i]: row0[i + 1]].copy(), points[row0[i]: row0[i + 1]].copy(),
                 out[row0[i]: row0[i] + n_out[i]].copy()) for i in range(P)]


    # --- the relative pose from a verified homography (sift_hip_recover_pose_homography_*; the rule: include/sift_hip.h,
    # in numpy sift_amd.cv.recover_pose_homography).  Argument for argument the pose calls above, on what the
    # homography verify and refine calls wrote, with the 96-byte record and the optional four candidates per pair.

    def recover_pose_homography_device(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int,
                                       t_xy_ptr: int, nt: int, result_ptr: int, mask_ptr: int, cam_q, cam_t, pose_ptr: int,
                                       mask_out_ptr: int = 0, points_ptr: int = 0, out_ptr: int = 0, out_count_ptr: int = 0,
                                       candidates_ptr: int = 0, max_depth: float = 50.0,
                                       max_cos_parallax: float = 0.99998, q_stride: int = 3, t_stride: int = 3,
                                       stream: Optional[int] = None) -> None:
        """Enqueue the plane pose of the pair (sift_hip_recover_pose_homography_device); every pointer is device memory.
        pose_ptr: a PLANE_POSE_RESULT_DTYPE record; candidates_ptr: four PLANE_CANDIDATE_DTYPE records, or 0; the other
        optional outputs as for recover_pose_device."""
        p = _PoseParams(max_depth, max_cos_parallax)
        _check(lib().sift_hip_recover_pose_homography_device(
            self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None, t_stride,
            nt, result_ptr or None, mask_ptr or None, _cameras(cam_q, 1), _cameras(cam_t, 1), ctypes.byref(p),
            pose_ptr or None, mask_out_ptr or None, points_ptr or None, out_ptr or None, out_count_ptr or None,
            candidates_ptr or None, stream), "recover_pose_homography_device")

    def recover_pose_homography_host(self, matches_ptr: int, count_ptr: int, cap: int, q_xy_ptr: int, nq: int,
                                     t_xy_ptr: int, nt: int, result, mask, cam_q, cam_t, max_depth: float = 50.0,
                                     max_cos_parallax: float = 0.99998, q_stride: int = 3, t_stride: int = 3):
        """Synchronous (sift_hip_recover_pose_homography_host): result (a HOMOGRAPHY_RESULT_DTYPE record) and mask (cap
        bytes) are host values; the list and positions are device memory.  Returns (the PLANE_POSE_RESULT_DTYPE record,
        the in-front mask, the points (cap, 3) float32, the in-front records, the four PLANE_CANDIDATE_DTYPE records)."""
        res = np.array([result], HOMOGRAPHY_RESULT_DTYPE)
        mask = np.array(np.asarray(mask, np.uint8).reshape(-1), np.uint8)
        if len(mask) != max(cap, 0):
            raise ValueError("one mask byte per row of the list (cap)")
        p = _PoseParams(max_depth, max_cos_parallax)
        pose = np.zeros(1, PLANE_POSE_RESULT_DTYPE)
        mask_out = np.zeros(max(cap, 0), np.uint8)
        points = np.full((max(cap, 0), 3), np.nan, np.float32)
        out = np.zeros(max(cap, 0), DMATCH_DTYPE)
        n_out = ctypes.c_int(0)
        cands = np.zeros(4, PLANE_CANDIDATE_DTYPE)
        _check(lib().sift_hip_recover_pose_homography_host(
            self._v, matches_ptr or None, count_ptr or None, cap, q_xy_ptr or None, q_stride, nq, t_xy_ptr or None, t_stride,
            nt, _ptr(res), _ptr(mask) if cap > 0 else None, _cameras(cam_q, 1), _cameras(cam_t, 1), ctypes.byref(p),
            _ptr(pose), _ptr(mask_out), _ptr(points), _ptr(out), ctypes.byref(n_out), _ptr(cands)),
            "recover_pose_homography_host")
        return pose[0], mask_out, points, out[: n_out.value], cands

    def recover_pose_homography_batched_device(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, results_ptr: int,
                                               mask_ptr: int, cams_q, cams_t, poses_ptr: int, mask_out_ptr: int = 0,
                                               points_ptr: int = 0, out_ptr: int = 0, out_counts_ptr: int = 0,
                                               candidates_ptr: int = 0, max_depth: float = 50.0,
                                               max_cos_parallax: float = 0.99998, q_stride: int = 3, t_stride: int = 3,
                                               stream: Optional[int] = None) -> None:
        """Enqueue the plane pose of every pair (sift_hip_recover_pose_homography_batched_device) on what
        verify_homography_batched_device and refine_homography_batched_device wrote; poses_ptr: len(pairs)
        PLANE_POSE_RESULT_DTYPE records; candidates_ptr: 4 x len(pairs) PLANE_CANDIDATE_DTYPE records, or 0.  Pair p's
        bytes are the single call's."""
        p = _PoseParams(max_depth, max_cos_parallax)
        table, _ = self._pairs(pairs)
        P = len(pairs)
        _check(lib().sift_hip_recover_pose_homography_batched_device(
            self._v, matches_ptr or None, counts_ptr or None, P, table, q_stride, t_stride, results_ptr or None,
            mask_ptr or None, _cameras(cams_q, P), _cameras(cams_t, P), ctypes.byref(p), poses_ptr or None,
            mask_out_ptr or None, points_ptr or None, out_ptr or None, out_counts_ptr or None, candidates_ptr or None,
            stream), "recover_pose_homography_batched_device")

    def recover_pose_homography_batched_host(self, matches_ptr: int, counts_ptr: int, pairs: Sequence, verified: Sequence,
                                             cams_q, cams_t, max_depth: float = 50.0, max_cos_parallax: float = 0.99998,
                                             q_stride: int = 3, t_stride: int = 3) -> list:
        """Synchronous (sift_hip_recover_pose_homography_batched_host): verified holds per pair a tuple with the
        HOMOGRAPHY_RESULT_DTYPE record first and the mask (cap bytes) last; per pair what recover_pose_homography_host
        returns."""
        table, caps = self._pairs(pairs)
        P = len(pairs)
        if len(verified) != P:
            raise ValueError("one verified (record, ..., mask) per pair")
        row0 = np.concatenate([[0], np.cumsum([c if 0 <= c <= 65536 else 0 for c in caps])]).astype(int)
        res = np.array([v[0] for v in verified], HOMOGRAPHY_RESULT_DTYPE) if P else np.zeros(1, HOMOGRAPHY_RESULT_DTYPE)
        mask = np.zeros(row0[-1], np.uint8)
        for i, v in enumerate(verified):
            mask[row0[i]: row0[i + 1]] = np.asarray(v[-1], np.uint8).reshape(-1)
        p = _PoseParams(max_depth, max_cos_parallax)
        poses = np.zeros(max(P, 1), PLANE_POSE_RESULT_DTYPE)
        mask_out = np.zeros(row0[-1], np.uint8)
        points = np.full((row0[-1], 3), np.nan, np.float32)
        out = np.zeros(row0[-1], DMATCH_DTYPE)
        n_out = np.zeros(max(P, 1), np.int32)
        cands = np.zeros((max(P, 1), 4), PLANE_CANDIDATE_DTYPE)
        _check(lib().sift_hip_recover_pose_homography_batched_host(
            self._v, matches_ptr or None, counts_ptr or None, P, table, q_stride, t_stride, _ptr(res),
            _ptr(mask) if len(mask) else None, _cameras(cams_q, P), _cameras(cams_t, P), ctypes.byref(p), _ptr(poses),
            _ptr(mask_out), _ptr(points), _ptr(out), _ptr(n_out), _ptr(cands)), "recover_pose_homography_batched_host")
        return [(poses[i].copy(), mask_out[row0[i]: row0[i + 1]].copy(), points[row0[i]: row0[i + 1]].copy(),
                 out[row0[i]: row0[i] + n_out[i]].copy(), cands[i].copy()) for i in range(P)]


def _verify_batched(host, refine, matches_per_pair, xy_per_pair, max_error, hypotheses, seed, refit,
                    max_hypotheses=None):
    if len(matches_per_pair) != len(xy_per_pair):
        raise ValueError("one (des_xy, src_xy) per match list")
    lists = [np.ascontiguousarray(np.asarray(m, DMATCH_DTYPE)).reshape(-1) for m in matches_per_pair]
    xy = [[np.ascontiguousarray(np.asarray(a, np.float32)[:, :2]) for a in qt] for qt in xy_per_pair]
    rows = sum(len(m) for m in lists)
    v = Verifier(max(rows, 1), max_hypotheses or hypotheses, max(len(lists), 1))
    d = DeviceArray.from_numpy(np.concatenate(lists) if lists else np.zeros(0, DMATCH_DTYPE))
    dxy = [[DeviceArray.from_numpy(a) for a in qt] for qt in xy]
    pairs = [(dq.value, len(q), dt.value, len(t), len(m)) for m, (q, t), (dq, dt) in zip(lists, xy, dxy)]
    if not refit:
        return host(v, d.value if rows else 0, 0, pairs, max_error, hypotheses, seed, 2, 2)
    verified = host(v, d.value if rows else 0, 0, pairs, max_error, hypotheses, seed, 2, 2, True)
    refined = refine(v, d.value if rows else 0, 0, pairs, verified, max_error, refit, 2, 2)
    return [(r[r.dtype.names[0]].reshape(3, 3).copy(), recs, int(r["hypothesis"])) for r, recs, _, _ in refined]


def verifyFundamentalBatched(matches_per_pair: Sequence[np.ndarray], xy_per_pair: Sequence, max_error: float = 1.5,
                             hypotheses: int = 1024, seed: int = 0, refit: int = 0) -> list:
    """verifyFundamental for P lists in one pass: matches_per_pair[p] a DMATCH_DTYPE array, xy_per_pair[p] =
    (des_xy, src_xy) host float arrays of rows with x, y first.  A list of what verifyFundamental returns per pair --
    (F, the inlier records, the winning hypothesis or -1) --, pair p verified with the seed `seed + p`.  refit: as for verifyFundamental."""
    return _verify_batched(Verifier.verify_batched_host, Verifier.refine_batched_host, matches_per_pair, xy_per_pair,
                           max_error, hypotheses, seed, refit)


def verifyHomographyBatched(matches_per_pair: Sequence[np.ndarray], xy_per_pair: Sequence, max_error: float = 1.5,
                            hypotheses: int = 1024, seed: int = 0, refit: int = 0) -> list:
    """verifyFundamentalBatched for the homography: per pair what verifyHomography returns."""
    return _verify_batched(Verifier.verify_homography_batched_host, Verifier.refine_homography_batched_host,
                           matches_per_pair, xy_per_pair, max_error, hypotheses, seed, refit)


def verifyAffineBatched(matches_per_pair: Sequence[np.ndarray], xy_per_pair: Sequence, similarity: bool = False,
                        max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, refit: int = 0) -> list:
    """verifyFundamentalBatched for the affine map or, with similarity, the similarity: per pair what verifyAffine
    returns."""
    def host(v, *args):
        return v.verify_affine_batched_host(*args, similarity=similarity)

    def refine(v, *args):
        return v.refine_affine_batched_host(*args, similarity=similarity)

    return _verify_batched(host, refine, matches_per_pair, xy_per_pair, max_error, hypotheses, seed, refit)


def verifyFundamental(matches: np.ndarray, des_xy, src_xy, n_des: int, n_src: int, max_error: float = 1.5,
                      hypotheses: int = 1024, seed: int = 0, des_stride: int = 3, src_stride: int = 3, refit: int = 0):
    """Geometric verification of a match list (matchList's output): (F 3 x 3 float32 with x_src^T F x_des = 0, the
    inlier records in input order, the winning hypothesis or -1 when there are fewer than 8 matches or no sample could
    be solved).  matches: a DMATCH_DTYPE array (uploaded here); des_xy / src_xy: DeviceBuffers or raw device pointers
    of n_des / n_src float rows with x, y first, as for matchListEpipolar.  The returned F is what matchListEpipolar
    takes.  refit = 1..8: that many refit rounds on the device (Verifier.refine_host) follow -- F is then the rank-2
    least-squares fit of its inliers whenever that fit counts at least as many; 0: the minimal-sample winner."""
    m = np.ascontiguousarray(np.asarray(matches, DMATCH_DTYPE))
    v = Verifier(max(len(m), 1), hypotheses)
    d = DeviceArray.from_numpy(m)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    args = (d.value if len(m) else 0, 0, len(m), qxy, n_des, txy, n_src)
    if not refit:
        return v.verify_host(*args, max_error, hypotheses, seed, des_stride, src_stride)
    r, _, mask = v.verify_host(*args, max_error, hypotheses, seed, des_stride, src_stride, True)
    r, recs, _, _ = v.refine_host(*args, r, mask, max_error, refit, des_stride, src_stride)
    return r["F"].reshape(3, 3).copy(), recs, int(r["hypothesis"])


def verifyHomography(matches: np.ndarray, des_xy, src_xy, n_des: int, n_src: int, max_error: float = 1.5,
                     hypotheses: int = 1024, seed: int = 0, des_stride: int = 3, src_stride: int = 3, refit: int = 0):
    """verifyFundamental for the homography: (H 3 x 3 float32 of unit norm with x_src ~ H x_des -- divide by H[2, 2]
    for cv::findHomography's scale --, the inlier records in input order, the winning hypothesis or -1 when there are
    fewer than 4 matches or no sample was valid).  refit: as for verifyFundamental (Verifier.refine_homography_host)."""
    m = np.ascontiguousarray(np.asarray(matches, DMATCH_DTYPE))
    v = Verifier(max(len(m), 1), hypotheses)
    d = DeviceArray.from_numpy(m)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    args = (d.value if len(m) else 0, 0, len(m), qxy, n_des, txy, n_src)
    if not refit:
        return v.verify_homography_host(*args, max_error, hypotheses, seed, des_stride, src_stride)
    r, _, mask = v.verify_homography_host(*args, max_error, hypotheses, seed, des_stride, src_stride, True)
    r, recs, _, _ = v.refine_homography_host(*args, r, mask, max_error, refit, des_stride, src_stride)
    return r["H"].reshape(3, 3).copy(), recs, int(r["hypothesis"])


def verifyAffine(matches: np.ndarray, des_xy, src_xy, n_des: int, n_src: int, similarity: bool = False,
                 max_error: float = 1.5, hypotheses: int = 1024, seed: int = 0, des_stride: int = 3, src_stride: int = 3,
                 refit: int = 0):
    """verifyFundamental for the affine map (cv::estimateAffine2D) or, with similarity, the similarity
    (cv::estimateAffinePartial2D): (A 3 x 3 float32 with x_src = A x_des and the last row 0 0 1, the inlier records
    in input order, the winning hypothesis or -1 when there are fewer than 3 / 2 matches or no sample was valid).
    refit: as for verifyFundamental (Verifier.refine_affine_host) -- worth more here than for the other models, a
    minimal model through 2 or 3 grid-rounded points being rough."""
    m = np.ascontiguousarray(np.asarray(matches, DMATCH_DTYPE))
    v = Verifier(max(len(m), 1), hypotheses)
    d = DeviceArray.from_numpy(m)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    args = (d.value if len(m) else 0, 0, len(m), qxy, n_des, txy, n_src)
    if not refit:
        return v.verify_affine_host(*args, max_error, hypotheses, seed, des_stride, src_stride, similarity=similarity)
    r, _, mask = v.verify_affine_host(*args, max_error, hypotheses, seed, des_stride, src_stride, True, similarity)
    r, recs, _, _ = v.refine_affine_host(*args, r, mask, max_error, refit, des_stride, src_stride, similarity)
    return r["H"].reshape(3, 3).copy(), recs, int(r["hypothesis"])


def verifyEssential(matches: np.ndarray, des_xy, src_xy, n_des: int, n_src: int, cam_q, cam_t, max_error: float = 1.5,
                    hypotheses: int = 256, seed: int = 0, des_stride: int = 3, src_stride: int = 3, refit: int = 0):
    """cv::findEssentialMat on a match list: verifyFundamental with 5-point samples under the two cameras
    (fx, fy, cx, cy) of the des and the src side.  Returns what verifyFundamental returns -- (F 3 x 3 float32 in pixel
    space, the inlier records in input order, the winning slot 10 k + r or -1 when there are fewer than 5 matches or no
    sample had a solution) -- and E = Kt^T F Kq (3 x 3 float64, cv.essential_from_fundamental).  `hypotheses` counts
    samples.  refit = 1..8: Verifier.refine_host on the record -- the 8-point least-squares F, not an essential refit;
    skip it on near-planar scenes, where that fit is ill-conditioned and can still be accepted."""
    from . import cv

    m = np.ascontiguousarray(np.asarray(matches, DMATCH_DTYPE))
    v = Verifier(max(len(m), 1), 1, essential_samples=hypotheses)
    d = DeviceArray.from_numpy(m)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    args = (d.value if len(m) else 0, 0, len(m), qxy, n_des, txy, n_src)
    if not refit:
        F, recs, hyp = v.verify_essential_host(*args, cam_q, cam_t, max_error, hypotheses, seed, des_stride, src_stride)
    else:
        r, _, mask = v.verify_essential_host(*args, cam_q, cam_t, max_error, hypotheses, seed, des_stride, src_stride,
                                             True)
        r, recs, _, _ = v.refine_host(*args, r, mask, max_error, refit, des_stride, src_stride)
        F, hyp = r["F"].reshape(3, 3).copy(), int(r["hypothesis"])
    return F, recs, hyp, cv.essential_from_fundamental(F, cam_q, cam_t)


def verifyEssentialBatched(matches_per_pair: Sequence[np.ndarray], xy_per_pair: Sequence, cams_q, cams_t,
                           max_error: float = 1.5, hypotheses: int = 256, seed: int = 0, refit: int = 0) -> list:
    """verifyFundamentalBatched for the essential matrix: cams_q / cams_t one (fx, fy, cx, cy) per pair; per pair what
    verifyEssential returns."""
    from . import cv

    def host(v, *args):
        if not v.essential_samples:
            v.reserve_essential(hypotheses)
        return v.verify_essential_batched_host(*args[:3], cams_q, cams_t, *args[3:])

    got = _verify_batched(host, Verifier.refine_batched_host, matches_per_pair, xy_per_pair, max_error, hypotheses, seed,
                          refit, max_hypotheses=1)
    cq, ct = np.asarray(cams_q, np.float32).reshape(-1, 4), np.asarray(cams_t, np.float32).reshape(-1, 4)
    return [(F, recs, hyp, cv.essential_from_fundamental(F, cq[p], ct[p])) for p, (F, recs, hyp) in enumerate(got)]


def recoverPose(matches: np.ndarray, des_xy, src_xy, n_des: int, n_src: int, result, mask, cam_q, cam_t,
                max_depth: float = 50.0, max_cos_parallax: float = 0.99998, des_stride: int = 3, src_stride: int = 3):
    """cv::recoverPose on a verified pair: matches (a DMATCH_DTYPE array, uploaded here), des_xy / src_xy (DeviceBuffers
    or raw device pointers, as for verifyFundamental), result -- a VERIFY_RESULT_DTYPE record, or F as 9 floats (3 x 3)
    -- and mask, the inlier mask (one byte per match; None: every match).  cam_q / cam_t: (fx, fy, cx, cy) of the des
    and the src side.  Returns (R 3 x 3 float32, t (3,) float32 with X_src = R X_des + t and |t| = 1, the in-front mask,
    the points (n, 3) in the des camera's frame, the POSE_RESULT_DTYPE record); candidate = -1 in the record: no pose."""
    m = np.ascontiguousarray(np.asarray(matches, DMATCH_DTYPE)).reshape(-1)
    if not (isinstance(result, np.void) or (isinstance(result, np.ndarray) and result.dtype == VERIFY_RESULT_DTYPE)):
        rec = np.zeros(1, VERIFY_RESULT_DTYPE)
        rec["F"][0] = np.asarray(result, np.float32).reshape(9)
        rec["matches"][0] = len(m)
        result = rec[0]
    mask = np.ones(len(m), np.uint8) if mask is None else mask
    v = Verifier(max(len(m), 1), 1)
    d = DeviceArray.from_numpy(m)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    pose, mask_out, points, _ = v.recover_pose_host(d.value if len(m) else 0, 0, len(m), qxy, n_des, txy, n_src, result,
                                                    mask, cam_q, cam_t, max_depth, max_cos_parallax, des_stride,
                                                    src_stride)
    return pose["R"].reshape(3, 3).copy(), pose["t"].copy(), mask_out, points, pose


def recoverPoseBatched(matches_per_pair: Sequence[np.ndarray], xy_per_pair: Sequence, results: Sequence, masks: Sequence,
                       cams_q, cams_t, max_depth: float = 50.0, max_cos_parallax: float = 0.99998) -> list:
    """recoverPose for P pairs in one pass: matches_per_pair[p] a DMATCH_DTYPE array, xy_per_pair[p] = (des_xy, src_xy)
    host float arrays of rows with x, y first, results[p] a VERIFY_RESULT_DTYPE record, masks[p] its inlier mask,
    cams_q / cams_t P cameras each.  A list of what recoverPose returns per pair."""
    if not (len(matches_per_pair) == len(xy_per_pair) == len(results) == len(masks)):
        raise ValueError("one (des_xy, src_xy), record and mask per match list")
    lists = [np.ascontiguousarray(np.asarray(m, DMATCH_DTYPE)).reshape(-1) for m in matches_per_pair]
    xy = [[np.ascontiguousarray(np.asarray(a, np.float32)[:, :2]) for a in qt] for qt in xy_per_pair]
    rows = sum(len(m) for m in lists)
    v = Verifier(max(rows, 1), 1, max(len(lists), 1))
    d = DeviceArray.from_numpy(np.concatenate(lists) if lists else np.zeros(0, DMATCH_DTYPE))
    dxy = [[DeviceArray.from_numpy(a) for a in qt] for qt in xy]
    pairs = [(dq.value, len(q), dt.value, len(t), len(m)) for m, (q, t), (dq, dt) in zip(lists, xy, dxy)]
    got = v.recover_pose_batched_host(d.value if rows else 0, 0, pairs, list(zip(results, masks)), cams_q, cams_t,
                                      max_depth, max_cos_parallax, 2, 2)
    return [(pose["R"].reshape(3, 3).copy(), pose["t"].copy(), mask_out, points, pose)
            for pose, mask_out, points, _ in got]


def recoverPoseHomography(matches: np.ndarray, des_xy, src_xy, n_des: int, n_src: int, result, mask, cam_q, cam_t,
                          max_depth: float = 50.0, max_cos_parallax: float = 0.99998, des_stride: int = 3,
                          src_stride: int = 3):
    """cv::decomposeHomographyMat and the choice by visible points on a verified pair: the arguments are recoverPose's,
    with result a HOMOGRAPHY_RESULT_DTYPE record or H as 9 floats (3 x 3, signed as verifyHomography signs it).
    Returns (R, t, the in-front mask, the points, the PLANE_POSE_RESULT_DTYPE record, the four PLANE_CANDIDATE_DTYPE
    candidates); the record's normal and distance are the plane n^T X_des = distance, in baselines.  Two equal entries
    at the top of the record's counts: the plane has two valid poses, and the first is returned."""
    m = np.ascontiguousarray(np.asarray(matches, DMATCH_DTYPE)).reshape(-1)
    if not (isinstance(result, np.void) or (isinstance(result, np.ndarray) and result.dtype == HOMOGRAPHY_RESULT_DTYPE)):
        rec = np.zeros(1, HOMOGRAPHY_RESULT_DTYPE)
        rec["H"][0] = np.asarray(result, np.float32).reshape(9)
        rec["matches"][0] = len(m)
        result = rec[0]
    mask = np.ones(len(m), np.uint8) if mask is None else mask
    v = Verifier(max(len(m), 1), 1)
    d = DeviceArray.from_numpy(m)
    qxy, txy = (p.data() if isinstance(p, DeviceBuffer) else int(p or 0) for p in (des_xy, src_xy))
    pose, mask_out, points, _, cands = v.recover_pose_homography_host(
        d.value if len(m) else 0, 0, len(m), qxy, n_des, txy, n_src, result, mask, cam_q, cam_t, max_depth,
        max_cos_parallax, des_stride, src_stride)
    return pose["R"].reshape(3, 3).copy(), pose["t"].copy(), mask_out, points, pose, cands


def recoverPoseHomographyBatched(matches_per_pair: Sequence[np.ndarray], xy_per_pair: Sequence, results: Sequence,
                                 masks: Sequence, cams_q, cams_t, max_depth: float = 50.0,
                                 max_cos_parallax: float = 0.99998) -> list:
    """recoverPoseHomography for P pairs in one pass; the arguments are recoverPoseBatched's with
    HOMOGRAPHY_RESULT_DTYPE records.  A list of what recoverPoseHomography returns per pair."""
    if not (len(matches_per_pair) == len(xy_per_pair) == len(results) == len(masks)):
        raise ValueError("one (des_xy, src_xy), record and mask per match list")
    lists = [np.ascontiguousarray(np.asarray(m, DMATCH_DTYPE)).reshape(-1) for m in matches_per_pair]
    xy = [[np.ascontiguousarray(np.asarray(a, np.float32)[:, :2]) for a in qt] for qt in xy_per_pair]
    rows = sum(len(m) for m in lists)
    v = Verifier(max(rows, 1), 1, max(len(lists), 1))
    d = DeviceArray.from_numpy(np.concatenate(lists) if lists else np.zeros(0, DMATCH_DTYPE))
    dxy = [[DeviceArray.from_numpy(a) for a in qt] for qt in xy]
    pairs = [(dq.value, len(q), dt.value, len(t), len(m)) for m, (q, t), (dq, dt) in zip(lists, xy, dxy)]
    got = v.recover_pose_homography_batched_host(d.value if rows else 0, 0, pairs, list(zip(results, masks)), cams_q,
                                                 cams_t, max_depth, max_cos_parallax, 2, 2)
    return [(pose["R"].reshape(3, 3).copy(), pose["t"].copy(), mask_out, points, pose, cands)
            for pose, mask_out, points, _, cands in got]


def project_homography_device(H_ptr: int, xy_ptr: int, n: int, out_ptr: int, stride: int = 3, out_stride: int = 2,
                              stream: Optional[int] = None) -> None:
    """Enqueue the projection (sift_hip_project_homography_device): row i of out = row i of xy (n device rows of
    `stride` floats, x and y first) carried over by the 9 device floats at H_ptr -- normally the result record of
    verify_homography_device --, (NaN, NaN) where the point lands behind the camera.  out_ptr may be xy_ptr with equal
    strides."""
    _check(lib().sift_hip_project_homography_device(H_ptr or None, xy_ptr or None, stride, n, out_ptr or None, out_stride,
                                                    stream), "project_homography_device")


def project_homography_batched_device(geometry_ptr: int, sets: Sequence, stride: int = 3, out_stride: int = 2,
                                      geometry_stride: int = 52, stream: Optional[int] = None) -> None:
    """project_homography_device for len(sets) sets in one launch (sift_hip_project_homography_batched_device): set p
    = (xy_ptr, n, out_ptr) goes through the 9 device floats at geometry_ptr + p * geometry_stride bytes -- with the
    default stride the HOMOGRAPHY_RESULT_DTYPE records of Verifier.verify_homography_batched_device as they lie."""
    P = len(sets)
    table = (_ProjectSet * max(P, 1))(*[_ProjectSet(s[0] or None, s[1], s[2] or None) for s in sets])
    _check(lib().sift_hip_project_homography_batched_device(geometry_ptr or None, geometry_stride, P, table, stride,
                                                            out_stride, stream), "project_homography_batched_device")


def _match_list_gated_batched(desc_per_pair, xy_per_pair, run):
    if len(desc_per_pair) != len(xy_per_pair):
        raise ValueError("one (des_xy, src_xy) per (des, src)")
    P = len(desc_per_pair)
    if P == 0:
        return []
    des = [[np.ascontiguousarray(np.asarray(a, np.float16).reshape(-1, 128)) for a in qt] for qt in desc_per_pair]
    xy = [[np.ascontiguousarray(np.asarray(a, np.float32)[:, :2]) for a in qt] for qt in xy_per_pair]
    cap = max(max(len(a) for ds in des for a in ds), 1)
    m = Matcher(cap, cap, max_pairs=2 * P if 2 * P <= 64 else P)
    dd = [[DeviceArray.from_numpy(a) for a in ds] for ds in des]
    dxy = [[DeviceArray.from_numpy(a) for a in qt] for qt in xy]
    nqs, nts = [len(ds[0]) for ds in des], [len(ds[1]) for ds in des]
    out, counts = DeviceArray(DMATCH_DTYPE.itemsize * max(sum(nqs), 1)), DeviceArray(4 * P)
    run(m, [d[0].value if n else 0 for d, n in zip(dd, nqs)], nqs, [d[1].value if n else 0 for d, n in zip(dd, nts)], nts,
        [(a.value, b.value) for a, b in dxy], out.value, counts.value)
    _check(lib().sift_hip_device_sync(), "device_sync")
    rec, cnt = out.to_numpy(DMATCH_DTYPE, max(sum(nqs), 1)), counts.to_numpy(np.int32, P)
    row0 = np.concatenate([[0], np.cumsum(nqs)]).astype(int)
    return [rec[row0[p]: row0[p] + cnt[p]].copy() for p in range(P)]


def matchListGuidedBatched(desc_per_pair: Sequence, xy_per_pair: Sequence, radius: float, **filter) -> list:
    """matchListGuided for P pairs in one pass, on host arrays: desc_per_pair[p] = (des, src) descriptor rows (n x 128,
    converted to float16), xy_per_pair[p] = (des_xy, src_xy) float rows with x, y first.  A list of DMATCH_DTYPE arrays
    (imgIdx = p), pair p what matchListGuided gives on it.  `filter` keywords as matchList."""
    return _match_list_gated_batched(
        desc_per_pair, xy_per_pair,
        lambda m, q, nq, t, nt, pos, out, counts: m.match_list_guided_batched(q, nq, t, nt, pos, radius, out, counts, 2, 2,
                                                                              **filter))


def matchListEpipolarBatched(desc_per_pair: Sequence, xy_per_pair: Sequence, F_per_pair: Sequence, max_error: float,
                             radius: float = float("inf"), **filter) -> list:
    """matchListEpipolar for P pairs in one pass, on host arrays as matchListGuidedBatched takes them; F_per_pair[p]:
    pair p's 9 floats (uploaded here; a pair whose F is not cv.geometry_usable gets an empty list)."""
    F = np.ascontiguousarray(np.asarray(F_per_pair, np.float32).reshape(len(desc_per_pair), 9))
    dF = DeviceArray.from_numpy(F)
    return _match_list_gated_batched(
        desc_per_pair, xy_per_pair,
        lambda m, q, nq, t, nt, pos, out, counts: m.match_list_epipolar_batched(q, nq, t, nt, pos, dF.value, max_error,
                                                                                out, counts, radius, 36, 2, 2,
                                                                                **filter))


def matchBruteForce(des: DeviceBuffer, num_des: int, src: DeviceBuffer, num_src: int) -> np.ndarray:
    """Match.cuh:9-14: nearest src row per des row if d1^2 < 0.8 d2^2, else -1."""
    global _default_matcher
    if _default_matcher is None or num_des > _default_matcher.max_query or num_src > _default_matcher.max_train:
        mq = max(num_des, _default_matcher.max_query if _default_matcher else 0, 1)
        mt = max(num_src, _default_matcher.max_train if _default_matcher else 0, 1)
        _default_matcher = Matcher(mq, mt)
    if num_des <= 0:
        return np.zeros(0, np.int32)
    return _default_matcher.match_host(des.data(), num_des, src.data(), num_src, 0.8, True)


def rootsift_device(src_ptr: int, n: int, dst_ptr: Optional[int] = None, stream: Optional[int] = None) -> None:
    """The RootSIFT rule (sift_hip_rootsift_device, cv.rootsift) on n device rows of 128 fp16 values
    the detector did not write with root_sift: src -> dst, dst_ptr=None in place.  One launch on
    `stream` (None: the default stream), not synchronised.  A detector's own buffer is passed as
    mutable_data(), so that later matches convert the written rows."""
    dst = src_ptr if dst_ptr is None else dst_ptr
    _check(lib().sift_hip_rootsift_device(src_ptr, int(n), dst, stream), "rootsift_device")


def rootsift(desc: np.ndarray) -> np.ndarray:
    """The same rule on a host array of rows (n, 128), through the device (sift_hip_rootsift_host,
    synchronous): float16 rows of integers 0..255, equal to cv.rootsift(desc) byte for byte."""
    a = np.ascontiguousarray(np.asarray(desc), dtype=np.float16)
    if a.ndim != 2 or a.shape[1] != 128:
        raise ValueError(f"rootsift: rows of 128 values expected, got shape {a.shape}")
    out = np.empty_like(a)
    _check(lib().sift_hip_rootsift_host(_ptr(a), a.shape[0], _ptr(out)), "rootsift_host")
    return out


class DeviceArray:
    """Minimal owning device allocation for callers without torch (tests)."""

    def __init__(self, nbytes: int):
        self.ptr = ctypes.c_void_p()
        self.nbytes = nbytes
        _check(lib().sift_hip_malloc(ctypes.byref(self.ptr), max(nbytes, 1)), "malloc")

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DeviceArray":
        a = np.ascontiguousarray(a)
        d = cls(a.nbytes)
        _check(lib().sift_hip_memcpy_h2d(d.ptr, _ptr(a), a.nbytes), "h2d")
        return d

    def to_numpy(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        _check(lib().sift_hip_memcpy_d2h(_ptr(out), self.ptr, out.nbytes), "d2h")
        return out

    @property
    def value(self) -> int:
        return self.ptr.value

    def __del__(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value and _lib is not None:
            _lib.sift_hip_free(self.ptr)
            self.ptr = None
