"""OpenCV interop, mirroring the reference's
cvUtils/Conversion.hh:12-70 (``OpencvUtils::localKptToCvKpt``,
``descriptorToCvMat``, ``cvtMatchToDMatch``).  The field mapping is plain
numpy so it is usable (and tested) without OpenCV; the ``cv2`` object builders
import cv2 lazily and raise ImportError where OpenCV is absent.
"""
from typing import List, Sequence

import numpy as np


def keypoint_fields(final_kpts: np.ndarray, final_features: np.ndarray, size: int = -1) -> dict:
    """Conversion.cc:21-42 field by field: pt = kpts[:, :2], octave = int(features.x),
    size = features.y, response = features.z, angle = features.w."""
    k = np.asarray(final_kpts, np.float32).reshape(-1, 3)
    f = np.asarray(final_features, np.float32).reshape(-1, 4)
    if len(k) != len(f):
        raise ValueError("kpts and features differ in length")
    n = len(k) if size < 0 else min(size, len(k))
    return {"x": k[:n, 0], "y": k[:n, 1], "octave": f[:n, 0].astype(np.int64).astype(np.int32),
            "size": f[:n, 1], "response": f[:n, 2], "angle": f[:n, 3]}


def keypoint_records(fields_or_kpts, final_features=None) -> np.ndarray:
    """The inverse of keypoint_fields: KPT_DTYPE records (what Detector.compute takes) from its field dict, or from
    (final_kpts, final_features) as a detector returns them."""
    from . import KPT_DTYPE

    f = fields_or_kpts if isinstance(fields_or_kpts, dict) else keypoint_fields(fields_or_kpts, final_features)
    out = np.zeros(len(f["x"]), KPT_DTYPE)
    for name in KPT_DTYPE.names:
        out[name] = f[name]
    return out


def from_cv_keypoints(kpts) -> np.ndarray:
    """list of cv2.KeyPoint -> KPT_DTYPE records (class_id dropped)."""
    import cv2  # noqa: F401  (the objects are cv2's; absent OpenCV is an ImportError, as in to_cv_keypoints)

    from . import KPT_DTYPE

    out = np.zeros(len(kpts), KPT_DTYPE)
    for i, k in enumerate(kpts):
        out[i] = (k.pt[0], k.pt[1], k.size, k.angle, k.response, k.octave)
    return out


def mask_keep(x, y, mask: np.ndarray) -> np.ndarray:
    """KeyPointsFilter::runByPixelsMask in numpy (the rule of Detector.detectAndCompute(image, mask)): keypoint i is
    kept when mask[int(y[i] + 0.5f), int(x[i] + 0.5f)] != 0 -- float32 add, truncating cast, any non-zero byte keeps.
    `mask`: 2-D uint8 (any strides).  Returns a bool array; kpts[mask_keep(kpts[:, 0], kpts[:, 1], mask)] is the
    kept list in its order.  The index is clamped to the mask (detector keypoints never need it)."""
    m = np.asarray(mask)
    if m.ndim != 2 or m.dtype != np.uint8:
        raise ValueError("mask must be a 2-D uint8 array")
    xs = np.asarray(x, np.float32).reshape(-1)
    ys = np.asarray(y, np.float32).reshape(-1)
    if len(xs) != len(ys):
        raise ValueError("x and y differ in length")
    ix = np.clip((xs + np.float32(0.5)).astype(np.int32), 0, m.shape[1] - 1)
    iy = np.clip((ys + np.float32(0.5)).astype(np.int32), 0, m.shape[0] - 1)
    return m[iy, ix] != 0


def descriptor_matrix(descriptors: np.ndarray, num_pts: int) -> np.ndarray:
    """ConversionImpl.hpp:66-82: row-major 128-wide descriptors -> float32 (n, 128)."""
    d = np.asarray(descriptors).reshape(-1, 128)
    n = min(num_pts, len(d))
    return d[:n].astype(np.float32)


def dmatch_triples(match: Sequence[int]) -> List[tuple]:
    """Conversion.cc:44-58: (queryIdx, trainIdx, distance 0) for every match != -1."""
    return [(i, int(m), 0.0) for i, m in enumerate(match) if m != -1]


def to_cv_keypoints(final_kpts, final_features, size: int = -1):
    import cv2

    f = keypoint_fields(final_kpts, final_features, size)
    out = []
    for i in range(len(f["x"])):
        kp = cv2.KeyPoint(float(f["x"][i]), float(f["y"][i]), float(f["size"][i]), float(f["angle"][i]),
                          float(f["response"][i]), int(f["octave"][i]))
        out.append(kp)
    return out


def to_cv_dmatches(match: Sequence[int]):
    import cv2

    return [cv2.DMatch(q, t, d) for q, t, d in dmatch_triples(match)]
