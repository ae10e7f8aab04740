"""OpenCV interop, mirroring the reference's
cvUtils/Conversion.hh:12-70 (``OpencvUtils::localKptToCvKpt``,
``descriptorToCvMat``, ``cvtMatchToDMatch``).  The field mapping is plain
numpy so it is usable (and tested) without OpenCV; the ``cv2`` object builders
import cv2 lazily and raise ImportError where OpenCV is absent.
``filter_matches`` is the match-list rule (cross check, ratio test, distance
cap; ``sift_amd.matchList``) on the host; ``gate_mask`` and ``guided_top2``
are the guided-matching rule (``sift_amd.matchListGuided``) there.
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


def rootsift(desc) -> np.ndarray:
    """The RootSIFT rule of include/sift_hip.h in numpy (Detector(root_sift=True), sift_amd.rootsift_device): rows of
    128 values -> uint8 (n, 128).  b = clip(rint(v), 0, 255) with NaN -> 0 (the identity on descriptor bytes); s = the
    row's integer sum; out = min(255, rint(512 * sqrt(b / s))) in float32 -- one correctly rounded division, one
    correctly rounded square root -- and the zero row stays zero.  The device equals this byte for byte."""
    v = np.asarray(desc)
    if v.ndim != 2 or v.shape[1] != 128:
        raise ValueError(f"rows of 128 values expected, got shape {v.shape}")
    with np.errstate(invalid="ignore"):
        b = np.clip(np.rint(np.nan_to_num(v.astype(np.float32), nan=0.0, posinf=255.0, neginf=0.0)), 0, 255).astype(np.int32)
    s = b.sum(axis=1, keepdims=True)
    q = b.astype(np.float32) / np.maximum(s, 1).astype(np.float32)  # s == 0: b is all zero
    r = np.sqrt(q, dtype=np.float32)
    return np.minimum(np.rint(np.float32(512) * r), np.float32(255)).astype(np.uint8)


def descriptor_matrix(descriptors: np.ndarray, num_pts: int) -> np.ndarray:
    """ConversionImpl.hpp:66-82: row-major 128-wide descriptors -> float32 (n, 128)."""
    d = np.asarray(descriptors).reshape(-1, 128)
    n = min(num_pts, len(d))
    return d[:n].astype(np.float32)


def dmatch_triples(match: Sequence[int]) -> List[tuple]:
    """Conversion.cc:44-58: (queryIdx, trainIdx, distance 0) for every match != -1."""
    return [(i, int(m), 0.0) for i, m in enumerate(match) if m != -1]


def _ratio_pass(idx2: np.ndarray, d2: np.ndarray, ratio, ratio_on_squared: bool) -> np.ndarray:
    """The ratio test of sift_hip_match_device's `match` output, per row of a top-2 array, in float32."""
    a1, a2 = idx2[:, 0], idx2[:, 1]
    r = np.float32(ratio)
    if not r > 0:
        return a1 >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        if ratio_on_squared:
            test = d2[:, 0] < r * d2[:, 1]
        else:
            test = np.sqrt(d2[:, 0]) < r * np.sqrt(d2[:, 1])
    return (a1 >= 0) & ((a2 < 0) | test)


def filter_matches(idx2_fwd, d2_fwd, idx2_rev=None, d2_rev=None, ratio: float = 0.8, ratio_on_squared: bool = False,
                   ratio_both_ways: bool = False, max_distance: float = 0.0, cross_check: bool = True,
                   img_idx: int = 0) -> np.ndarray:
    """The match-list rule of include/sift_hip.h (Matcher.match_list_*, matchList) in numpy, float32 arithmetic: the
    reference the tests hold the device operation to.

    idx2_fwd / d2_fwd: (nq, 2) top-2 train indices (-1: none) and squared distances of every query, as
    Matcher.match_device(Q, T) writes them; idx2_rev / d2_rev: (nt, 2), the same for match_device(T, Q) (needed with
    cross_check or ratio_both_ways only).  Query i with forward (i1, e1, i2, e2) is kept when i1 >= 0, the ratio
    test passes on its forward pair (it passes when i2 < 0; ratio <= 0: no test; on e or on sqrt(e)),
    max_distance <= 0 or sqrt(e1) <= max_distance, with cross_check idx2_rev[i1, 0] == i, and with ratio_both_ways
    the ratio test passes on row i1 of the reverse arrays.  Returns DMATCH_DTYPE records (i, i1, img_idx, sqrt(e1))
    of the kept queries in ascending i."""
    from . import DMATCH_DTYPE

    fi = np.asarray(idx2_fwd, np.int32).reshape(-1, 2)
    fd = np.asarray(d2_fwd, np.float32).reshape(-1, 2)
    if len(fi) != len(fd):
        raise ValueError("idx2_fwd and d2_fwd differ in length")
    i1 = fi[:, 0]
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(fd[:, 0])
    keep = (i1 >= 0) & _ratio_pass(fi, fd, ratio, ratio_on_squared)
    if np.float32(max_distance) > 0:
        keep &= dist <= np.float32(max_distance)
    if cross_check or ratio_both_ways:
        if idx2_rev is None or d2_rev is None:
            raise ValueError("cross_check / ratio_both_ways need the reverse top-2 arrays")
        ri = np.asarray(idx2_rev, np.int32).reshape(-1, 2)
        rd = np.asarray(d2_rev, np.float32).reshape(-1, 2)
        if len(ri) != len(rd):
            raise ValueError("idx2_rev and d2_rev differ in length")
        if keep.any() and i1[keep].max() >= len(ri):
            raise ValueError("a forward index lies outside the reverse arrays")
        row = np.where(keep, i1, 0)  # rows of queries already dropped are not looked at
        if len(ri) == 0:
            keep &= False
        else:
            if cross_check:
                keep &= ri[row, 0] == np.arange(len(fi))
            if ratio_both_ways:
                keep &= _ratio_pass(ri, rd, ratio, ratio_on_squared)[row]
    q = np.flatnonzero(keep)
    out = np.zeros(len(q), DMATCH_DTYPE)
    out["queryIdx"], out["trainIdx"], out["imgIdx"], out["distance"] = q, i1[q], img_idx, dist[q]
    return out


KNN_MAX = 8  # SIFT_HIP_KNN_MAX


def knn(q, t, k: int):
    """The k-NN rule of include/sift_hip.h (Matcher.match_knn_*, knnMatch) in numpy: (idx int32 (nq, k), d2 float32
    (nq, k)).  Row i holds the min(k, candidates) train rows of smallest squared L2 distance to query i in ascending
    (d2, train index) order -- a stable argsort, so a tie at any rank goes to the lower train index -- and -1 / FLT_MAX
    in the remaining entries.  Sets of integers 0..255: exact int64 distances (what the device returns, as bytes).
    Otherwise float64, term by term on the values given: a train row holding NaN or an infinity is nobody's
    neighbour, a query row holding one has none (the device's general path is within its stated bound of this)."""
    if not 1 <= int(k) <= KNN_MAX:
        raise ValueError(f"k = {k} outside 1..{KNN_MAX}")
    q, t = np.asarray(q), np.asarray(t)
    nq, nt = len(q), len(t)
    q = q.reshape(nq, q.size // max(nq, 1))
    t = t.reshape(nt, t.size // max(nt, 1))
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.finfo(np.float32).max, np.float32)
    if nq == 0 or nt == 0:
        return idx, d2

    def integers(a):
        a = a.astype(np.float64)
        with np.errstate(invalid="ignore"):
            return bool(np.all(np.isfinite(a)) and np.all((a == np.rint(a)) & (a >= 0) & (a <= 255))
                        and not np.any(np.signbit(a)))

    if integers(q) and integers(t):
        qi, ti = q.astype(np.int64), t.astype(np.int64)
        D = (qi * qi).sum(1)[:, None] + (ti * ti).sum(1)[None, :] - 2 * (qi @ ti.T)
        qok, tok = np.ones(nq, bool), np.ones(nt, bool)
    else:
        qf, tf = q.astype(np.float64), t.astype(np.float64)
        qok, tok = np.isfinite(qf).all(1), np.isfinite(tf).all(1)
        D = np.empty((nq, nt), np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for i0 in range(0, nq, 16):
                D[i0:i0 + 16] = ((qf[i0:i0 + 16, None, :] - tf[None, :, :]) ** 2).sum(-1)
    cand = np.flatnonzero(tok)
    m = min(k, len(cand))
    if m:
        Dc = D[:, cand]
        order = np.argsort(Dc, axis=1, kind="stable")[:, :m]
        rows = np.flatnonzero(qok)
        idx[rows, :m] = cand[order[rows]]
        d2[rows, :m] = np.take_along_axis(Dc, order, 1)[rows].astype(np.float32)
    return idx, d2


def knn_records(idx, d2, max_distance: float = 0.0, img_idx: int = 0) -> np.ndarray:
    """The capped radius list of a k-NN table (Matcher.match_knn_list_*, matchKnnList) in numpy float32: neighbour j
    of query i is kept when idx[i, j] >= 0 and (max_distance <= 0 or sqrt(d2[i, j]) <= max_distance); DMATCH_DTYPE
    records (i, idx[i, j], img_idx, sqrt(d2[i, j])) in (queryIdx, rank) order."""
    from . import DMATCH_DTYPE

    idx = np.asarray(idx, np.int32)
    d2 = np.asarray(d2, np.float32)
    if idx.shape != d2.shape or idx.ndim != 2:
        raise ValueError("idx and d2 are (nq, k) arrays of one shape")
    if np.isnan(max_distance):
        raise ValueError("max_distance is NaN")
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(d2)
    keep = idx >= 0
    if np.float32(max_distance) > 0:
        keep &= dist <= np.float32(max_distance)
    i, j = np.nonzero(keep)  # row-major: (queryIdx, rank) order
    out = np.zeros(len(i), DMATCH_DTYPE)
    out["queryIdx"], out["trainIdx"], out["imgIdx"], out["distance"] = i, idx[i, j], img_idx, dist[i, j]
    return out


def gate_mask(q_xy, t_xy, radius) -> np.ndarray:
    """The guided-matching gate of include/sift_hip.h in numpy float32: an (nq, nt) bool array, True where train row
    t is a candidate of query i -- fabsf(tx - qx) <= radius and fabsf(ty - qy) <= radius, one float32 subtraction per
    axis and an inclusive compare.  A NaN coordinate makes its row a candidate of nothing; radius = inf is no gate.
    q_xy / t_xy: (n, >= 2) arrays with x, y in the first two columns (further columns are ignored)."""
    q = np.asarray(q_xy, np.float32).reshape(len(q_xy), -1)[:, :2]
    t = np.asarray(t_xy, np.float32).reshape(len(t_xy), -1)[:, :2]
    r = np.float32(radius)
    with np.errstate(invalid="ignore"):
        dx = np.abs(t[None, :, 0] - q[:, None, 0])
        dy = np.abs(t[None, :, 1] - q[:, None, 1])
        return (dx <= r) & (dy <= r)


def epipolar_mask(q_xy, t_xy, F, max_error, radius=np.inf) -> np.ndarray:
    """The epipolar gate of include/sift_hip.h in numpy float32: an (nq, nt) bool array, True where train row t is a
    candidate of query i.  F: 9 floats, row-major, x_train^T F x_query = 0.  Every operation is one float32 operation
    rounded to nearest, in the header's order (numpy fuses nothing):
        per query   a = (F00 qx + F01 qy) + F02, b = (F10 qx + F11 qy) + F12, c = (F20 qx + F21 qy) + F22, nq = a a + b b
        per train   u = (F00 tx + F10 ty) + F20, v = (F01 tx + F11 ty) + F21, nr = u u + v v
        per pair    r = (a tx + b ty) + c;  candidate when r r <= (max_error max_error) (nq + nr) and gate_mask(radius)
    -- the Sampson distance <= max_error, inclusive.  A NaN anywhere is a candidate of nothing."""
    q = np.asarray(q_xy, np.float32).reshape(len(q_xy), -1)[:, :2]
    t = np.asarray(t_xy, np.float32).reshape(len(t_xy), -1)[:, :2]
    f = np.asarray(F, np.float32).reshape(-1)
    if f.size != 9:
        raise ValueError("F must have 9 entries (3 x 3, row-major)")
    e = np.float32(max_error)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        qx, qy, tx, ty = q[:, 0], q[:, 1], t[:, 0], t[:, 1]
        a = (f[0] * qx + f[1] * qy) + f[2]
        b = (f[3] * qx + f[4] * qy) + f[5]
        c = (f[6] * qx + f[7] * qy) + f[8]
        nq = a * a + b * b
        u = (f[0] * tx + f[3] * ty) + f[6]
        v = (f[1] * tx + f[4] * ty) + f[7]
        nr = u * u + v * v
        r = (a[:, None] * tx[None, :] + b[:, None] * ty[None, :]) + c[:, None]
        e2 = e * e
        band = r * r <= e2 * (nq[:, None] + nr[None, :])
    assert r.dtype == np.float32 and nq.dtype == np.float32 and nr.dtype == np.float32
    return band & gate_mask(q, t, radius)


def geometry_usable(F) -> bool:
    """The device-side rule of the batched epipolar calls (include/sift_hip.h): a pair's nine floats are usable when
    every one is finite and not all are zero (-0 counts as zero).  The single-pair calls refuse an F that fails this
    on the host; a batched call reads F on the device, where a pair that fails it has no candidates at all -- every
    query -1 / FLT_MAX, an empty list -- instead of epipolar_mask's formula (under which a zero F passes every row).
    The empty verify result (hypothesis = -1, F all zero) is the case it exists for."""
    f = np.asarray(F, np.float32).reshape(-1)
    if f.size != 9:
        raise ValueError("F must have 9 entries (3 x 3, row-major)")
    return bool(np.isfinite(f).all() and (f != 0).any())


def mask_top2(q, t, cand):
    """The top-2 of a candidate mask: (idx2, d2), (nq, 2) int32 / float32 laid out as match_device writes them -- the
    two nearest rows of t among cand[i] for every row i of q, ties to the lower train index, -1 / FLT_MAX where there
    is none.  Squared distances come from an exact integer product when both sets hold integers, otherwise from
    float64 as |q|^2 + |t|^2 - 2 q.t, rounded to float32 once: exact (and compared byte for byte) where every product
    and sum is representable, as for multiples of 0.5; for values where fp32 rounds it is the reference of a toleranced
    comparison only (the bound of include/sift_hip.h; tests/general_cases.py sums (q_k - t_k)^2 instead, which is 0
    for identical rows).  cand: the (nq, nt) bool array, or a function returning it, called only when neither set is
    empty."""
    q, t = np.asarray(q), np.asarray(t)
    nq, nt = len(q), len(t)
    idx2 = np.full((nq, 2), -1, np.int32)
    d2 = np.full((nq, 2), np.finfo(np.float32).max, np.float32)
    if nq == 0 or nt == 0:
        return idx2, d2
    exact = np.int64 if (np.all(q == np.rint(q)) and np.all(t == np.rint(t))) else np.float64
    a, b = q.astype(exact), t.astype(exact)
    dist = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    cand = np.asarray(cand() if callable(cand) else cand, bool)
    if cand.shape != dist.shape:
        raise ValueError("positions and descriptor sets differ in length")
    order = np.argsort(np.where(cand, dist, np.inf), axis=1, kind="stable")[:, :2]  # stable: ties to the lower index
    rows = np.arange(nq)
    for k in range(order.shape[1]):
        j = order[:, k]
        ok = cand[rows, j]
        idx2[ok, k] = j[ok]
        d2[ok, k] = dist[rows, j][ok]
    return idx2, d2


def guided_top2(q, t, q_xy, t_xy, radius):
    """Matcher.match_guided_device in numpy: the top-2 (mask_top2) of every query among its candidates (gate_mask).
    filter_matches consumes the output unchanged."""
    return mask_top2(q, t, lambda: gate_mask(q_xy, t_xy, radius))


def epipolar_top2(q, t, q_xy, t_xy, F, max_error, radius=np.inf):
    """Matcher.match_epipolar_device in numpy: the top-2 (mask_top2) of every query among its candidates
    (epipolar_mask).  The reverse direction of a cross check is epipolar_top2(t, q, t_xy, q_xy, F^T, ...)."""
    return mask_top2(q, t, lambda: epipolar_mask(q_xy, t_xy, F, max_error, radius))


def mask_knn(q, t, cand, k: int):
    """knn restricted to a candidate mask -- the gated k-NN rule of include/sift_hip.h, and cv::DescriptorMatcher::
    knnMatch(query, train, k, mask): (idx int32 (nq, k), d2 float32 (nq, k)).  Row i holds the min(k, |cand[i]|) rows
    of t among cand[i] of smallest squared L2 distance to row i of q, in ascending (d2, train index) order (a stable
    argsort: a tie at any rank goes to the lower train index), -1 / FLT_MAX in the remaining entries.  Sets of
    integers go through the exact int64 product; otherwise float64 as |q|^2 + |t|^2 - 2 q.t (mask_top2's form),
    rounded to float32 once, so exactly representable inputs compare byte for byte; a train row holding NaN or an
    infinity is nobody's neighbour and a query row holding one has none.  cand: the (nq, nt) bool array, or a function
    returning it, called only when neither set is empty."""
    if not 1 <= int(k) <= KNN_MAX:
        raise ValueError(f"k = {k} outside 1..{KNN_MAX}")
    q, t = np.asarray(q), np.asarray(t)
    nq, nt = len(q), len(t)
    q = q.reshape(nq, q.size // max(nq, 1))
    t = t.reshape(nt, t.size // max(nt, 1))
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.finfo(np.float32).max, np.float32)
    if nq == 0 or nt == 0:
        return idx, d2
    qok, tok = np.isfinite(q.astype(np.float64)).all(1), np.isfinite(t.astype(np.float64)).all(1)
    with np.errstate(invalid="ignore"):
        integers = bool(qok.all() and tok.all() and np.all(q == np.rint(q)) and np.all(t == np.rint(t)))
    a, b = (q.astype(np.int64), t.astype(np.int64)) if integers else (q.astype(np.float64), t.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        dist = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    cand = np.asarray(cand() if callable(cand) else cand, bool)
    if cand.shape != dist.shape:
        raise ValueError("positions and descriptor sets differ in length")
    cand = cand & qok[:, None] & tok[None, :]
    order = np.argsort(np.where(cand, dist, np.inf), axis=1, kind="stable")[:, :k]  # stable: ties to the lower index
    rows = np.arange(nq)
    for j in range(order.shape[1]):
        col = order[:, j]
        ok = cand[rows, col]
        idx[ok, j] = col[ok]
        d2[ok, j] = dist[rows, col][ok]
    return idx, d2


def guided_knn(q, t, q_xy, t_xy, radius, k: int):
    """Matcher.match_knn_guided_device in numpy: mask_knn of every query among its candidates (gate_mask).
    knn_records turns the table into the list of Matcher.match_knn_list_guided_*."""
    return mask_knn(q, t, lambda: gate_mask(q_xy, t_xy, radius), k)


def epipolar_knn(q, t, q_xy, t_xy, F, max_error, k: int, radius=np.inf):
    """Matcher.match_knn_epipolar_device in numpy: mask_knn of every query among its candidates (epipolar_mask).  A
    batched call's pair whose geometry record is not usable (geometry_usable) has no candidates instead."""
    return mask_knn(q, t, lambda: epipolar_mask(q_xy, t_xy, F, max_error, radius), k)


# --- Two-view verification: the rule of sift_hip_verify_* (include/sift_hip.h) in numpy float32.  Every function
# below works on whole arrays of hypotheses at once; each array operation is one float32 operation per element, rounded
# to nearest, in the header's order (numpy fuses nothing), so the device's bytes are the reference's.

_F32 = np.float32
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(h):
    """lowbias32 on uint32 values held in uint64 arrays (no overflow warnings)."""
    h = np.asarray(h, np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & _M32
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & _M32
    return h ^ (h >> np.uint64(16))


def _samples(n: int, K: int, seed: int, m: int) -> np.ndarray:
    """The sampler of the verify rules: (K, m) int32, row k the m distinct indices of [0, n) hypothesis k draws -- a
    function of (seed, k, n) only.  n < m: every entry -1 (nothing is drawn)."""
    out = np.full((K, m), -1, np.int64)
    if n < m:
        return out.astype(np.int32)
    base = _mix32(np.uint64(int(seed) & 0xFFFFFFFF) ^ _mix32(np.arange(K, dtype=np.uint64)))
    for j in range(m):
        h = _mix32((base + np.uint64((0x9E3779B9 * (j + 1)) & 0xFFFFFFFF)) & _M32)
        r = ((h * np.uint64(n - j)) >> np.uint64(32)).astype(np.int64)
        earlier = np.sort(out[:, :j], axis=1)
        for i in range(j):
            r = r + (r >= earlier[:, i])
        out[:, j] = r
    return out.astype(np.int32)


def ransac_samples(n: int, K: int, seed: int = 0) -> np.ndarray:
    """The sampler of the fundamental rule: (K, 8) int32, row k the 8 distinct indices of [0, n) hypothesis k draws --
    a function of (seed, k, n) only.  n < 8: every entry -1 (nothing is drawn)."""
    return _samples(n, K, seed, 8)


def _normalise(x, y):
    """Hartley normalisation of (K, m) coordinates: (x', y', s, ox, oy, mx, my), sums in index order."""
    m = x.shape[1]
    sx, sy = x[:, 0].copy(), y[:, 0].copy()
    for i in range(1, m):
        sx = sx + x[:, i]
        sy = sy + y[:, i]
    mx, my = sx / _F32(m), sy / _F32(m)
    dx, dy = x - mx[:, None], y - my[:, None]
    d = np.sqrt(dx * dx + dy * dy)
    sd = d[:, 0].copy()
    for i in range(1, m):
        sd = sd + d[:, i]
    md = sd / _F32(m)
    s = _F32(1.41421354) / md
    return dx * s[:, None], dy * s[:, None], s, -(s * mx), -(s * my), mx, my


def _solve_8x9(A):
    """The shared solver of both rules on (K, 8, 9) systems (changed in place): Gaussian elimination with full
    pivoting, back-substitution with the free variable y[8] = 1, the permutation undone.  (g (K, 9), ok (K,)): ok is
    False where a pivot was zero or non-finite."""
    K = len(A)
    ar = np.arange(K)
    perm = np.tile(np.arange(9), (K, 1))
    ok = np.ones(K, bool)
    for c in range(8):
        mag = np.abs(A[:, c:, c:]).reshape(K, -1)
        flat = np.argmax(np.where(np.isnan(mag), _F32(-1), mag), axis=1)  # the first of the largest, row-major
        flat = np.where(np.isnan(mag[:, 0]), 0, flat)  # nothing is larger than a NaN at (c, c)
        pr, pc = c + flat // (9 - c), c + flat % (9 - c)
        tmp = A[ar, c, :].copy()
        A[ar, c, :] = A[ar, pr, :]
        A[ar, pr, :] = tmp
        tmp = A[ar, :, c].copy()
        A[ar, :, c] = A[ar, :, pc]
        A[ar, :, pc] = tmp
        tmp = perm[ar, c].copy()
        perm[ar, c] = perm[ar, pc]
        perm[ar, pc] = tmp
        p = A[:, c, c]
        ok &= (p != 0) & np.isfinite(p)
        m = A[:, c + 1:, c] / p[:, None]
        A[:, c + 1:, c + 1:] = A[:, c + 1:, c + 1:] - m[:, :, None] * A[:, c:c + 1, c + 1:]
    y = np.zeros((K, 9), np.float32)
    y[:, 8] = 1
    for i in range(7, -1, -1):
        acc = A[:, i, i + 1] * y[:, i + 1]
        for j in range(i + 2, 9):
            acc = acc + A[:, i, j] * y[:, j]
        y[:, i] = (-acc) / A[:, i, i]
    g = np.zeros((K, 9), np.float32)
    g[ar[:, None], perm] = y
    assert A.dtype == np.float32 and y.dtype == np.float32
    return g, ok


def fundamental_from_8(q_xy8, t_xy8):
    """The solver of the verify rule: the normalised 8-point F of 8 pairs (Gaussian elimination with full pivoting, no
    rank-2 constraint, unit Frobenius norm).  q_xy8 / t_xy8: (8, 2) -> (F (9,) float32, valid bool), or (K, 8, 2) ->
    (F (K, 9), valid (K,)).  An invalid hypothesis (a zero or non-finite pivot or result) has F all zero."""
    q = np.asarray(q_xy8, np.float32)
    t = np.asarray(t_xy8, np.float32)
    single = q.ndim == 2
    q, t = q.reshape(-1, 8, 2), t.reshape(-1, 8, 2)
    K = len(q)
    with np.errstate(all="ignore"):
        qx, qy, sq, oqx, oqy, _, _ = _normalise(q[:, :, 0], q[:, :, 1])
        tx, ty, st, otx, oty, _, _ = _normalise(t[:, :, 0], t[:, :, 1])
        A = np.stack([tx * qx, tx * qy, tx, ty * qx, ty * qy, ty, qx, qy, np.ones_like(qx)], axis=2)  # (K, 8, 9)
        g, ok = _solve_8x9(A)
        G = g.reshape(K, 3, 3)
        H = np.zeros((K, 3, 3), np.float32)
        H[:, :, 0] = G[:, :, 0] * sq[:, None]
        H[:, :, 1] = G[:, :, 1] * sq[:, None]
        H[:, :, 2] = (G[:, :, 0] * oqx[:, None] + G[:, :, 1] * oqy[:, None]) + G[:, :, 2]
        F = np.zeros((K, 3, 3), np.float32)
        F[:, 0, :] = st[:, None] * H[:, 0, :]
        F[:, 1, :] = st[:, None] * H[:, 1, :]
        F[:, 2, :] = (otx[:, None] * H[:, 0, :] + oty[:, None] * H[:, 1, :]) + H[:, 2, :]
        F = F.reshape(K, 9)
        ss = F[:, 0] * F[:, 0]
        for i in range(1, 9):
            ss = ss + F[:, i] * F[:, i]
        F = F / np.sqrt(ss)[:, None]
        ok &= np.isfinite(F).all(1)
    assert A.dtype == np.float32 and g.dtype == np.float32 and F.dtype == np.float32 and ss.dtype == np.float32
    F[~ok] = 0
    return (F[0], bool(ok[0])) if single else (F, ok)


def _match_points(matches, q_xy, t_xy) -> np.ndarray:
    """(n, 4) float32 (qx, qy, tx, ty) of a match list; NaN x 4 for a record with an index outside its array."""
    q = np.asarray(q_xy, np.float32).reshape(len(q_xy), -1)[:, :2]
    t = np.asarray(t_xy, np.float32).reshape(len(t_xy), -1)[:, :2]
    qi = np.asarray(matches["queryIdx"], np.int64)
    ti = np.asarray(matches["trainIdx"], np.int64)
    ok = (qi >= 0) & (qi < len(q)) & (ti >= 0) & (ti < len(t))
    pts = np.full((len(qi), 4), np.nan, np.float32)
    pts[ok, :2] = q[qi[ok]]
    pts[ok, 2:] = t[ti[ok]]
    return pts


def _sampson_pass(pts, F, max_error) -> np.ndarray:
    """(K, n) bool: the epipolar predicate (epipolar_mask's operations, radius = inf) of every match's own pair under
    each of the K rows of F (K, 9)."""
    f = np.asarray(F, np.float32).reshape(-1, 9)[:, :, None]
    e = np.float32(max_error)
    qx, qy, tx, ty = (pts[None, :, i] for i in range(4))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = (f[:, 0] * qx + f[:, 1] * qy) + f[:, 2]
        b = (f[:, 3] * qx + f[:, 4] * qy) + f[:, 5]
        c = (f[:, 6] * qx + f[:, 7] * qy) + f[:, 8]
        nq = a * a + b * b
        u = (f[:, 0] * tx + f[:, 3] * ty) + f[:, 6]
        v = (f[:, 1] * tx + f[:, 4] * ty) + f[:, 7]
        nr = u * u + v * v
        r = (a * tx + b * ty) + c
        band = r * r <= (e * e) * (nq + nr)
        window = (np.abs(tx - qx) <= np.float32(np.inf)) & (np.abs(ty - qy) <= np.float32(np.inf))
    assert r.dtype == np.float32 and nq.dtype == np.float32 and nr.dtype == np.float32
    return band & window


def sampson_inliers(matches, q_xy, t_xy, F, max_error) -> np.ndarray:
    """The score of the verify rule: a bool per DMATCH_DTYPE record, True where the record's own pair passes the
    epipolar predicate under F (Sampson distance <= max_error, inclusive) -- the diagonal of
    epipolar_mask(q_xy[queryIdx], t_xy[trainIdx], F, max_error), computed per pair.  A record with an index outside
    its position array, or a NaN position, is an inlier of nothing."""
    f = np.asarray(F, np.float32).reshape(-1)
    if f.size != 9:
        raise ValueError("F must have 9 entries (3 x 3, row-major)")
    return _sampson_pass(_match_points(matches, q_xy, t_xy), f, max_error)[0]


def ransac_fundamental(matches, q_xy, t_xy, max_error=1.5, K: int = 1024, seed: int = 0) -> dict:
    """The whole verify operation (sift_hip_verify_fundamental_*) in numpy.  matches: the n DMATCH_DTYPE records that
    count.  Returns a dict: F (9,) float32, inliers, hypothesis (-1: none), matches (= n), valid_hypotheses, mask (n,)
    uint8, list (the inlier records in input order), and what every hypothesis drew, solved and counted: samples
    (K, 8), Fs (K, 9), valid (K,), counts (K,)."""
    from . import DMATCH_DTYPE

    matches = np.asarray(matches, DMATCH_DTYPE)
    n = len(matches)
    pts = _match_points(matches, q_xy, t_xy)
    samples = ransac_samples(n, K, seed)
    if n >= 8:
        Fs, valid = fundamental_from_8(pts[samples][:, :, :2], pts[samples][:, :, 2:])
        passes = _sampson_pass(pts, Fs, max_error) & valid[:, None]
    else:
        Fs, valid, passes = np.zeros((K, 9), np.float32), np.zeros(K, bool), np.zeros((K, n), bool)
    counts = passes.sum(1).astype(np.int32)
    hyp = -1
    if valid.any():
        hyp = int(np.argmax(np.where(valid, counts, -1)))  # the first of the largest: ties to the lowest k
    mask = passes[hyp].astype(np.uint8) if hyp >= 0 else np.zeros(n, np.uint8)
    return dict(F=Fs[hyp].copy() if hyp >= 0 else np.zeros(9, np.float32), inliers=int(counts[hyp]) if hyp >= 0 else 0,
                hypothesis=hyp, matches=n, valid_hypotheses=int(valid.sum()), mask=mask, list=matches[mask != 0],
                samples=samples, Fs=Fs, valid=valid, counts=counts)


def fundamental_lstsq(q_pts, t_pts, rank2: bool = True) -> np.ndarray:
    """A convenience, not part of the device rule: the float64 normalised 8-point least-squares F (3 x 3, unit
    Frobenius norm, x_t^T F x_q = 0) of n >= 8 pairs through np.linalg.svd, with the rank-2 projection -- a pose-grade
    F from the inliers a verify call returns."""
    q = np.asarray(q_pts, np.float64).reshape(len(q_pts), -1)[:, :2]
    t = np.asarray(t_pts, np.float64).reshape(len(t_pts), -1)[:, :2]
    if len(q) != len(t) or len(q) < 8:
        raise ValueError("fundamental_lstsq needs the same number (>= 8) of points on both sides")

    def norm(p):
        m = p.mean(0)
        s = np.sqrt(2.0) / np.sqrt(((p - m) ** 2).sum(1)).mean()
        return (p - m) * s, np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1]])

    (qn, Tq), (tn, Tt) = norm(q), norm(t)
    A = np.stack([tn[:, 0] * qn[:, 0], tn[:, 0] * qn[:, 1], tn[:, 0], tn[:, 1] * qn[:, 0], tn[:, 1] * qn[:, 1],
                  tn[:, 1], qn[:, 0], qn[:, 1], np.ones(len(q))], 1)
    G = np.linalg.svd(A)[2][-1].reshape(3, 3)
    if rank2:
        u, s, vt = np.linalg.svd(G)
        G = u @ np.diag([s[0], s[1], 0.0]) @ vt
    F = Tt.T @ G @ Tq
    return F / np.linalg.norm(F)


# --- Homography verification: the rule of sift_hip_verify_homography_* and sift_hip_project_homography_device
# (include/sift_hip.h) in numpy float32, on the conventions above.  The model is x_train ~ H x_query, H row-major: the
# orientation of cv::findHomography(query_points, train_points).

_TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


def homography_samples(n: int, K: int, seed: int = 0) -> np.ndarray:
    """The sampler of the homography rule: (K, 4) int32, ransac_samples' draw with 4 indices in place of 8.  n < 4:
    every entry -1 (nothing is drawn)."""
    return _samples(n, K, seed, 4)


def _oriented(q, t):
    """The orientation test on raw (K, 4, 2) samples: True where the signed areas of the four point triples have, on
    both sides, products that are all > 0 or all < 0 (a collinear triple or a NaN fails both)."""
    p = []
    for i, j, k in _TRIPLES:
        a = [(s[:, j, 0] - s[:, i, 0]) * (s[:, k, 1] - s[:, i, 1]) - (s[:, j, 1] - s[:, i, 1]) * (s[:, k, 0] - s[:, i, 0])
             for s in (q, t)]
        p.append(a[0] * a[1])
    p = np.stack(p, 1)
    assert p.dtype == np.float32
    return (p > 0).all(1) | (p < 0).all(1)


def homography_from_4(q_xy4, t_xy4, max_error=None):
    """The solver of the homography rule: the normalised 4-point H of 4 pairs (the orientation test, the 8 x 9 system
    through the fundamental rule's elimination, unit Frobenius norm, the sign that makes w positive at sample 0).
    q_xy4 / t_xy4: (4, 2) -> (H (9,) float32, valid bool), or (K, 4, 2) -> (H (K, 9), valid (K,)).  An invalid
    hypothesis (a failed orientation test, a zero or non-finite pivot or result, w0 = 0) has H all zero.  With a
    max_error the rule's last step applies too, as in a verify call: a hypothesis that does not count each of its own
    four pairs under the transfer predicate is invalid."""
    q = np.asarray(q_xy4, np.float32)
    t = np.asarray(t_xy4, np.float32)
    single = q.ndim == 2
    q, t = q.reshape(-1, 4, 2), t.reshape(-1, 4, 2)
    K = len(q)
    with np.errstate(all="ignore"):
        ok = _oriented(q, t)
        x, y, sq, oqx, oqy, _, _ = _normalise(q[:, :, 0], q[:, :, 1])
        u, v, st, _, _, mtx, mty = _normalise(t[:, :, 0], t[:, :, 1])
        one, zero = np.ones_like(x), np.zeros_like(x)
        even = np.stack([x, y, one, zero, zero, zero, -(u * x), -(u * y), -u], axis=2)
        odd = np.stack([zero, zero, zero, x, y, one, -(v * x), -(v * y), -v], axis=2)
        A = np.stack([even, odd], axis=2).reshape(K, 8, 9)  # rows 2 i and 2 i + 1 belong to pair i
        g, solved = _solve_8x9(A)
        ok &= solved
        G = g.reshape(K, 3, 3)
        M = np.zeros((K, 3, 3), np.float32)
        M[:, :, 0] = G[:, :, 0] * sq[:, None]
        M[:, :, 1] = G[:, :, 1] * sq[:, None]
        M[:, :, 2] = (G[:, :, 0] * oqx[:, None] + G[:, :, 1] * oqy[:, None]) + G[:, :, 2]
        H = np.zeros((K, 3, 3), np.float32)
        H[:, 0, :] = M[:, 0, :] / st[:, None] + mtx[:, None] * M[:, 2, :]
        H[:, 1, :] = M[:, 1, :] / st[:, None] + mty[:, None] * M[:, 2, :]
        H[:, 2, :] = M[:, 2, :]
        H = H.reshape(K, 9)
        ss = H[:, 0] * H[:, 0]
        for i in range(1, 9):
            ss = ss + H[:, i] * H[:, i]
        H = H / np.sqrt(ss)[:, None]
        w0 = (H[:, 6] * q[:, 0, 0] + H[:, 7] * q[:, 0, 1]) + H[:, 8]
        H = np.where((w0 < 0)[:, None], -H, H)
        ok &= np.isfinite(H).all(1) & (w0 != 0)
        if max_error is not None:  # the own-sample rule: _transfer_pass's operations, hypothesis k on its own pair i
            e = np.float32(max_error)
            for i in range(4):
                px = (H[:, 0] * q[:, i, 0] + H[:, 1] * q[:, i, 1]) + H[:, 2]
                py = (H[:, 3] * q[:, i, 0] + H[:, 4] * q[:, i, 1]) + H[:, 5]
                w = (H[:, 6] * q[:, i, 0] + H[:, 7] * q[:, i, 1]) + H[:, 8]
                dx, dy = px - t[:, i, 0] * w, py - t[:, i, 1] * w
                ok &= (w > 0) & (dx * dx + dy * dy <= (e * e) * (w * w))
    assert A.dtype == np.float32 and g.dtype == np.float32 and H.dtype == np.float32 and ss.dtype == np.float32
    assert M.dtype == np.float32 and w0.dtype == np.float32
    H[~ok] = 0
    return (H[0], bool(ok[0])) if single else (H, ok)


def _transfer_pass(pts, H, max_error) -> np.ndarray:
    """(K, n) bool: the transfer predicate of every match (qx, qy, tx, ty) under each of the K rows of H (K, 9):
    w > 0 and dx dx + dy dy <= (max_error max_error) (w w), inclusive, with dx = px - tx w, dy = py - ty w."""
    h = np.asarray(H, np.float32).reshape(-1, 9)[:, :, None]
    e = np.float32(max_error)
    qx, qy, tx, ty = (pts[None, :, i] for i in range(4))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        px = (h[:, 0] * qx + h[:, 1] * qy) + h[:, 2]
        py = (h[:, 3] * qx + h[:, 4] * qy) + h[:, 5]
        w = (h[:, 6] * qx + h[:, 7] * qy) + h[:, 8]
        dx = px - tx * w
        dy = py - ty * w
        near = dx * dx + dy * dy <= (e * e) * (w * w)
        front = w > 0
    assert dx.dtype == np.float32 and dy.dtype == np.float32 and w.dtype == np.float32
    return front & near


def transfer_inliers(matches, q_xy, t_xy, H, max_error) -> np.ndarray:
    """The score of the homography rule: a bool per DMATCH_DTYPE record, True where the record's query position,
    carried over by H, lies in front (w > 0) and within max_error pixels of its train position (the forward transfer
    error, inclusive, division-free).  A record with an index outside its position array, or a NaN position, is an
    inlier of nothing."""
    h = np.asarray(H, np.float32).reshape(-1)
    if h.size != 9:
        raise ValueError("H must have 9 entries (3 x 3, row-major)")
    return _transfer_pass(_match_points(matches, q_xy, t_xy), h, max_error)[0]


def ransac_homography(matches, q_xy, t_xy, max_error=1.5, K: int = 1024, seed: int = 0) -> dict:
    """The whole operation (sift_hip_verify_homography_*) in numpy.  matches: the n DMATCH_DTYPE records that count.
    Returns ransac_fundamental's dict with H (9,) and Hs (K, 9) in place of F and Fs; samples is (K, 4)."""
    from . import DMATCH_DTYPE

    matches = np.asarray(matches, DMATCH_DTYPE)
    n = len(matches)
    pts = _match_points(matches, q_xy, t_xy)
    samples = homography_samples(n, K, seed)
    if n >= 4:
        Hs, valid = homography_from_4(pts[samples][:, :, :2], pts[samples][:, :, 2:], max_error)
        passes = _transfer_pass(pts, Hs, max_error) & valid[:, None]
    else:
        Hs, valid, passes = np.zeros((K, 9), np.float32), np.zeros(K, bool), np.zeros((K, n), bool)
    counts = passes.sum(1).astype(np.int32)
    hyp = -1
    if valid.any():
        hyp = int(np.argmax(np.where(valid, counts, -1)))  # the first of the largest: ties to the lowest k
    mask = passes[hyp].astype(np.uint8) if hyp >= 0 else np.zeros(n, np.uint8)
    return dict(H=Hs[hyp].copy() if hyp >= 0 else np.zeros(9, np.float32), inliers=int(counts[hyp]) if hyp >= 0 else 0,
                hypothesis=hyp, matches=n, valid_hypotheses=int(valid.sum()), mask=mask, list=matches[mask != 0],
                samples=samples, Hs=Hs, valid=valid, counts=counts)


def project_homography(H, xy) -> np.ndarray:
    """sift_hip_project_homography_device in numpy: (n, 2) float32, row i the position (px / w, py / w) that H carries
    xy[i] to, (NaN, NaN) where w is not > 0 (a zero H -- the empty result -- gives NaN everywhere: candidates of
    nothing under the window gate).  xy: (n, >= 2), x and y first."""
    h = np.asarray(H, np.float32).reshape(-1)
    if h.size != 9:
        raise ValueError("H must have 9 entries (3 x 3, row-major)")
    if len(xy) == 0:
        return np.zeros((0, 2), np.float32)
    p = np.asarray(xy, np.float32).reshape(len(xy), -1)[:, :2]
    x, y = p[:, 0], p[:, 1]
    with np.errstate(all="ignore"):
        px = (h[0] * x + h[1] * y) + h[2]
        py = (h[3] * x + h[4] * y) + h[5]
        w = (h[6] * x + h[7] * y) + h[8]
        out = np.stack([px / w, py / w], 1)
    assert out.dtype == np.float32
    out[~(w > 0)] = np.nan
    return out


def homography_lstsq(q_pts, t_pts) -> np.ndarray:
    """A convenience, not part of the device rule: the float64 normalised DLT least-squares H (3 x 3, H[2][2] = 1,
    x_t ~ H x_q) of n >= 4 pairs through np.linalg.svd -- a refit on the inliers a verify call returns."""
    q = np.asarray(q_pts, np.float64).reshape(len(q_pts), -1)[:, :2]
    t = np.asarray(t_pts, np.float64).reshape(len(t_pts), -1)[:, :2]
    if len(q) != len(t) or len(q) < 4:
        raise ValueError("homography_lstsq needs the same number (>= 4) of points on both sides")

    def norm(p):
        m = p.mean(0)
        s = np.sqrt(2.0) / np.sqrt(((p - m) ** 2).sum(1)).mean()
        return (p - m) * s, np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1]])

    (qn, Tq), (tn, Tt) = norm(q), norm(t)
    x, y, u, v = qn[:, 0], qn[:, 1], tn[:, 0], tn[:, 1]
    one, zero = np.ones(len(q)), np.zeros(len(q))
    A = np.r_[np.stack([x, y, one, zero, zero, zero, -u * x, -u * y, -u], 1),
              np.stack([zero, zero, zero, x, y, one, -v * x, -v * y, -v], 1)]
    G = np.linalg.svd(A)[2][-1].reshape(3, 3)
    H = np.linalg.inv(Tt) @ G @ Tq
    return H / H[2, 2]


# --- The refit of a verified model on its inliers: the rule of sift_hip_refine_* (include/sift_hip.h, "Refit of the
# verified model") in numpy float64.  Every operation below is one IEEE float64 operation, rounded to nearest, in the
# header's order; the nine results are rounded to float32 once.  The device performs the same operations in the same
# order, so its bytes are this code's.

REFIT_SLOTS = 256   # slot of record j: j mod 256
REFIT_SWEEPS = 8    # Jacobi sweeps, for the 9 x 9 and the 3 x 3 problem alike
REFIT_MAX_ROUNDS = 8
_SQRT2 = np.float64(1.4142135623730951)


def _slot_sum(v, fit):
    """The one summation order of the refit rule, for the columns of v (n, c) float64 over the records fit marks:
    record j belongs to slot j mod 256; a slot adds its fit records to +0 in ascending j; the 64 slots of each of the
    four groups [64 g, 64 g + 64) combine by a halving tree (slot i += slot i + d, d = 32, 16 .. 1, i mod 64 < d);
    the total is (g0 + g1) + (g2 + g3).  A record that is not fit adds nothing (as +0 it changes no sum)."""
    return _slot_sum_rows([np.asarray(v, np.float64)], fit)


def _jacobi_pivots(m: int):
    """The pivot order of one sweep for odd m: round r = 0 .. m - 1 holds the pivots ((r + i) mod m, (r - i) mod m),
    i = 1 .. (m - 1) / 2, each written (p, q) with p < q.  Every index pair occurs once per sweep; the pairs of a round
    are disjoint, and index r rests."""
    return [[tuple(sorted(((r + i) % m, (r - i) % m))) for i in range(1, (m - 1) // 2 + 1)] for r in range(m)]


def _jacobi_full(A, sweeps: int = REFIT_SWEEPS):
    """Cyclic Jacobi on a symmetric (m, m) float64 matrix, m odd: `sweeps` sweeps over the pivots in round-robin order
    (_jacobi_pivots: m rounds of (m - 1) / 2 pivots on disjoint index pairs, which a device applies side by side -- a
    rotation reads nothing an earlier rotation of its round wrote but the entries it shares with it, and those in
    this order); a pivot whose entry is exactly 0 is skipped.  The rotation, with a = A[p][q]:
        theta = (A[q][q] - A[p][p]) / (2 a);  t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0;
        c = 1 / sqrt(t t + 1);  s = t c;
        k != p, q:  A[k][p] = A[p][k] = c A[k][p] - s A[k][q],  A[k][q] = A[q][k] = s A[k][p] + c A[k][q] (old values);
        A[p][p] -= t a;  A[q][q] += t a;  A[p][q] = A[q][p] = 0;
        every k:  V[k][p] = c V[k][p] - s V[k][q],  V[k][q] = s V[k][p] + c V[k][q] (old values), V = I at the start.
    Returns V as m rows of Python floats (column i: the eigenvector of diagonal entry i) and the diagonal."""
    m = len(A)
    A = [[float(A[r][c]) for c in range(m)] for r in range(m)]
    V = [[1.0 if r == c else 0.0 for c in range(m)] for r in range(m)]
    for _ in range(sweeps):
        for rnd in _jacobi_pivots(m):
            for p, q in rnd:
                a = A[p][q]
                if a == 0.0:
                    continue
                theta = np.float64(A[q][q] - A[p][p]) / np.float64(2.0 * a)  # numpy: x / 0 and inf pass silently
                theta = float(theta)
                root = float(np.sqrt(np.float64(theta * theta + 1.0)))
                t = 1.0 / (abs(theta) + root)
                if theta < 0.0:
                    t = -t
                c = 1.0 / float(np.sqrt(np.float64(t * t + 1.0)))
                s = t * c
                for k in range(m):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                A[p][p] = A[p][p] - t * a
                A[q][q] = A[q][q] + t * a
                A[p][q] = A[q][p] = 0.0
                for k in range(m):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return V, [A[i][i] for i in range(m)]


def _jacobi(A, sweeps: int = REFIT_SWEEPS):
    """_jacobi_full's column of V whose diagonal entry of A is the smallest (ties to the lowest index) -- the
    eigenvector of the smallest eigenvalue -- and the diagonal."""
    V, d = _jacobi_full(A, sweeps)
    m = len(d)
    best = 0
    for i in range(1, m):
        if d[i] < d[best]:
            best = i
    return np.array([V[k][best] for k in range(m)], np.float64), np.array(d, np.float64)


def _refit_points(pts_or_matches, q_xy, t_xy):
    a = np.asarray(pts_or_matches)
    if a.dtype.names:
        return _match_points(a, q_xy, t_xy)
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("points must be (n, 4): qx, qy, tx, ty")
    return a


def _refit(model: str, pts, mask, sweeps: int = REFIT_SWEEPS, detail: bool = False):
    """One fit of the refit rule on gathered points (n, 4) float32 and their mask: (model (9,) float32, valid)."""
    assert pts.dtype == np.float32
    n = len(pts)
    mask = np.asarray(mask).reshape(-1)[:n]
    if len(mask) != n:
        raise ValueError("one mask byte per record")
    need = 8 if model == "F" else 4
    zero = np.zeros(9, np.float32)
    fit = (mask != 0) & np.isfinite(pts).all(1)
    m = int(fit.sum())
    if m < need:
        return (zero, False, None) if detail else (zero, False)
    p = pts.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = _slot_sum(p, fit) / np.float64(m)                       # (mqx, mqy, mtx, mty)
        d = p - mean
        dist = np.stack([np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]), np.sqrt(d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3])], 1)
        md = _slot_sum(dist, fit) / np.float64(m)
        sq, st = _SQRT2 / md[0], _SQRT2 / md[1]
        if not (np.isfinite(sq) and np.isfinite(st)):
            return (zero, False, None) if detail else (zero, False)
        x, y, u, v = d[:, 0] * sq, d[:, 1] * sq, d[:, 2] * st, d[:, 3] * st
        one, nil = np.ones(n), np.zeros(n)
        if model == "F":
            rows = [np.stack([u * x, u * y, u, v * x, v * y, v, x, y, one], 1)]
        else:
            rows = [np.stack([x, y, one, nil, nil, nil, -(u * x), -(u * y), -u], 1),
                    np.stack([nil, nil, nil, x, y, one, -(v * x), -(v * y), -v], 1)]
        iu = [(r, c) for r in range(9) for c in range(r, 9)]
        # a record adds its rows' products one row after the other; a product of a structural zero adds nothing
        if len(rows) == 1:
            terms = np.stack([rows[0][:, r] * rows[0][:, c] for r, c in iu], 1)
            sums = _slot_sum(terms, fit)
        else:
            sums = _slot_sum_rows([np.stack([a[:, r] * a[:, c] for r, c in iu], 1) for a in rows], fit)
        M = np.zeros((9, 9), np.float64)
        for (r, c), s in zip(iu, sums):
            M[r, c] = M[c, r] = s
        g, _ = _jacobi(M, sweeps)
        G = g.reshape(3, 3).copy()
        if model == "F":
            GtG = np.zeros((3, 3), np.float64)
            for r in range(3):
                for c in range(r, 3):
                    GtG[r, c] = GtG[c, r] = (G[0, r] * G[0, c] + G[1, r] * G[1, c]) + G[2, r] * G[2, c]
            v3, _ = _jacobi(GtG, sweeps)
            Gv = [(G[r, 0] * v3[0] + G[r, 1] * v3[1]) + G[r, 2] * v3[2] for r in range(3)]
            for r in range(3):
                for c in range(3):
                    G[r, c] = G[r, c] - Gv[r] * v3[c]
        oqx, oqy = -(sq * mean[0]), -(sq * mean[1])
        T = np.zeros((3, 3), np.float64)
        T[:, 0] = G[:, 0] * sq
        T[:, 1] = G[:, 1] * sq
        T[:, 2] = (G[:, 0] * oqx + G[:, 1] * oqy) + G[:, 2]
        R = np.zeros((3, 3), np.float64)
        if model == "F":
            otx, oty = -(st * mean[2]), -(st * mean[3])
            R[0] = st * T[0]
            R[1] = st * T[1]
            R[2] = (otx * T[0] + oty * T[1]) + T[2]
        else:
            R[0] = T[0] / st + mean[2] * T[2]
            R[1] = T[1] / st + mean[3] * T[2]
            R[2] = T[2]
        R = R.reshape(9)
        ss = R[0] * R[0]
        for i in range(1, 9):
            ss = ss + R[i] * R[i]
        R = R / np.sqrt(ss)
        ok = True
        if model == "H":
            j0 = int(np.flatnonzero(fit)[0])
            w0 = (R[6] * p[j0, 0] + R[7] * p[j0, 1]) + R[8]
            if w0 < 0:
                R = -R
            ok = bool(w0 != 0)
        out = R.astype(np.float32)
        ok = ok and bool(np.isfinite(out).all())
    assert M.dtype == np.float64 and R.dtype == np.float64 and out.dtype == np.float32
    if not ok:
        out = zero
    return (out, ok, G) if detail else (out, ok)


def _slot_sum_rows(terms, fit):
    """_slot_sum where a record adds several terms to its slot one after the other (the homography's two rows): the
    slot's order is record by record in ascending j, and within a record term by term."""
    n, c = terms[0].shape
    k = len(terms)
    inter = np.stack(terms, 1)  # (n, k, c): record j's terms in order
    rows = -(-max(n, 1) // REFIT_SLOTS)
    pad = np.zeros((rows * REFIT_SLOTS, k, c), np.float64)
    pad[:n] = np.where(np.asarray(fit, bool)[:, None, None], inter, 0.0)
    pad = pad.reshape(rows, REFIT_SLOTS, k, c)
    slots = np.zeros((REFIT_SLOTS, c), np.float64)
    for r in range(rows):
        for i in range(k):
            slots = slots + pad[r, :, i]
    g = slots.reshape(4, 64, c)
    d = 32
    while d >= 1:
        g = g[:, :d] + g[:, d:2 * d]
        d //= 2
    g = g[:, 0]
    return (g[0] + g[1]) + (g[2] + g[3])


def refit_fundamental(pts_or_matches, q_xy=None, t_xy=None, mask=None):
    """One fit of the refit rule (include/sift_hip.h) for the fundamental matrix: the least-squares, rank-2 F of the
    records mask marks, (F (9,) float32 of unit norm, valid).  pts_or_matches: gathered points (n, 4) float32 (qx, qy,
    tx, ty; q_xy and t_xy are then ignored), or DMATCH_DTYPE records with their position arrays.  An invalid fit
    (fewer than 8 fit records, a degenerate normalisation, a non-finite result) has F all zero."""
    pts = _refit_points(pts_or_matches, q_xy, t_xy)
    return _refit("F", pts, np.ones(len(pts), np.uint8) if mask is None else mask)


def refit_homography(pts_or_matches, q_xy=None, t_xy=None, mask=None):
    """refit_fundamental for the homography: the least-squares H of the records mask marks (at least 4), of unit norm
    and with w > 0 at the first fit record; w = 0 there is invalid."""
    pts = _refit_points(pts_or_matches, q_xy, t_xy)
    return _refit("H", pts, np.ones(len(pts), np.uint8) if mask is None else mask)


def _refine(model, passes, matches, q_xy, t_xy, result, max_error, rounds):
    from . import DMATCH_DTYPE

    if not 1 <= int(rounds) <= REFIT_MAX_ROUNDS:
        raise ValueError("rounds must lie in 1..8")
    matches = np.asarray(matches, DMATCH_DTYPE)
    n = len(matches)
    out = dict(result)
    cur = np.asarray(result[model], np.float32).reshape(9).copy()
    mask = np.asarray(result["mask"], np.uint8).reshape(-1)[:n].copy()
    if len(mask) != n:
        raise ValueError("one mask byte per record")
    inliers = int(result["inliers"])
    accepted = 0
    pts = _match_points(matches, q_xy, t_xy)
    if int(result["hypothesis"]) >= 0 and geometry_usable(cur):
        for _ in range(int(rounds)):
            cand, ok = _refit(model, pts, mask)
            if not ok:
                break  # the state is unchanged, so every later round fails the same way
            keep = passes(pts, cand, max_error)[0]
            if int(keep.sum()) < inliers:
                break
            cur, mask, inliers = cand, keep.astype(np.uint8), int(keep.sum())
            accepted += 1
    assert cur.dtype == np.float32 and mask.dtype == np.uint8
    out[model], out["mask"], out["inliers"], out["list"] = cur, mask, inliers, matches[mask != 0]
    out["accepted"] = accepted
    return out


def refine_fundamental(matches, q_xy, t_xy, result, max_error=1.5, rounds: int = 1) -> dict:
    """The whole refit operation (sift_hip_refine_fundamental_*) in numpy, on a ransac_fundamental dict (read: F,
    inliers, hypothesis, mask): `rounds` rounds of fit -> rescore -> accept.  Returns the dict with F, inliers, mask
    and list updated and `accepted`, the number of accepted rounds; every other entry is the input's."""
    return _refine("F", _sampson_pass, matches, q_xy, t_xy, result, max_error, rounds)


def refine_homography(matches, q_xy, t_xy, result, max_error=1.5, rounds: int = 1) -> dict:
    """refine_fundamental for a ransac_homography dict (sift_hip_refine_homography_*)."""
    return _refine("H", _transfer_pass, matches, q_xy, t_xy, result, max_error, rounds)


# --- Affine and similarity verification: the rule of sift_hip_verify_affine_* / sift_hip_refine_affine_*
# (include/sift_hip.h, "Affine and similarity verification") in numpy, on the conventions above: the minimal solve and
# the score in float32, the refit in float64, one rounded operation per array operation in the header's order.  The
# model is x_train = A x_query + t, stored as the nine floats {a, b, tx, c, d, ty, 0, 0, 1} -- a homography record.


def affine_samples(n: int, K: int, seed: int = 0) -> np.ndarray:
    """The sampler of the affine rule: (K, 3) int32, ransac_samples' draw with 3 indices.  n < 3: every entry -1."""
    return _samples(n, K, seed, 3)


def similarity_samples(n: int, K: int, seed: int = 0) -> np.ndarray:
    """The sampler of the similarity rule: (K, 2) int32, ransac_samples' draw with 2 indices.  n < 2: every entry -1."""
    return _samples(n, K, seed, 2)


def _affine_rows(a, b, c, d, q0, t0, ok):
    """The nine floats of (K,) matrix entries and the first sample (K, 2) each side; invalid rows all zero."""
    tx = t0[:, 0] - (a * q0[:, 0] + b * q0[:, 1])
    ty = t0[:, 1] - (c * q0[:, 0] + d * q0[:, 1])
    zero, one = np.zeros_like(a), np.ones_like(a)
    A = np.stack([a, b, tx, c, d, ty, zero, zero, one], 1)
    assert A.dtype == np.float32
    ok = ok & np.isfinite(A).all(1)
    A[~ok] = 0
    return A, ok


def affine_from_3(q_xy3, t_xy3):
    """The solver of the affine rule: the map through 3 pairs, in closed form on the raw coordinates.  q_xy3 / t_xy3:
    (3, 2) -> (A (9,) float32, valid bool), or (K, 3, 2) -> (A (K, 9), valid (K,)).  An invalid hypothesis (a collinear
    triple or a repeated position on either side, a NaN, a non-finite entry) has A all zero; a reflection is valid."""
    q = np.asarray(q_xy3, np.float32)
    t = np.asarray(t_xy3, np.float32)
    single = q.ndim == 2
    q, t = q.reshape(-1, 3, 2), t.reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        d1, d2, e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
        dett = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        p = det * dett
        ok = (p > 0) | (p < 0)
        a = (e1[:, 0] * d2[:, 1] - e2[:, 0] * d1[:, 1]) / det
        b = (e2[:, 0] * d1[:, 0] - e1[:, 0] * d2[:, 0]) / det
        c = (e1[:, 1] * d2[:, 1] - e2[:, 1] * d1[:, 1]) / det
        d = (e2[:, 1] * d1[:, 0] - e1[:, 1] * d2[:, 0]) / det
        A, ok = _affine_rows(a, b, c, d, q[:, 0], t[:, 0], ok)
    assert p.dtype == np.float32
    return (A[0], bool(ok[0])) if single else (A, ok)


def similarity_from_2(q_xy2, t_xy2):
    """The solver of the similarity rule: the rotation, scale and translation through 2 pairs, [a, -b, tx; b, a, ty].
    q_xy2 / t_xy2: (2, 2) -> (A (9,) float32, valid bool), or (K, 2, 2) -> (A (K, 9), valid (K,)).  An invalid
    hypothesis (a repeated position on either side, a NaN, a non-finite entry) has A all zero."""
    q = np.asarray(q_xy2, np.float32)
    t = np.asarray(t_xy2, np.float32)
    single = q.ndim == 2
    q, t = q.reshape(-1, 2, 2), t.reshape(-1, 2, 2)
    with np.errstate(all="ignore"):
        dq, dt = q[:, 1] - q[:, 0], t[:, 1] - t[:, 0]
        den = dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]
        dent = dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1]
        ok = (den > 0) & (dent > 0)
        a = (dq[:, 0] * dt[:, 0] + dq[:, 1] * dt[:, 1]) / den
        b = (dq[:, 0] * dt[:, 1] - dq[:, 1] * dt[:, 0]) / den
        A, ok = _affine_rows(a, -b, b, a, q[:, 0], t[:, 0], ok)
    assert den.dtype == np.float32
    return (A[0], bool(ok[0])) if single else (A, ok)


def _affine_pass(pts, A, max_error) -> np.ndarray:
    """(K, n) bool: the affine predicate of every match (qx, qy, tx, ty) under each of the K rows of A (K, 9):
    dx dx + dy dy <= max_error max_error, inclusive, with dx = px - tx, dy = py - ty.  The last row is not read."""
    m = np.asarray(A, np.float32).reshape(-1, 9)[:, :, None]
    e = np.float32(max_error)
    qx, qy, tx, ty = (pts[None, :, i] for i in range(4))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        px = (m[:, 0] * qx + m[:, 1] * qy) + m[:, 2]
        py = (m[:, 3] * qx + m[:, 4] * qy) + m[:, 5]
        dx = px - tx
        dy = py - ty
        near = dx * dx + dy * dy <= e * e
    assert dx.dtype == np.float32 and dy.dtype == np.float32
    return near


def affine_inliers(matches, q_xy, t_xy, A, max_error) -> np.ndarray:
    """The score of the affine and similarity rules: a bool per DMATCH_DTYPE record, True where the record's query
    position, carried over by A (9 floats, the last row 0 0 1), lies within max_error pixels of its train position,
    inclusive -- transfer_inliers' answer on the same nine floats.  A record with an index outside its position array,
    or a NaN position, is an inlier of nothing."""
    a = np.asarray(A, np.float32).reshape(-1)
    if a.size != 9:
        raise ValueError("A must have 9 entries (3 x 3, row-major, the last row 0 0 1)")
    return _affine_pass(_match_points(matches, q_xy, t_xy), a, max_error)[0]


def ransac_affine(matches, q_xy, t_xy, max_error=1.5, K: int = 1024, seed: int = 0, similarity: bool = False) -> dict:
    """The whole operation (sift_hip_verify_affine_*) in numpy, for the affine map or, with similarity, the similarity.
    Returns ransac_homography's dict, keys H and Hs included (the record is a homography record); samples is (K, 3) or
    (K, 2)."""
    from . import DMATCH_DTYPE

    matches = np.asarray(matches, DMATCH_DTYPE)
    n = len(matches)
    m = 2 if similarity else 3
    pts = _match_points(matches, q_xy, t_xy)
    samples = _samples(n, K, seed, m)
    if n >= m:
        solve = similarity_from_2 if similarity else affine_from_3
        Hs, valid = solve(pts[samples][:, :, :2], pts[samples][:, :, 2:])
        passes = _affine_pass(pts, Hs, max_error) & valid[:, None]
    else:
        Hs, valid, passes = np.zeros((K, 9), np.float32), np.zeros(K, bool), np.zeros((K, n), bool)
    counts = passes.sum(1).astype(np.int32)
    hyp = -1
    if valid.any():
        hyp = int(np.argmax(np.where(valid, counts, -1)))  # the first of the largest: ties to the lowest k
    mask = passes[hyp].astype(np.uint8) if hyp >= 0 else np.zeros(n, np.uint8)
    return dict(H=Hs[hyp].copy() if hyp >= 0 else np.zeros(9, np.float32), inliers=int(counts[hyp]) if hyp >= 0 else 0,
                hypothesis=hyp, matches=n, valid_hypotheses=int(valid.sum()), mask=mask, list=matches[mask != 0],
                samples=samples, Hs=Hs, valid=valid, counts=counts)


def _refit_affine(pts, mask, similarity: bool):
    """One fit of the affine refit rule on gathered points (n, 4) float32 and their mask: (A (9,) float32, valid)."""
    assert pts.dtype == np.float32
    n = len(pts)
    mask = np.asarray(mask).reshape(-1)[:n]
    if len(mask) != n:
        raise ValueError("one mask byte per record")
    zero = np.zeros(9, np.float32)
    fit = (mask != 0) & np.isfinite(pts).all(1)
    m = int(fit.sum())
    if m < (2 if similarity else 3):
        return zero, False
    p = pts.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = _slot_sum(p, fit) / np.float64(m)                       # (mqx, mqy, mtx, mty)
        c = p - mean
        x, y, u, v = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
        Sxx, Sxy, Syy, Txx, Txy, Tyx, Tyy = _slot_sum(np.stack([x * x, x * y, y * y, u * x, u * y, v * x, v * y], 1), fit)
        if similarity:
            den = Sxx + Syy
            ok = bool(np.isfinite(den) and den > 0)
            a = (Txx + Tyy) / den
            c_ = (Tyx - Txy) / den
            b, d = -c_, a
        else:
            det = Sxx * Syy - Sxy * Sxy
            ok = bool(np.isfinite(det) and det > 0)
            a = (Txx * Syy - Txy * Sxy) / det
            b = (Txy * Sxx - Txx * Sxy) / det
            c_ = (Tyx * Syy - Tyy * Sxy) / det
            d = (Tyy * Sxx - Tyx * Sxy) / det
        R = np.array([a, b, mean[2] - (a * mean[0] + b * mean[1]), c_, d, mean[3] - (c_ * mean[0] + d * mean[1]),
                      0.0, 0.0, 1.0], np.float64)
        out = R.astype(np.float32)
    ok = ok and bool(np.isfinite(out).all())
    return (out, True) if ok else (zero, False)


def refit_affine(pts_or_matches, q_xy=None, t_xy=None, mask=None, similarity: bool = False):
    """One fit of the affine refit rule (include/sift_hip.h): the least-squares affine map -- or similarity -- of the
    records mask marks, (A (9,) float32 over the row 0 0 1, valid), from the means and the seven sums of centred
    products in the refit's summation order.  pts_or_matches: as for refit_fundamental.  An invalid fit (fewer than 3
    / 2 fit records, a fit set on one line or at one point, a non-finite result) has A all zero."""
    pts = _refit_points(pts_or_matches, q_xy, t_xy)
    return _refit_affine(pts, np.ones(len(pts), np.uint8) if mask is None else mask, similarity)


def refine_affine(matches, q_xy, t_xy, result, max_error=1.5, rounds: int = 1, similarity: bool = False) -> dict:
    """refine_fundamental for a ransac_affine dict (sift_hip_refine_affine_*)."""
    from . import DMATCH_DTYPE

    if not 1 <= int(rounds) <= REFIT_MAX_ROUNDS:
        raise ValueError("rounds must lie in 1..8")
    matches = np.asarray(matches, DMATCH_DTYPE)
    n = len(matches)
    out = dict(result)
    cur = np.asarray(result["H"], np.float32).reshape(9).copy()
    mask = np.asarray(result["mask"], np.uint8).reshape(-1)[:n].copy()
    if len(mask) != n:
        raise ValueError("one mask byte per record")
    inliers = int(result["inliers"])
    accepted = 0
    pts = _match_points(matches, q_xy, t_xy)
    if int(result["hypothesis"]) >= 0 and geometry_usable(cur):
        for _ in range(int(rounds)):
            cand, ok = _refit_affine(pts, mask, similarity)
            if not ok:
                break  # the state is unchanged, so every later round fails the same way
            keep = _affine_pass(pts, cand, max_error)[0]
            if int(keep.sum()) < inliers:
                break
            cur, mask, inliers = cand, keep.astype(np.uint8), int(keep.sum())
            accepted += 1
    assert cur.dtype == np.float32 and mask.dtype == np.uint8
    out["H"], out["mask"], out["inliers"], out["list"] = cur, mask, inliers, matches[mask != 0]
    out["accepted"] = accepted
    return out


def affine_lstsq(q_pts, t_pts, similarity: bool = False) -> np.ndarray:
    """A reference, not part of the device rule: the float64 least-squares affine map (or similarity) of n >= 3 (2)
    pairs through np.linalg.lstsq, as 3 x 3 with the last row 0 0 1 -- the truth the tests hold the rule against."""
    q = np.asarray(q_pts, np.float64).reshape(len(q_pts), -1)[:, :2]
    t = np.asarray(t_pts, np.float64).reshape(len(t_pts), -1)[:, :2]
    if len(q) != len(t) or len(q) < (2 if similarity else 3):
        raise ValueError("affine_lstsq needs the same number (>= 3, similarity: >= 2) of points on both sides")
    one, nil = np.ones(len(q)), np.zeros(len(q))
    if similarity:  # unknowns (a, b, tx, ty): u = a x - b y + tx, v = b x + a y + ty
        M = np.r_[np.stack([q[:, 0], -q[:, 1], one, nil], 1), np.stack([q[:, 1], q[:, 0], nil, one], 1)]
        a, b, tx, ty = np.linalg.lstsq(M, np.r_[t[:, 0], t[:, 1]], rcond=None)[0]
        return np.array([[a, -b, tx], [b, a, ty], [0, 0, 1]])
    sol = np.linalg.lstsq(np.stack([q[:, 0], q[:, 1], one], 1), t, rcond=None)[0]  # (3, 2)
    return np.r_[sol.T, [[0.0, 0.0, 1.0]]]


# --- Relative pose from a verified fundamental matrix: the rule of sift_hip_recover_pose_* (include/sift_hip.h,
# "Relative pose from a verified fundamental matrix") in numpy float64.  As in the refit: every operation below is one
# IEEE float64 operation in the header's association -- products and sums are written out elementwise, no @, dot,
# einsum or linalg, which may fuse --, and the outputs are rounded to float32 once.  The device's bytes are this code's.

POSE_MAX_DEPTH = 50.0            # cv::recoverPose's distanceThresh, in baselines
POSE_MAX_COS_PARALLAX = 0.99998  # ORB-SLAM's parallax bar
POSE_NAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]  # the one NaN the points carry


def _camera(cam, what: str):
    """(fx, fy, cx, cy) as float64 values of the float32 camera, refused as the calls refuse it."""
    c = np.asarray(cam, np.float32).reshape(-1)
    if c.size != 4:
        raise ValueError(f"{what}: a camera is (fx, fy, cx, cy)")
    if not (c[0] > 0 and c[1] > 0 and np.isfinite(c[:2]).all()):
        raise ValueError(f"{what}: fx and fy must be > 0 and finite")
    if not np.isfinite(c[2:]).all():
        raise ValueError(f"{what}: cx and cy must be finite")
    return [float(v) for v in c]


def essential_from_fundamental(F, cam_q, cam_t) -> np.ndarray:
    """E = Kt^T F Kq (3 x 3 float64) for skew-free cameras (fx, fy, cx, cy): G = F Kq column by column, then Kt^T G row
    by row, each entry in the header's association."""
    f = np.asarray(F, np.float32).reshape(-1)
    if f.size != 9:
        raise ValueError("F must have 9 entries (3 x 3, row-major)")
    f = [float(v) for v in f]
    fxq, fyq, cxq, cyq = _camera(cam_q, "cam_q")
    fxt, fyt, cxt, cyt = _camera(cam_t, "cam_t")
    G = [[f[3 * r] * fxq, f[3 * r + 1] * fyq, (f[3 * r] * cxq + f[3 * r + 1] * cyq) + f[3 * r + 2]] for r in range(3)]
    E = np.zeros((3, 3), np.float64)
    for c in range(3):
        E[0, c] = fxt * G[0][c]
        E[1, c] = fyt * G[1][c]
        E[2, c] = (cxt * G[0][c] + cyt * G[1][c]) + G[2][c]
    return E


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def decompose_essential(E, sweeps: int = REFIT_SWEEPS) -> list:
    """The four (R, t) candidates of an essential matrix in cv::decomposeEssentialMat's and cv::recoverPose's order --
    (R1, t), (R2, t), (R1, -t), (R2, -t), R (3, 3) and t (3,) float64, |t| = 1 -- or [] when E has rank <= 1.  The
    right singular vectors are the eigenvectors of E^T E by the refit's Jacobi routine (3 x 3, `sweeps` sweeps), taken
    in descending order of their eigenvalues (ties to the lower index); v3 = v1 x v2, u_i = (E v_i) / s_i,
    u3 = u1 x u2, so U and V are proper by construction and R1 = U W V^T, R2 = U W^T V^T are rotations."""
    E = [[float(np.asarray(E, np.float64).reshape(3, 3)[r, c]) for c in range(3)] for r in range(3)]
    N = [[(E[0][r] * E[0][c] + E[1][r] * E[1][c]) + E[2][r] * E[2][c] for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        V, d = _jacobi_full(N, sweeps)
    i1 = 0
    for i in (1, 2):
        if d[i] > d[i1]:
            i1 = i
    i2 = -1
    for i in range(3):
        if i != i1 and (i2 < 0 or d[i] > d[i2]):
            i2 = i
    with np.errstate(all="ignore"):
        s1, s2 = np.sqrt(np.float64(d[i1])), np.sqrt(np.float64(d[i2]))
        if not (np.isfinite(s2) and s2 > 0):
            return []
        v1, v2 = [V[k][i1] for k in range(3)], [V[k][i2] for k in range(3)]
        v3 = _cross(v1, v2)
        u1 = [float(np.float64((E[r][0] * v1[0] + E[r][1] * v1[1]) + E[r][2] * v1[2]) / s1) for r in range(3)]
        u2 = [float(np.float64((E[r][0] * v2[0] + E[r][1] * v2[1]) + E[r][2] * v2[2]) / s2) for r in range(3)]
    u3 = _cross(u1, u2)
    R1 = np.array([[(u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c] for c in range(3)] for r in range(3)], np.float64)
    R2 = np.array([[(u1[r] * v2[c] - u2[r] * v1[c]) + u3[r] * v3[c] for c in range(3)] for r in range(3)], np.float64)
    t = np.array(u3, np.float64)
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def triangulate_depths(R, t, xq, xt):
    """The two depths of every record under the pose X_t = R X_q + t: (a, b, det, cosine), each (n,) float64.  xq, xt:
    (n, 2) float64 normalised image coordinates (the rays are (x, y, 1)).  With p = R xq, (a, b) minimise
    |a p + t - b xt|^2 -- the closed form of the 2 x 2 normal equations, det = pp xx - px px -- and cosine =
    px / sqrt(pp xx) is the cosine of the angle between the two rays."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    xq, xt = np.asarray(xq, np.float64).reshape(-1, 2), np.asarray(xt, np.float64).reshape(-1, 2)
    x0, x1, y0, y1 = xq[:, 0], xq[:, 1], xt[:, 0], xt[:, 1]
    with np.errstate(all="ignore"):
        p0 = (R[0, 0] * x0 + R[0, 1] * x1) + R[0, 2]
        p1 = (R[1, 0] * x0 + R[1, 1] * x1) + R[1, 2]
        p2 = (R[2, 0] * x0 + R[2, 1] * x1) + R[2, 2]
        pp = (p0 * p0 + p1 * p1) + p2 * p2
        xx = (y0 * y0 + y1 * y1) + 1.0
        px = (p0 * y0 + p1 * y1) + p2
        pt = (p0 * t[0] + p1 * t[1]) + p2 * t[2]
        xt_t = (y0 * t[0] + y1 * t[1]) + t[2]
        det = pp * xx - px * px
        a = (px * xt_t - pt * xx) / det
        b = (pp * xt_t - px * pt) / det
        cosine = px / np.sqrt(pp * xx)
    assert a.dtype == np.float64 and b.dtype == np.float64 and cosine.dtype == np.float64
    return a, b, det, cosine


def recover_pose(matches, q_xy, t_xy, result, mask, cam_q, cam_t, max_depth=POSE_MAX_DEPTH,
                 max_cos_parallax=POSE_MAX_COS_PARALLAX, sweeps: int = REFIT_SWEEPS) -> dict:
    """The whole pose operation (sift_hip_recover_pose_*) in numpy.  matches: the n DMATCH_DTYPE records that count;
    result: a ransac_fundamental / refine_fundamental dict or a VERIFY_RESULT_DTYPE record (read: F, hypothesis); mask:
    n bytes, the fit set; cam_q / cam_t: (fx, fy, cx, cy).  Returns a dict: R (9,) and t (3,) float32 with
    X_train = R X_query + t and |t| = 1, in_front, with_parallax, counts (4,) int32, candidate (-1: the empty result),
    fit, mask (n,) uint8, points (n, 3) float32 in the query camera's frame (POSE_NAN rows where the record is not in
    front) and list, the in-front records in input order."""
    from . import DMATCH_DTYPE

    matches = np.asarray(matches, DMATCH_DTYPE).reshape(-1)
    n = len(matches)
    mask = np.asarray(mask, np.uint8).reshape(-1)[:n]
    if len(mask) != n:
        raise ValueError("one mask byte per record")
    kq, kt = _camera(cam_q, "cam_q"), _camera(cam_t, "cam_t")
    md, mc = np.float32(max_depth), np.float32(max_cos_parallax)
    if not md > 0:
        raise ValueError("max_depth must be > 0")
    if not (mc >= -1 and mc <= 1):
        raise ValueError("max_cos_parallax must lie in [-1, 1]")
    md, mc = np.float64(md), np.float64(mc)
    pts = _match_points(matches, q_xy, t_xy)
    fit = (mask != 0) & np.isfinite(pts).all(1)
    out = {"R": np.zeros(9, np.float32), "t": np.zeros(3, np.float32), "in_front": 0, "with_parallax": 0,
           "counts": np.zeros(4, np.int32), "candidate": -1, "fit": int(fit.sum()), "mask": np.zeros(n, np.uint8),
           "points": np.full((n, 3), POSE_NAN, np.float32), "list": matches[:0].copy()}
    f = np.asarray(result["F"], np.float32).reshape(-1)
    if not (int(result["hypothesis"]) >= 0 and geometry_usable(f)):
        return out
    cands = decompose_essential(essential_from_fundamental(f, cam_q, cam_t), sweeps)
    if not cands:
        return out
    p = pts.astype(np.float64)
    with np.errstate(all="ignore"):
        xq = np.stack([(p[:, 0] - kq[2]) / kq[0], (p[:, 1] - kq[3]) / kq[1]], 1)
        xt = np.stack([(p[:, 2] - kt[2]) / kt[0], (p[:, 3] - kt[3]) / kt[1]], 1)
        front, parallax, depth = [], [], []
        for R, t in cands:
            a, b, det, cosine = triangulate_depths(R, t, xq, xt)
            ok = fit & (det > 0) & (a > 0) & (b > 0) & (a < md) & (b < md)
            front.append(ok)
            parallax.append(ok & (cosine < mc))
            depth.append(a)
    counts = np.array([int(k.sum()) for k in front], np.int32)
    best = 0
    for k in range(1, 4):
        if counts[k] > counts[best]:
            best = k
    if counts[best] == 0:
        return out
    keep = front[best]
    with np.errstate(all="ignore"):
        a = depth[best]
        X = np.stack([a * xq[:, 0], a * xq[:, 1], a], 1).astype(np.float32)
    out["points"][keep] = X[keep]
    out.update(R=cands[best][0].reshape(9).astype(np.float32), t=cands[best][1].astype(np.float32),
               in_front=int(counts[best]), with_parallax=int(parallax[best].sum()), counts=counts, candidate=best,
               mask=keep.astype(np.uint8), list=matches[keep])
    assert out["R"].dtype == np.float32 and out["points"].dtype == np.float32
    return out


# --- Relative pose from a verified homography: the rule of sift_hip_recover_pose_homography_* (include/sift_hip.h,
# "Relative pose from a verified homography") in numpy float64, written as the rule above is: one IEEE operation per
# operation written, the header's associations, outputs rounded to float32 once.

def calibrated_homography(H, cam_q, cam_t) -> np.ndarray:
    """A = Kt^-1 H Kq (3 x 3 float64) for skew-free cameras (fx, fy, cx, cy): G = H Kq column by column as in
    essential_from_fundamental, then the rows of Kt^-1, each entry in the header's association.  H keeps its sign."""
    h = np.asarray(H, np.float32).reshape(-1)
    if h.size != 9:
        raise ValueError("H must have 9 entries (3 x 3, row-major)")
    h = [float(v) for v in h]
    fxq, fyq, cxq, cyq = _camera(cam_q, "cam_q")
    fxt, fyt, cxt, cyt = _camera(cam_t, "cam_t")
    G = [[h[3 * r] * fxq, h[3 * r + 1] * fyq, (h[3 * r] * cxq + h[3 * r + 1] * cyq) + h[3 * r + 2]] for r in range(3)]
    A = np.zeros((3, 3), np.float64)
    with np.errstate(all="ignore"):
        for c in range(3):
            A[0, c] = np.float64(G[0][c] - cxt * G[2][c]) / np.float64(fxt)
            A[1, c] = np.float64(G[1][c] - cyt * G[2][c]) / np.float64(fyt)
            A[2, c] = G[2][c]
    return A


def decompose_homography(A, sweeps: int = REFIT_SWEEPS) -> list:
    """The four (R, t, n, distance) candidates of a calibrated homography A ~ R + t n^T / distance (Ma, Soatto, Kosecka,
    Sastry, 5.3.3), in the order 0 = (R+, t+, N+), 1 = (R-, t-, N-), 2 = (R+, -t+, -N+), 3 = (R-, -t-, -N-): R (3, 3),
    t (3,) with |t| = 1, n (3,) with |n| = 1, all float64, and distance a float64 scalar, the plane's distance from the
    query camera in baselines (X_train = R X_query + t, n^T X_query = distance on the plane).  [] when A^T A has rank
    <= 1, when its largest and smallest eigenvalue do not differ, or when a translation has no length.  The
    eigenvectors of A^T A come from the refit's Jacobi routine (3 x 3, `sweeps` sweeps)."""
    A = [[float(np.asarray(A, np.float64).reshape(3, 3)[r, c]) for c in range(3)] for r in range(3)]
    S = [[(A[0][r] * A[0][c] + A[1][r] * A[1][c]) + A[2][r] * A[2][c] for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        V, d = _jacobi_full(S, sweeps)
    i1 = 0
    for i in (1, 2):
        if d[i] > d[i1]:
            i1 = i
    i2 = -1
    for i in range(3):
        if i != i1 and (i2 < 0 or d[i] > d[i2]):
            i2 = i
    i3 = 3 - i1 - i2
    w1, w2, w3 = np.float64(d[i1]), np.float64(d[i2]), np.float64(d[i3])
    with np.errstate(all="ignore"):
        if not (np.isfinite(w2) and w2 > 0):
            return []
        span = w1 - w3
        if not span > 0:
            return []
        s = np.sqrt(w2)
        Hn = [[float(np.float64(A[r][c]) / s) for c in range(3)] for r in range(3)]
        d23, d12 = w2 - w3, w1 - w2
        d23 = d23 if d23 > 0 else np.float64(0.0)
        d12 = d12 if d12 > 0 else np.float64(0.0)
        a, b = float(np.sqrt(d23 / span)), float(np.sqrt(d12 / span))
    v1, v2 = [V[k][i1] for k in range(3)], [V[k][i2] for k in range(3)]
    v3 = _cross(v1, v2)
    half = []
    for u in ([a * v1[k] + b * v3[k] for k in range(3)], [a * v1[k] - b * v3[k] for k in range(3)]):
        N = _cross(v2, u)
        hv = [(Hn[r][0] * v2[0] + Hn[r][1] * v2[1]) + Hn[r][2] * v2[2] for r in range(3)]
        hu = [(Hn[r][0] * u[0] + Hn[r][1] * u[1]) + Hn[r][2] * u[2] for r in range(3)]
        hc = _cross(hv, hu)
        R = [[(hv[r] * v2[c] + hu[r] * u[c]) + hc[r] * N[c] for c in range(3)] for r in range(3)]
        T = [((Hn[r][0] - R[r][0]) * N[0] + (Hn[r][1] - R[r][1]) * N[1]) + (Hn[r][2] - R[r][2]) * N[2]
             for r in range(3)]
        with np.errstate(all="ignore"):
            norm = np.sqrt(np.float64((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2]))
            if not (np.isfinite(norm) and norm > 0):
                return []
            t = np.array([np.float64(T[r]) / norm for r in range(3)], np.float64)
            dist = np.float64(1.0) / norm
        half.append((np.array(R, np.float64), t, np.array(N, np.float64), dist))
    return half + [(R, -t, -N, dist) for R, t, N, dist in half]


def recover_pose_homography(matches, q_xy, t_xy, result, mask, cam_q, cam_t, max_depth=POSE_MAX_DEPTH,
                            max_cos_parallax=POSE_MAX_COS_PARALLAX, sweeps: int = REFIT_SWEEPS) -> dict:
    """The whole plane pose operation (sift_hip_recover_pose_homography_*) in numpy.  The arguments are recover_pose's,
    with result a ransac_homography / refine_homography dict or a HOMOGRAPHY_RESULT_DTYPE record (read: H,
    hypothesis).  Returns recover_pose's dict -- the fit set here also asks for w = (h6 qx + h7 qy) + h8 > 0 -- plus
    normal (3,) float32, distance (float32) of the winner and candidates, four PLANE_CANDIDATE_DTYPE records (all zero
    when H has no decomposition, filled also when no record is in front).  counts shows a tie between two candidates;
    the first of them is the winner."""
    from . import DMATCH_DTYPE, PLANE_CANDIDATE_DTYPE

    matches = np.asarray(matches, DMATCH_DTYPE).reshape(-1)
    n = len(matches)
    mask = np.asarray(mask, np.uint8).reshape(-1)[:n]
    if len(mask) != n:
        raise ValueError("one mask byte per record")
    kq, kt = _camera(cam_q, "cam_q"), _camera(cam_t, "cam_t")
    md, mc = np.float32(max_depth), np.float32(max_cos_parallax)
    if not md > 0:
        raise ValueError("max_depth must be > 0")
    if not (mc >= -1 and mc <= 1):
        raise ValueError("max_cos_parallax must lie in [-1, 1]")
    md, mc = np.float64(md), np.float64(mc)
    pts = _match_points(matches, q_xy, t_xy)
    h = np.asarray(result["H"], np.float32).reshape(-1)
    p = pts.astype(np.float64)
    with np.errstate(all="ignore"):
        w = (np.float64(h[6]) * p[:, 0] + np.float64(h[7]) * p[:, 1]) + np.float64(h[8])
        fit = (mask != 0) & np.isfinite(pts).all(1) & (w > 0)
    out = {"R": np.zeros(9, np.float32), "t": np.zeros(3, np.float32), "in_front": 0, "with_parallax": 0,
           "counts": np.zeros(4, np.int32), "candidate": -1, "fit": int(fit.sum()), "normal": np.zeros(3, np.float32),
           "distance": np.float32(0), "candidates": np.zeros(4, PLANE_CANDIDATE_DTYPE), "mask": np.zeros(n, np.uint8),
           "points": np.full((n, 3), POSE_NAN, np.float32), "list": matches[:0].copy()}
    if not (int(result["hypothesis"]) >= 0 and geometry_usable(h)):
        return out
    cands = decompose_homography(calibrated_homography(h, cam_q, cam_t), sweeps)
    if not cands:
        return out
    for k, (R, t, N, dist) in enumerate(cands):
        out["candidates"][k] = (R.reshape(9).astype(np.float32), t.astype(np.float32), N.astype(np.float32),
                                np.float32(dist))
    with np.errstate(all="ignore"):
        xq = np.stack([(p[:, 0] - kq[2]) / kq[0], (p[:, 1] - kq[3]) / kq[1]], 1)
        xt = np.stack([(p[:, 2] - kt[2]) / kt[0], (p[:, 3] - kt[3]) / kt[1]], 1)
        front, parallax, depth = [], [], []
        for R, t, _, _ in cands:
            a, b, det, cosine = triangulate_depths(R, t, xq, xt)
            ok = fit & (det > 0) & (a > 0) & (b > 0) & (a < md) & (b < md)
            front.append(ok)
            parallax.append(ok & (cosine < mc))
            depth.append(a)
    counts = np.array([int(k.sum()) for k in front], np.int32)
    out["counts"] = counts
    best = 0
    for k in range(1, 4):
        if counts[k] > counts[best]:
            best = k
    if counts[best] == 0:
        return out
    keep = front[best]
    with np.errstate(all="ignore"):
        a = depth[best]
        X = np.stack([a * xq[:, 0], a * xq[:, 1], a], 1).astype(np.float32)
    out["points"][keep] = X[keep]
    R, t, N, dist = cands[best]
    out.update(R=R.reshape(9).astype(np.float32), t=t.astype(np.float32), in_front=int(counts[best]),
               with_parallax=int(parallax[best].sum()), candidate=best, normal=N.astype(np.float32),
               distance=np.float32(dist), mask=keep.astype(np.uint8), list=matches[keep])
    assert out["R"].dtype == np.float32 and out["points"].dtype == np.float32
    return out


# --- Essential-matrix verification: the rule of sift_hip_verify_essential_* (include/sift_hip.h, "Essential-matrix
# verification") in numpy.  The 5-point solve is float64 from the calibrated rays to the unit-norm pixel-space F, one
# IEEE operation per array operation in the header's association (no @, dot, einsum, polynomial or linalg routine),
# vectorised across the samples; the models are rounded to float32 once, and the score is ransac_fundamental's.

ESSENTIAL_SLOTS = 10        # model slots per sample: the degree of the polynomial in z
ESSENTIAL_BISECTIONS = 48   # bisection steps per bracket with a sign change
ESSENTIAL_NEWTON = 3        # Newton steps after them, each kept only inside the bracket

# The variables of a constraint polynomial are indexed 0 = x, 1 = y, 2 = z, 3 = 1.  A quadratic's ten coefficients are
# those of the pairs i <= j in lexicographic order; a cubic's twenty are stored in Nister's column order.
_ESS_PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]
_ESS_COLUMNS = ["xxx", "yyy", "xxy", "xyy", "xxz", "xx", "yyz", "yy", "xyz", "xy",
                "xzz", "xz", "x", "yzz", "yz", "y", "zzz", "zz", "z", ""]
_ESS_T2 = [[_ESS_PAIRS.index((min(i, j), max(i, j))) for j in range(4)] for i in range(4)]
_ESS_T3 = [[_ESS_COLUMNS.index("".join("xyz"[v] for v in sorted(_ESS_PAIRS[m] + (k,)) if v < 3)) for k in range(4)]
           for m in range(10)]


def essential_samples(n: int, K: int, seed: int = 0) -> np.ndarray:
    """The sampler of the essential rule: (K, 5) int32, ransac_samples' draw with 5 indices.  n < 5: every entry -1."""
    return _samples(n, K, seed, 5)


def _ess_first_largest(mag):
    """The pivot scan on (K, m) magnitudes: the first of the largest, starting from entry 0 and moving on a strictly
    larger value only (nothing is larger than a NaN at entry 0, and a NaN is larger than nothing)."""
    flat = np.argmax(np.where(np.isnan(mag), -1.0, mag), axis=1)
    return np.where(np.isnan(mag[:, 0]), 0, flat)


def _ess_null_space(A):
    """Gauss-Jordan with full pivoting on (K, 5, 9) float64 systems (changed in place): (B (K, 4, 9), ok (K,)), B[:, f]
    the solution with the free variable at position 5 + f set to 1, the column permutation undone."""
    K = len(A)
    ar = np.arange(K)
    perm = np.tile(np.arange(9), (K, 1))
    ok = np.ones(K, bool)
    for c in range(5):
        flat = _ess_first_largest(np.abs(A[:, c:, c:]).reshape(K, -1))
        pr, pc = c + flat // (9 - c), c + flat % (9 - c)
        tmp = A[ar, c, :].copy()
        A[ar, c, :] = A[ar, pr, :]
        A[ar, pr, :] = tmp
        tmp = A[ar, :, c].copy()
        A[ar, :, c] = A[ar, :, pc]
        A[ar, :, pc] = tmp
        tmp = perm[ar, c].copy()
        perm[ar, c] = perm[ar, pc]
        perm[ar, pc] = tmp
        p = A[:, c, c]
        ok &= (p != 0) & np.isfinite(p)
        for r in range(5):
            if r != c:
                m = A[:, r, c] / p
                A[:, r, c + 1:] = A[:, r, c + 1:] - m[:, None] * A[:, c, c + 1:]
    B = np.zeros((K, 4, 9), np.float64)
    for f in range(4):
        y = np.zeros((K, 9), np.float64)
        y[:, 5 + f] = 1
        for i in range(5):
            y[:, i] = (-A[:, i, 5 + f]) / A[:, i, i]
        B[ar[:, None], f, perm] = y
    return B, ok


def _ess_mul11(a, b):
    """(K, 4) x (K, 4) linear polynomials -> (K, 10) quadratic, each coefficient summed from zero in loop order."""
    c = np.zeros((len(a), 10), np.float64)
    for i in range(4):
        for j in range(4):
            c[:, _ESS_T2[i][j]] = c[:, _ESS_T2[i][j]] + a[:, i] * b[:, j]
    return c


def _ess_mul21(a, b):
    """(K, 10) quadratic x (K, 4) linear -> (K, 20) cubic in Nister's column order, summed from zero in loop order."""
    c = np.zeros((len(a), 20), np.float64)
    for m in range(10):
        for k in range(4):
            c[:, _ESS_T3[m][k]] = c[:, _ESS_T3[m][k]] + a[:, m] * b[:, k]
    return c


def _ess_constraints(B):
    """The (K, 10, 20) coefficient matrix of det E = 0 (row 0) and of the nine entries of (E E^T - tr(E E^T) / 2) E = 0
    (rows 1 .. 9, row-major) for E = x X + y Y + z Z + W."""
    e = [[np.stack([B[:, 0, 3 * r + c], B[:, 1, 3 * r + c], B[:, 2, 3 * r + c], B[:, 3, 3 * r + c]], 1)
          for c in range(3)] for r in range(3)]
    M = np.zeros((len(B), 10, 20), np.float64)
    m0 = _ess_mul11(e[1][1], e[2][2]) - _ess_mul11(e[1][2], e[2][1])
    m1 = _ess_mul11(e[1][0], e[2][2]) - _ess_mul11(e[1][2], e[2][0])
    m2 = _ess_mul11(e[1][0], e[2][1]) - _ess_mul11(e[1][1], e[2][0])
    M[:, 0] = (_ess_mul21(m0, e[0][0]) - _ess_mul21(m1, e[0][1])) + _ess_mul21(m2, e[0][2])
    G = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            G[i][j] = (_ess_mul11(e[i][0], e[j][0]) + _ess_mul11(e[i][1], e[j][1])) + _ess_mul11(e[i][2], e[j][2])
            G[j][i] = G[i][j]
    half = 0.5 * ((G[0][0] + G[1][1]) + G[2][2])
    L = [[G[i][j] - half if i == j else G[i][j] for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(3):
            M[:, 1 + 3 * i + j] = (_ess_mul21(L[i][0], e[0][j]) + _ess_mul21(L[i][1], e[1][j])) + _ess_mul21(L[i][2], e[2][j])
    return M


def _ess_reduce(M):
    """Gauss-Jordan on the first ten columns of (K, 10, 20) with row pivoting (changed in place): (R (K, 6, 10), ok),
    R the right-hand ten columns of rows 4 .. 9, each divided by its pivot."""
    K = len(M)
    ar = np.arange(K)
    ok = np.ones(K, bool)
    for c in range(10):
        pr = c + _ess_first_largest(np.abs(M[:, c:, c]))
        tmp = M[ar, c, :].copy()
        M[ar, c, :] = M[ar, pr, :]
        M[ar, pr, :] = tmp
        p = M[:, c, c]
        ok &= (p != 0) & np.isfinite(p)
        for r in range(10):
            if r != c:
                m = M[:, r, c] / p
                M[:, r, c + 1:] = M[:, r, c + 1:] - m[:, None] * M[:, c, c + 1:]
    R = np.zeros((K, 6, 10), np.float64)
    for r in range(6):
        R[:, r] = M[:, 4 + r, 10:] / M[:, 4 + r, 4 + r][:, None]
    return R, ok


def _ess_conv(a, b):
    """The product of two polynomials in z, coefficients ascending, (K, la) x (K, lb), summed from zero in loop order."""
    c = np.zeros((len(a), a.shape[1] + b.shape[1] - 1), np.float64)
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            c[:, i + j] = c[:, i + j] + a[:, i] * b[:, j]
    return c


def _ess_horner(c, d, z):
    """sum c[k] z^k for k <= d: acc = c[d], then acc = acc z + c[k] downwards."""
    acc = c[:, d]
    for k in range(d - 1, -1, -1):
        acc = acc * z + c[:, k]
    return acc


def _ess_value(c, d, z):
    """_ess_horner where z is finite; at z = -inf / +inf a value with the polynomial's sign there (c[d], negated at
    -inf for an odd d)."""
    lead = c[:, d]
    return np.where(z == -np.inf, -lead if d % 2 else lead, np.where(z == np.inf, lead, _ess_horner(c, d, z)))


def _ess_z(s):
    """The point of the real line that s in [-1, 1] stands for: s / (1 - |s|)."""
    return s / (1.0 - np.abs(s))


def _ess_roots(c):
    """The real roots of the (K, 11) polynomials by the derivative chain: (z (K, 10), has (K, 10), ok (K,)) -- bracket i
    of the last level, its root where has, in ascending order.  Brackets are bisected in s = z / (1 + |z|)."""
    K = len(c)
    ok = (c[:, 10] != 0) & np.isfinite(c).all(1)
    D = [None] * 11
    D[10] = c
    for d in range(10, 0, -1):
        D[d - 1] = np.stack([D[d][:, k + 1] * float(k + 1) for k in range(d)], 1)
    ns = [np.full(K, -1.0), np.full(K, 1.0)]
    nz = [np.full(K, -np.inf), np.full(K, np.inf)]
    has = []
    for d in range(1, 11):
        f = [_ess_value(D[d], d, z) for z in nz]
        new_s, new_z, has = [ns[0]], [nz[0]], []
        for i in range(d):
            flo, fhi = f[i], f[i + 1]
            h = ((flo < 0) & (fhi >= 0)) | ((flo > 0) & (fhi <= 0))
            a, b = ns[i], ns[i + 1]
            for _ in range(ESSENTIAL_BISECTIONS):
                mid = 0.5 * (a + b)
                fm = _ess_value(D[d], d, _ess_z(mid))
                same = np.where(flo < 0, fm < 0, fm > 0)
                a, b = np.where(same, mid, a), np.where(same, b, mid)
            z, za, zb = _ess_z(0.5 * (a + b)), _ess_z(a), _ess_z(b)
            for _ in range(ESSENTIAL_NEWTON):
                zn = z - _ess_horner(D[d], d, z) / _ess_horner(D[d - 1], d - 1, z)
                z = np.where((zn >= za) & (zn <= zb), zn, z)
            s = z / (1.0 + np.abs(z))
            s = np.where(s < a, a, s)
            s = np.where(s > b, b, s)
            new_s.append(np.where(h, s, ns[i]))
            new_z.append(np.where(h, z, nz[i]))
            has.append(h)
        new_s.append(ns[-1])
        new_z.append(nz[-1])
        ns, nz = new_s, new_z
    assert len(nz) == 12 and nz[1].shape == (K,)
    return np.stack(nz[1:11], 1), np.stack(has, 1), ok


def _essential_from_5(q, t, cam_q, cam_t):
    """(K, 5, 2) float32 pairs -> (F (K, 10, 9) float32, valid (K, 10), E (K, 10, 9) float64, z (K, 10) float64)."""
    fxq, fyq, cxq, cyq = cam_q
    fxt, fyt, cxt, cyt = cam_t
    K = len(q)
    with np.errstate(all="ignore"):
        qx = (q[:, :, 0].astype(np.float64) - cxq) / fxq
        qy = (q[:, :, 1].astype(np.float64) - cyq) / fyq
        tx = (t[:, :, 0].astype(np.float64) - cxt) / fxt
        ty = (t[:, :, 1].astype(np.float64) - cyt) / fyt
        A = np.stack([tx * qx, tx * qy, tx, ty * qx, ty * qy, ty, qx, qy, np.ones_like(qx)], axis=2)  # (K, 5, 9)
        B, ok = _ess_null_space(A)
        R, ok2 = _ess_reduce(_ess_constraints(B))
        ok &= ok2
        # The 3 x 3 matrix in z over (x, y, 1): row i from rows e = R[2 i], f = R[2 i + 1] as e - z f.
        P = [[np.stack([e[:, 3 * v + 2], e[:, 3 * v + 1] - f[:, 3 * v + 2], e[:, 3 * v] - f[:, 3 * v + 1], -f[:, 3 * v]], 1)
              for v in range(2)] +
             [np.stack([e[:, 9], e[:, 8] - f[:, 9], e[:, 7] - f[:, 8], e[:, 6] - f[:, 7], -f[:, 6]], 1)]
             for e, f in ((R[:, 0], R[:, 1]), (R[:, 2], R[:, 3]), (R[:, 4], R[:, 5]))]
        det = (_ess_conv(_ess_conv(P[1][1], P[2][2]) - _ess_conv(P[1][2], P[2][1]), P[0][0])
               - _ess_conv(_ess_conv(P[1][0], P[2][2]) - _ess_conv(P[1][2], P[2][0]), P[0][1])) \
            + _ess_conv(_ess_conv(P[1][0], P[2][1]) - _ess_conv(P[1][1], P[2][0]), P[0][2])
        zs, has, ok3 = _ess_roots(det)
        ok &= ok3
        F = np.zeros((K, 10, 9), np.float32)
        Es = np.zeros((K, 10, 9), np.float64)
        Z = np.zeros((K, 10), np.float64)
        valid = np.zeros((K, 10), bool)
        slot = np.zeros(K, np.int64)
        for i in range(10):
            z = zs[:, i]
            b = [[_ess_horner(P[r][v], 3 if v < 2 else 4, z) for v in range(3)] for r in range(3)]
            # Cramer's rule on the row pair (0, 1), (0, 2) or (1, 2) with the largest |d|, the first on a tie.
            d = x = y = None
            for u, v in ((0, 1), (0, 2), (1, 2)):
                du = b[u][0] * b[v][1] - b[u][1] * b[v][0]
                xu = b[u][1] * b[v][2] - b[u][2] * b[v][1]
                yu = b[u][2] * b[v][0] - b[u][0] * b[v][2]
                if d is None:
                    d, x, y = du, xu, yu
                else:
                    better = np.abs(du) > np.abs(d)
                    d, x, y = np.where(better, du, d), np.where(better, xu, x), np.where(better, yu, y)
            x, y = x / d, y / d
            E = ((x[:, None] * B[:, 0] + y[:, None] * B[:, 1]) + z[:, None] * B[:, 2]) + B[:, 3]
            # F = Kt^-T E Kq^-1: M = E Kq^-1 column by column, then Kt^-T M row by row.
            M = np.zeros((K, 3, 3), np.float64)
            E3 = E.reshape(K, 3, 3)
            M[:, :, 0] = E3[:, :, 0] / fxq
            M[:, :, 1] = E3[:, :, 1] / fyq
            M[:, :, 2] = E3[:, :, 2] - (M[:, :, 0] * cxq + M[:, :, 1] * cyq)
            G = np.zeros((K, 3, 3), np.float64)
            G[:, 0] = M[:, 0] / fxt
            G[:, 1] = M[:, 1] / fyt
            G[:, 2] = M[:, 2] - (G[:, 0] * cxt + G[:, 1] * cyt)
            G = G.reshape(K, 9)
            ss = G[:, 0] * G[:, 0]
            for j in range(1, 9):
                ss = ss + G[:, j] * G[:, j]
            f32 = (G / np.sqrt(ss)[:, None]).astype(np.float32)
            use = ok & has[:, i]
            good = use & np.isfinite(f32).all(1)
            rows = np.nonzero(good)[0]
            F[rows, slot[rows]] = f32[rows]
            Es[rows, slot[rows]] = E[rows]
            Z[rows, slot[rows]] = z[rows]
            valid[rows, slot[rows]] = True
            slot = slot + use
    assert A.dtype == np.float64 and det.dtype == np.float64 and det.shape == (K, 11)
    return F, valid, Es, Z


def essential_from_5(q_xy5, t_xy5, cam_q, cam_t, calibrated: bool = False):
    """The solver of the essential rule: the up to ten pixel-space models F = Kt^-T E Kq^-1 (unit Frobenius norm,
    float32) of 5 pairs under the two cameras (fx, fy, cx, cy).  q_xy5 / t_xy5: (5, 2) -> (F (10, 9), valid (10,)), or
    (K, 5, 2) -> (F (K, 10, 9), valid (K, 10)).  Slot r holds the r-th real root in ascending order; a slot without a
    root, a non-finite model and every slot of a sample without a solution are zero and invalid.  With `calibrated`
    the float64 E of every slot (as solved: x X + y Y + z Z + W, not normalised) and its root z follow."""
    cq, ct = _camera(cam_q, "cam_q"), _camera(cam_t, "cam_t")
    q = np.asarray(q_xy5, np.float32)
    t = np.asarray(t_xy5, np.float32)
    single = q.ndim == 2
    out = _essential_from_5(q.reshape(-1, 5, 2), t.reshape(-1, 5, 2), cq, ct)
    out = out if calibrated else out[:2]
    return tuple(o[0] for o in out) if single else out


def ransac_essential(matches, q_xy, t_xy, cam_q, cam_t, max_error=1.5, K: int = 256, seed: int = 0) -> dict:
    """The whole operation (sift_hip_verify_essential_*) in numpy.  Returns ransac_fundamental's dict over the 10 K
    model slots: F (the winner's pixel-space matrix), inliers, hypothesis (the slot 10 k + r, -1: none), matches,
    valid_hypotheses (valid slots), mask, list, samples (K, 5), Fs (10 K, 9), valid (10 K,), counts (10 K,)."""
    from . import DMATCH_DTYPE

    cq, ct = _camera(cam_q, "cam_q"), _camera(cam_t, "cam_t")
    matches = np.asarray(matches, DMATCH_DTYPE)
    n = len(matches)
    S = ESSENTIAL_SLOTS * K
    pts = _match_points(matches, q_xy, t_xy)
    samples = essential_samples(n, K, seed)
    if n >= 5:
        Fs, valid, _, _ = _essential_from_5(pts[samples][:, :, :2], pts[samples][:, :, 2:], cq, ct)
        Fs, valid = Fs.reshape(S, 9), valid.reshape(S)
        passes = _sampson_pass(pts, Fs, max_error) & valid[:, None]
    else:
        Fs, valid, passes = np.zeros((S, 9), np.float32), np.zeros(S, bool), np.zeros((S, n), bool)
    counts = passes.sum(1).astype(np.int32)
    hyp = -1
    if valid.any():
        hyp = int(np.argmax(np.where(valid, counts, -1)))  # the first of the largest: ties to the lowest slot
    mask = passes[hyp].astype(np.uint8) if hyp >= 0 else np.zeros(n, np.uint8)
    return dict(F=Fs[hyp].copy() if hyp >= 0 else np.zeros(9, np.float32), inliers=int(counts[hyp]) if hyp >= 0 else 0,
                hypothesis=hyp, matches=n, valid_hypotheses=int(valid.sum()), mask=mask, list=matches[mask != 0],
                samples=samples, Fs=Fs, valid=valid, counts=counts)


def to_cv_keypoints(final_kpts, final_features, size: int = -1):
    import cv2

    f = keypoint_fields(final_kpts, final_features, size)
    out = []
    for i in range(len(f["x"])):
        kp = cv2.KeyPoint(float(f["x"][i]), float(f["y"][i]), float(f["size"][i]), float(f["angle"][i]),
                          float(f["response"][i]), int(f["octave"][i]))
        out.append(kp)
    return out


def to_cv_dmatches(match):
    """list of cv2.DMatch from DMATCH_DTYPE records (matchList, Matcher.match_list_*: real distances and imgIdx), or
    from a match index per query (matchBruteForce: distance 0, -1 skipped)."""
    import cv2

    names = getattr(getattr(match, "dtype", None), "names", None)
    if names and "queryIdx" in names:
        return [cv2.DMatch(int(r["queryIdx"]), int(r["trainIdx"]), int(r["imgIdx"]), float(r["distance"])) for r in match]
    return [cv2.DMatch(q, t, d) for q, t, d in dmatch_triples(match)]
