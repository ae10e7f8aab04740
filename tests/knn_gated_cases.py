"""Inputs shared by the gated k-NN tests (tests/test_knn_gated_cases.py on the CPU, tests/test_gpu_match_knn_gated.py
and tests/test_gpu_match_knn_gated_cxx.py on the GPU).

Descriptors: the sets of tests/knn_cases.py (SHAPES, tie_sets, low_entropy, split_shape).  Positions: uniform in a
square -- SIDE = 1000 for the big shapes, smaller for the small ones so that their windows are not empty -- with a
window of RADIUS = 37 and a synthetic fundamental matrix F (a pure translation: every epipolar line passes through
the epipole EPIPOLE, left of the frame) with MAX_ERROR = 2.  At BIG = 300 x 1100 both gates admit about six train
rows per query, so the candidate counts straddle every served k; on top of that BIG has planted

    query FAR_QUERY      far outside the frame: no candidate under either gate,
    query NAN_QUERY      a NaN x coordinate, and train row NAN_TRAIN a NaN y: candidates of nothing,
    query CLUSTER_QUERY  with the CLUSTER train rows within half a pixel of it: at least 2 * 8 candidates.

The tie sets (twelve train rows identical to query 0, knn_cases.TIE_ROWS) come with two position variants: the copies
in TIE_INSIDE[v] sit on query 0's position, the others 100 pixels above it (outside the window and far off query 0's
line).  Variant "a" has row 255 inside and row 256 outside, variant "b" the other way round: the key-group boundary,
the split boundary (split_shape cuts after row 255) and the gate all cut through one tie.

References are sift_amd.cv.guided_knn / epipolar_knn, computed once per case and shared read-only.
"""
import functools

import numpy as np

import knn_cases as kc

RADIUS = 37.0
MAX_ERROR = 2.0
SIDE = 1000.0
EPIPOLE = (-700.0, 450.0)
# F = [e]_x for e = (ex, ey, 1): F x_q is the line through e and x_q (x_t^T F x_q = 0 for every x_t on it).
F = np.float32([[0.0, -1.0, EPIPOLE[1]], [1.0, 0.0, -EPIPOLE[0]], [-EPIPOLE[1], EPIPOLE[0], 0.0]])
GATES = ("window", "band")
KS = (1, 2, 3, 5, 8)
SEED = 0
FLT_MAX = kc.FLT_MAX

FAR_QUERY, NAN_QUERY, CLUSTER_QUERY = 290, 291, 292
NAN_TRAIN = 1050
CLUSTER = tuple(range(700, 717))  # 17 train rows

TIE_INSIDE = {"a": (1, 40, 255, 600, 100, 500, 1000), "b": (1, 40, 256, 600, 100, 500, 1000)}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def side_of(nt):
    """The square's side: SIDE, or what gives a window about six of nt train rows."""
    return float(min(SIDE, 2 * RADIUS * np.sqrt(max(nt, 1) / 6.0)))


@functools.lru_cache(maxsize=None)
def positions(nq, nt):
    """(q_xy (nq, 2), t_xy (nt, 2)) float32; BIG carries the plants of the module docstring."""
    rng = np.random.default_rng(SEED + 1000 * nq + nt)
    s = side_of(nt)
    q_xy = rng.uniform(0, s, (nq, 2)).astype(np.float32)
    t_xy = rng.uniform(0, s, (nt, 2)).astype(np.float32)
    if (nq, nt) == kc.BIG:
        q_xy[FAR_QUERY] = (5000.0, 5000.0)
        q_xy[NAN_QUERY, 0] = np.nan
        t_xy[NAN_TRAIN, 1] = np.nan
        q_xy[CLUSTER_QUERY] = (412.0, 655.0)
        t_xy[list(CLUSTER)] = q_xy[CLUSTER_QUERY] + rng.uniform(-0.5, 0.5, (len(CLUSTER), 2)).astype(np.float32)
    return _freeze(q_xy, t_xy)


@functools.lru_cache(maxsize=None)
def tie_positions(variant):
    """BIG's positions with the copies of query 0 placed: TIE_INSIDE[variant] on query 0, the rest 100 px above."""
    q_xy, t_xy = (a.copy() for a in positions(*kc.BIG))
    q_xy[0] = (500.0, 500.0)
    for r in kc.TIE_ROWS:
        t_xy[r] = q_xy[0] if r in TIE_INSIDE[variant] else q_xy[0] + np.float32([0.0, 100.0])
    return _freeze(q_xy, t_xy)


def with_stride(xy, stride, fill=np.nan):
    """(n, 2) positions as rows of `stride` floats, the columns past y holding `fill`."""
    out = np.full((len(xy), stride), fill, np.float32)
    out[:, :2] = xy
    return out


def mask(gate, q_xy, t_xy, F=F, max_error=MAX_ERROR, radius=RADIUS):
    from sift_amd import cv

    if gate == "window":
        return cv.gate_mask(q_xy, t_xy, radius)
    return cv.epipolar_mask(q_xy, t_xy, F, max_error)


def mirror(gate, q, t, q_xy, t_xy, k, F=F):
    """The gated table of the numpy mirror: the window of RADIUS, or the band of F and MAX_ERROR (no window)."""
    from sift_amd import cv

    if gate == "window":
        return cv.guided_knn(q, t, q_xy, t_xy, RADIUS, k)
    return cv.epipolar_knn(q, t, q_xy, t_xy, F, MAX_ERROR, k)


@functools.lru_cache(maxsize=None)
def reference(gate, nq, nt, k):
    return _freeze(*mirror(gate, *kc.sets(nq, nt), *positions(nq, nt), k))


def brute_force(q, t, cand, k):
    """The rule of include/sift_hip.h by a double loop: exact integer distances over the candidates only."""
    idx = np.full((len(q), k), -1, np.int32)
    d2 = np.full((len(q), k), FLT_MAX, np.float32)
    for i, row in enumerate(q):
        best = sorted((int(((row.astype(np.int64) - tr.astype(np.int64)) ** 2).sum()), j)
                      for j, tr in enumerate(t) if cand[i, j])[:k]
        for r, (d, j) in enumerate(best):
            idx[i, r], d2[i, r] = j, d
    return idx, d2


@functools.lru_cache(maxsize=None)
def half_sets():
    """Sets of multiples of 0.5 in 0..15.5 (the general path; every product and sum is exact in fp16 x fp16 -> fp32:
    |d2| <= 128 * 15.5^2 < 2^15 in units of 0.25), 70 x 300, with duplicates so that ranks tie."""
    rng = np.random.default_rng(5)
    q = (rng.integers(0, 32, (70, 128)) * 0.5).astype(np.float32)
    t = (rng.integers(0, 32, (300, 128)) * 0.5).astype(np.float32)
    t[[3, 40, 257, 299]] = q[0]
    t[[10, 11]] = q[5]
    return _freeze(q, t)
