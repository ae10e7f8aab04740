"""Inputs shared by the homography verification tests (tests/test_homography_cases.py, tests/test_gpu_homography.py,
tests/test_gpu_homography_cxx.py).

The scene is tests/epipolar_cases.py's two cameras (reused unchanged) looking at the plane n . X = d of the first
camera's frame, n = (0.15, -0.1, 1) / |n|, d = 5, so a point of the plane seen at x in the first view is seen at
H_true x in the second, H_true = K (R + T n^T / d) K^-1.  A planted pair is a query position on the 0.25 grid and its
image under H_true rounded to that grid (an eighth of a pixel at most per axis), both inside the square; outliers are
pairs of independent uniform positions on the same grid.  As in tests/verify_cases.py both are shuffled into one
DMATCH_DTYPE list whose records index shuffled position arrays, which hold a few rows no record uses.

SHAPES: (inliers, outliers, hypotheses K).  CAPPED is the list of 65 + 64 records inside a buffer of 200 whose tail
holds further, valid-looking records that must not count.
"""
import functools

import numpy as np

import epipolar_cases as ec

SHAPES = [(120, 80, 512), (24, 9, 256), (5, 0, 64), (4, 0, 64), (3, 0, 64), (0, 0, 64), (300, 300, 1024), (65, 64, 256)]
MAIN = (120, 80, 512)
CAPPED = (65, 64, 256)
LARGE = (1800, 313, 64)  # past the score kernel's LDS tile and the select kernel's chunks
CAP = 200
MAX_ERROR = 1.5
SPARE = 5  # position rows no record uses
PLANE_N = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0])
PLANE_D = 5.0


def homography():
    """H_true of the scene (float64, 3 x 3, H[2][2] = 1): x_train ~ H x_query."""
    H = ec.K @ (ec.R + np.outer(ec.T, PLANE_N) / PLANE_D) @ np.linalg.inv(ec.K)
    return H / H[2, 2]


def apply(H, xy):
    """The images (n, 2) of positions (n, 2) under H, in float64."""
    p = np.c_[np.asarray(xy, np.float64), np.ones(len(xy))] @ np.asarray(H, np.float64).reshape(3, 3).T
    return p[:, :2] / p[:, 2:]


def plane_pairs(rng, n):
    """n points of the plane seen by both cameras: their positions (n, 2) in the first and in the second view, on the
    grid and inside the square."""
    a, b = np.zeros((n, 2)), np.zeros((n, 2))
    done = 0
    while done < n:
        m = 2 * (n - done) + 8
        p = np.rint(rng.uniform(0, ec.SIDE, (m, 2)) * 4) / 4
        s = np.rint(apply(homography(), p) * 4) / 4
        ok = np.flatnonzero(((p >= 0) & (p < ec.SIDE) & (s >= 0) & (s < ec.SIDE)).all(1))[: n - done]
        a[done:done + len(ok)], b[done:done + len(ok)] = p[ok], s[ok]
        done += len(ok)
    return a, b


def make(n_in, n_out, seed=0):
    """(matches, q_xy, t_xy, planted): the DMATCH_DTYPE list (n_in + n_out records), float32 positions
    (n + SPARE, 2) each, and per record whether it is a planted (true) pair."""
    from sift_amd import DMATCH_DTYPE

    rng = np.random.default_rng(9000 * n_in + n_out + seed)
    n = n_in + n_out
    a, b = plane_pairs(rng, n_in) if n_in else (np.zeros((0, 2)), np.zeros((0, 2)))
    rows = n + SPARE
    q_xy = rng.integers(0, int(4 * ec.SIDE), (rows, 2)) * 0.25
    t_xy = rng.integers(0, int(4 * ec.SIDE), (rows, 2)) * 0.25
    qrow, trow = rng.permutation(rows)[:n], rng.permutation(rows)[:n]  # record i's rows, before the list is shuffled
    q_xy[qrow[:n_in]], t_xy[trow[:n_in]] = a, b
    order = rng.permutation(n)
    m = np.zeros(n, DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"] = qrow[order], trow[order]
    m["imgIdx"] = 0
    m["distance"] = (100 + order).astype(np.float32)  # a value per record: the list must come back unchanged
    planted = order < n_in
    return m, q_xy.astype(np.float32), t_xy.astype(np.float32), planted


@functools.lru_cache(maxsize=None)
def case(n_in, n_out):
    m, q_xy, t_xy, planted = make(n_in, n_out)
    for a in (m, q_xy, t_xy, planted):
        a.setflags(write=False)
    return m, q_xy, t_xy, planted


@functools.lru_cache(maxsize=None)
def capped():
    """CAPPED's list at the head of a buffer of CAP records; the tail holds records with valid indices of the same
    position arrays, which change the result if they are counted."""
    m, q_xy, t_xy, planted = case(*CAPPED[:2])
    buf = np.zeros(CAP, m.dtype)
    buf[:len(m)] = m
    rng = np.random.default_rng(5)
    buf["queryIdx"][len(m):] = rng.integers(0, len(q_xy), CAP - len(m))
    buf["trainIdx"][len(m):] = rng.integers(0, len(t_xy), CAP - len(m))
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def reference(n_in, n_out, K, seed=0, max_error=MAX_ERROR):
    """sift_amd.cv.ransac_homography of a shape, computed once and shared; read-only."""
    from sift_amd import cv

    m, q_xy, t_xy, _ = case(n_in, n_out)
    r = cv.ransac_homography(m, q_xy, t_xy, max_error, K, seed)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def recovery(mask, planted):
    """(recall of the planted pairs, number of outlier pairs) among the records mask marks."""
    mask = np.asarray(mask, bool)
    n_in = int(planted.sum())
    return (float((mask & planted).sum()) / n_in if n_in else 1.0), int((mask & ~planted).sum())


@functools.lru_cache(maxsize=None)
def chain_case(nq=65, nt=64):
    """(q, t, q_xy, t_xy, planted) for the matcher chain: descriptor sets built as epipolar_cases.make_epipolar builds
    its own (random integers 0..127; half of the smaller set's size worth of train rows are noisy copies of distinct
    query rows), with positions from the plane: a planted copy and its query are one point of the plane, every other
    position is uniform on the grid.  No decoys, so the putative list is mostly the planted pairs."""
    rng = np.random.default_rng(2000 * nq + nt)
    q = rng.integers(0, 128, (nq, 128))
    t = rng.integers(0, 128, (nt, 128))
    k = min(nq, nt) // 2
    src, dst = rng.permutation(nq)[:k], rng.permutation(nt)[:k]
    amp = rng.integers(2, 9, k)
    t[dst] = np.clip(q[src] + rng.integers(-amp[:, None], amp[:, None] + 1, (k, 128)), 0, 255)
    q_xy = rng.integers(0, int(4 * ec.SIDE), (nq, 2)) * 0.25
    t_xy = rng.integers(0, int(4 * ec.SIDE), (nt, 2)) * 0.25
    q_xy[src], t_xy[dst] = plane_pairs(rng, k)
    out = (q.astype(np.float32), t.astype(np.float32), q_xy.astype(np.float32), t_xy.astype(np.float32),
           np.stack([src, dst], 1))
    for a in out:
        a.setflags(write=False)
    return out
