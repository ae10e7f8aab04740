"""Inputs shared by the two-view verification tests (tests/test_verify_cases.py, tests/test_gpu_verify.py).

The scene is that of tests/epipolar_cases.py (reused unchanged): inliers are project_pairs -- one 3-D point seen in both
views, rounded to the 0.25 grid --, outliers are pairs of independent uniform positions on the same grid.  Both are
shuffled into one DMATCH_DTYPE list whose records index shuffled position arrays (queryIdx != the record's own index
for all but a chance few), so an indirection error shows.  The position arrays hold a few rows no record uses.

SHAPES: (inliers, outliers, hypotheses K).  CAPPED is the list of 65 + 64 records inside a buffer of 200 whose tail
holds further, valid-looking records that must not count.
"""
import functools

import numpy as np

import epipolar_cases as ec

SHAPES = [(120, 80, 512), (24, 9, 256), (9, 0, 64), (8, 0, 64), (7, 0, 64), (0, 0, 64), (300, 300, 1024), (65, 64, 256)]
MAIN = (120, 80, 512)
CAPPED = (65, 64, 256)
CAP = 200
MAX_ERROR = 1.5
SPARE = 5  # position rows no record uses


def make(n_in, n_out, seed=0):
    """(matches, q_xy, t_xy, planted): the DMATCH_DTYPE list (n_in + n_out records), float32 positions
    (n + SPARE, 2) each, and per record whether it is a planted (true) pair."""
    from sift_amd import DMATCH_DTYPE

    rng = np.random.default_rng(7000 * n_in + n_out + seed)
    n = n_in + n_out
    a, b = ec.project_pairs(rng, n_in) if n_in else (np.zeros((0, 2)), np.zeros((0, 2)))
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
    """CAPPED's list at the head of a buffer of CAP records; the tail holds MAIN's first records (valid indices of the
    same position arrays' range), which change the result if they are counted."""
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
    """sift_amd.cv.ransac_fundamental of a shape, computed once and shared; read-only."""
    from sift_amd import cv

    m, q_xy, t_xy, _ = case(n_in, n_out)
    r = cv.ransac_fundamental(m, q_xy, t_xy, max_error, K, seed)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def recovery(mask, planted):
    """(recall of the planted pairs, number of outlier pairs) among the records mask marks."""
    mask = np.asarray(mask, bool)
    n_in = int(planted.sum())
    return (float((mask & planted).sum()) / n_in if n_in else 1.0), int((mask & ~planted).sum())
