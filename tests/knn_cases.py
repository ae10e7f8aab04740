"""Inputs shared by the k-NN tests (tests/test_knn_cases.py on the CPU, tests/test_gpu_match_knn.py on the GPU).

Integer rows 0..127 with planted noisy copies (tests/test_gpu_match_list.py::make_sets) in the shapes where the k-NN
kernel takes another path; the planted tie sets; the low-entropy set.  The reference is sift_amd.cv.knn, computed once
per case and shared read-only.
"""
import functools

import numpy as np

from test_gpu_match_list import make_sets

KNN_MAX = 8
FLT_MAX = np.finfo(np.float32).max
# (nq, nt, k): one row; nt < k (missing entries are written); nt == k; k = 1 on one train row; partial tiles in both
# sets; train rows past one 256-row key group (the decode and the group merge run); and every served k of both kernel
# instantiations (4 and 8 entries) on a shape that splits.
BIG = (300, 1100)
SHAPES = [(1, 1, 8), (5, 3, 8), (3, 8, 8), (40, 1, 1), (33, 31, 4), (70, 300, 8)] + [BIG + (k,) for k in (1, 2, 3, 5, 8)]

# Twelve train rows identical to query 0, nt = 1100.  Accumulator row = (i & 3) + 8 (i >> 2) + 4 h, so 1 and 5 are in
# one 32-row tile on the two lane halves; 40 is in the next tile of the same key group, 255 the last row of that group,
# 256 the first of the next, 600 in another group, nt - 1 in the last, partial tile; five more in other tiles.
TIE_ROWS = (1, 5, 40, 255, 256, 600, BIG[1] - 1, 100, 333, 500, 777, 1000)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def sets(nq, nt):
    return _freeze(*make_sets(nq, nt))


@functools.lru_cache(maxsize=None)
def reference(nq, nt, k):
    from sift_amd import cv

    return _freeze(*cv.knn(*sets(nq, nt), k))


@functools.lru_cache(maxsize=None)
def tie_sets():
    """BIG-shaped sets with the twelve copies of query 0 planted."""
    q, t = make_sets(*BIG, seed=7)
    t[list(TIE_ROWS)] = q[0]
    return _freeze(q, t)


@functools.lru_cache(maxsize=None)
def low_entropy():
    """Values 0..3, 257 x 600: squared distances are small integers, so most ranks tie."""
    rng = np.random.default_rng(21)
    return _freeze(rng.integers(0, 4, (257, 128)).astype(np.float32), rng.integers(0, 4, (600, 128)).astype(np.float32))


def split_shape(plan):
    """(nq, nt) with nq = 300 and the smallest nt for which plan(nq, nt, 1, KNN_MAX) reports two splits or more."""
    for nt in range(1, 8193):
        if plan(300, nt, 1, KNN_MAX) >= 2:
            return 300, nt
    raise AssertionError("no shape below 8192 train rows splits")


def split_sets(nt):
    """The tie sets cut to nt train rows: the copies at 255 and 256 lie in different splits when nt > 256."""
    q, t = tie_sets()
    return q, t[:nt]


def brute_force(q, t, k):
    """The rule of include/sift_hip.h by a double loop over exact integer distances."""
    idx = np.full((len(q), k), -1, np.int32)
    d2 = np.full((len(q), k), FLT_MAX, np.float32)
    for i, row in enumerate(q):
        cand = sorted((int(((row.astype(np.int64) - tr.astype(np.int64)) ** 2).sum()), j) for j, tr in enumerate(t))[:k]
        for r, (d, j) in enumerate(cand):
            idx[i, r], d2[i, r] = j, d
    return idx, d2
