"""Inputs shared by the guided-matching tests (tests/test_match_guided_abi.py, tests/test_gpu_match_guided.py).

Descriptors follow the make_sets recipe of tests/test_gpu_match_list.py (random integers 0..127, half of the smaller
set's size worth of train rows are noisy copies of distinct query rows), and every row of both sets gets a position:
multiples of 0.25 in a 200 x 200 square, so every coordinate difference is exact in float32.

* A planted near-copy sits at the far side of the square from its query (+100 on both axes, wrapped): the global
  nearest neighbour of a planted query is never inside its window, which is what a guided match is for.
* The recipe's second queries (an eighth of the planted ones get a noisy twin) are put next to the planted copy of
  their twin instead: these are the close matches inside a window, some of them under a distance cap of 30.
* About two thirds of the other train rows lie inside the window of some query (offsets in [-RADIUS, RADIUS]); the
  first two of them lie next to the same query, one of them at dx == +RADIUS exactly (the inclusive compare), so some
  query has two candidates even in the small shapes; the rest are uniform.
"""
import functools

import numpy as np

RADIUS = 6.0
SIDE = 200.0
SHAPES = [(1, 1), (1, 40), (40, 1), (33, 31), (257, 300), (300, 257), (600, 1100)]
FLT_MAX = np.finfo(np.float32).max


def make_guided(nq, nt, seed=0):
    """(q, t, q_xy, t_xy): float32 descriptor sets (nq, 128) / (nt, 128) and positions (nq, 2) / (nt, 2)."""
    rng = np.random.default_rng(1000 * nq + nt + seed)
    q = rng.integers(0, 128, (nq, 128))
    t = rng.integers(0, 128, (nt, 128))
    k = min(nq, nt) // 2
    order = rng.permutation(nq)
    src, rest = order[:k], order[k:]
    dst = rng.permutation(nt)[:k]
    amp = rng.integers(1, 9, k)
    t[dst] = np.clip(q[src] + rng.integers(-amp[:, None], amp[:, None] + 1, (k, 128)), 0, 255)
    ndup = min(k // 8, len(rest))
    q[rest[:ndup]] = np.clip(q[src[:ndup]] + rng.integers(-2, 3, (ndup, 128)), 0, 255)

    quarter = lambda shape, lo, hi: rng.integers(int(4 * lo), int(4 * hi), shape) * 0.25  # noqa: E731
    q_xy = quarter((nq, 2), 0, SIDE)
    t_xy = quarter((nt, 2), 0, SIDE)
    t_xy[dst] = (q_xy[src] + SIDE / 2) % SIDE
    q_xy[rest[:ndup]] = np.clip(t_xy[dst[:ndup]] + quarter((ndup, 2), -3, 3.25), 0, SIDE - 0.25)
    free = np.setdiff1d(np.arange(nt), dst)
    near = free[rng.random(len(free)) < 0.67]
    t_xy[near] = np.clip(q_xy[rng.integers(0, nq, len(near))] + quarter((len(near), 2), -RADIUS, RADIUS + 0.25),
                         0, SIDE - 0.25)
    if len(free) >= 2:  # two candidates of one query, one of them on the window's edge
        anchor = np.clip(q_xy[rest[-1] if len(rest) else 0], RADIUS, SIDE - RADIUS - 0.25)
        q_xy[rest[-1] if len(rest) else 0] = anchor
        t_xy[free[0]] = anchor + (RADIUS, 0.0)
        t_xy[free[1]] = anchor + (-2.5, 1.0)
    elif len(free) == 1:
        t_xy[free[0]] = np.clip(q_xy[0], 0, SIDE - RADIUS - 0.25) + (RADIUS, 0.0)
    return q.astype(np.float32), t.astype(np.float32), q_xy.astype(np.float32), t_xy.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(nq, nt):
    """The sets of a shape and the guided reference of both directions (sift_amd.cv.guided_top2), computed once and
    shared; every array is read-only."""
    from sift_amd import cv

    q, t, q_xy, t_xy = make_guided(nq, nt)
    fwd = cv.guided_top2(q, t, q_xy, t_xy, RADIUS)
    rev = cv.guided_top2(t, q, t_xy, q_xy, RADIUS)
    for a in (q, t, q_xy, t_xy) + fwd + rev:
        a.setflags(write=False)
    return q, t, q_xy, t_xy, fwd, rev


def with_stride(xy, stride, fill=np.nan):
    """(n, 2) positions as an (n, stride) array; the extra columns hold `fill` (they must never be read as x or y)."""
    out = np.full((len(xy), stride), fill, np.float32)
    out[:, :2] = xy
    return out
