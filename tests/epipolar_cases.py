"""Inputs shared by the epipolar-gate tests (tests/test_match_epipolar_abi.py, tests/test_gpu_match_epipolar.py).

The shapes and the descriptor recipe are those of tests/guided_cases.py (random integers 0..127; half of the smaller
set's size worth of train rows are noisy copies of distinct query rows; an eighth of those queries get a noisy twin),
and every row of both sets gets a position: multiples of 0.25 in a 200 x 200 square.  The geometry is a synthetic
two-camera scene: K = [[180, 0, 100], [0, 180, 100], [0, 0, 1]] for both views, the second camera rotated a little
and moved by t = (0.6, 0.1, 0.15), so F = K^-T [t]x R K^-1 (scaled to unit Frobenius norm, float32) has
x_train^T F x_query = 0.

* A planted near-copy and its query are one 3-D point at depth 3 .. 8 projected into both views (and rounded to the
  0.25 grid, an eighth of a pixel at most per axis): the true correspondence is inside the band of MAX_ERROR = 1.5.
* Every planted query also has a decoy among the other train rows, a closer copy (noise of +-1 against the true
  copy's +-2 .. +-8) at a uniform position: the repeated structure a geometric gate is for.  The global nearest
  neighbour of a planted query is its decoy, mostly off the line, and the guided best is the true correspondence.
* All other positions are uniform, so the band of a query holds about MAX_ERROR * 2 * 200 / 200^2 = 1.5 % of the
  train rows by chance; two queries are then moved to where their band holds no / exactly one train row, so every
  shape from 33 x 31 on has queries with no, one and several candidates.

HAND is the hand-written case for the inclusive edge.
"""
import functools

import numpy as np

from guided_cases import FLT_MAX, SHAPES, SIDE, with_stride  # noqa: F401  (re-exported for the tests)

MAX_ERROR = 1.5
K = np.array([[180.0, 0.0, 100.0], [0.0, 180.0, 100.0], [0.0, 0.0, 1.0]])
T = np.array([0.6, 0.1, 0.15])
RVEC = np.array([0.02, -0.03, 0.01])  # the second camera's rotation (axis * angle, radians)

# F, max_error, query, trains: r = 0.5 tx - ty + 2, nq = 1.25, nr = 1, e2 (nq + nr) = 9.  Train (4, 1) has r = 3, so
# r r == 9 exactly (a candidate: the compare is inclusive); (4.25, 1) has r = 3.125 (not one); (3.75, 1) r = 2.875.
HAND = dict(F=np.float32([[0, 0, 0.5], [0, 0, -1], [0, 1, 0]]), max_error=2.0, q_xy=np.float32([[7, 2]]),
            t_xy=np.float32([[4, 1], [4.25, 1], [3.75, 1]]), mask=[[True, False, True]])


def rotation(rvec):
    th = np.linalg.norm(rvec)
    k = rvec / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)


R = rotation(RVEC)


def fundamental():
    """F of the scene (float32, 3 x 3): x_train^T F x_query = 0."""
    tx = np.array([[0, -T[2], T[1]], [T[2], 0, -T[0]], [-T[1], T[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return (F / np.linalg.norm(F)).astype(np.float32)


def project_pairs(rng, n):
    """n 3-D points seen by both cameras: their positions (n, 2) in the first and in the second view, on the grid."""
    a, b = np.zeros((n, 2)), np.zeros((n, 2))
    done = 0
    while done < n:
        m = 2 * (n - done) + 8
        uv = rng.uniform(0, SIDE, (m, 2))
        z = rng.uniform(3.0, 8.0, m)
        X = (np.linalg.inv(K) @ np.c_[uv, np.ones(m)].T) * z
        Y = K @ (R @ X + T[:, None])
        p = np.rint(uv * 4) / 4
        s = np.rint((Y[:2] / Y[2]).T * 4) / 4
        ok = np.flatnonzero(((p >= 0) & (p < SIDE) & (s >= 0) & (s < SIDE)).all(1))[: n - done]
        a[done:done + len(ok)], b[done:done + len(ok)] = p[ok], s[ok]
        done += len(ok)
    return a, b


def make_epipolar(nq, nt, seed=0):
    """(q, t, q_xy, t_xy, planted): float32 descriptor sets (nq, 128) / (nt, 128), positions (nq, 2) / (nt, 2), and
    the (k, 2) array of planted (query row, train row) pairs."""
    rng = np.random.default_rng(2000 * nq + nt + seed)
    q = rng.integers(0, 128, (nq, 128))
    t = rng.integers(0, 128, (nt, 128))
    k = min(nq, nt) // 2
    order = rng.permutation(nq)
    src, rest = order[:k], order[k:]
    tperm = rng.permutation(nt)
    dst, decoy = tperm[:k], tperm[k:2 * k]
    amp = rng.integers(2, 9, k)
    t[dst] = np.clip(q[src] + rng.integers(-amp[:, None], amp[:, None] + 1, (k, 128)), 0, 255)
    t[decoy] = np.clip(q[src] + rng.integers(-1, 2, (k, 128)), 0, 255)
    ndup = min(k // 8, len(rest))
    q[rest[:ndup]] = np.clip(q[src[:ndup]] + rng.integers(-2, 3, (ndup, 128)), 0, 255)

    q_xy = rng.integers(0, int(4 * SIDE), (nq, 2)) * 0.25
    t_xy = rng.integers(0, int(4 * SIDE), (nt, 2)) * 0.25
    q_xy[src], t_xy[dst] = project_pairs(rng, k)
    if len(rest) - ndup >= 2 and nt >= 31:
        # Whatever the density, one query with no candidate and one with exactly one: two queries that are neither
        # planted nor twins move to the first sampled positions whose band holds no / one train row (lines that only
        # clip a corner of the square).
        from sift_amd import cv

        spots = (rng.integers(0, int(4 * SIDE), (4000, 2)) * 0.25).astype(np.float32)
        count = cv.epipolar_mask(spots, t_xy.astype(np.float32), fundamental(), MAX_ERROR).sum(1)
        for row, want in ((rest[-1], 0), (rest[-2], 1)):
            hit = np.flatnonzero(count == want)
            if len(hit):
                q_xy[row] = spots[hit[0]]
    return (q.astype(np.float32), t.astype(np.float32), q_xy.astype(np.float32), t_xy.astype(np.float32),
            np.stack([src, dst], 1))


@functools.lru_cache(maxsize=None)
def case(nq, nt):
    """The sets of a shape, F, and the reference of both directions (sift_amd.cv.epipolar_top2; the reverse under
    F^T), computed once and shared; every array is read-only."""
    from sift_amd import cv

    q, t, q_xy, t_xy, planted = make_epipolar(nq, nt)
    F = fundamental()
    fwd = cv.epipolar_top2(q, t, q_xy, t_xy, F, MAX_ERROR)
    rev = cv.epipolar_top2(t, q, t_xy, q_xy, F.T, MAX_ERROR)
    for a in (q, t, q_xy, t_xy, F, planted) + fwd + rev:
        a.setflags(write=False)
    return q, t, q_xy, t_xy, F, fwd, rev, planted
