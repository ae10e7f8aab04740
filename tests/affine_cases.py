"""Inputs shared by the affine and similarity verification tests (tests/test_affine_cases.py,
tests/test_gpu_affine.py, tests/test_gpu_affine_cxx.py).

The square and the grid are tests/epipolar_cases.py's (SIDE = 200, positions on the 0.25 grid).  The true affine map is
R(17 deg) [[1.2, 0.18], [0, 0.85]] about the square's centre plus (6, -4); the true similarity 1.15 R(17 deg) about the
centre plus (6, -4).  A planted pair is a query position on the grid and its image rounded to the grid (an eighth of
a pixel at most per axis), both inside the square; outliers are pairs of independent uniform positions.  As in
tests/homography_cases.py both are shuffled into one DMATCH_DTYPE list whose records index shuffled position arrays,
which hold a few rows no record uses.  Every case exists once per model: similarity = False / True.

SHAPES: (planted, unrelated, hypotheses K).  (3, 0), (2, 0), (1, 0), (0, 0) bracket n = m and n < m for both models.
CAPPED is the list of 65 + 64 records inside a buffer of 200 whose tail holds further, valid-looking records that must
not count.  LARGE goes past the score kernel's 2048-match LDS tile and the select kernel's 1024-match chunks.  BUDGET
is the list of 20 % planted pairs the budget bars are stated on, with the K of either model.
"""
import functools

import numpy as np

import epipolar_cases as ec

MAIN = (120, 80, 256)
CAPPED = (65, 64, 128)
LARGE = (1800, 313, 64)
BUDGET = (60, 240, 256)
SHAPES = [MAIN, (24, 9, 128), (3, 0, 64), (2, 0, 64), (1, 0, 64), (0, 0, 64), (300, 300, 256), CAPPED, BUDGET]
# The budget bars: with K = BUDGET_K[similarity] hypotheses the mirror finds >= BUDGET_BAR of the 60 planted pairs of
# BUDGET on each of the seeds 0..7 (tests/test_affine_cases.py checks it; on these lists it finds all 60, and does so
# from K = 512 for the affine map and K = 64 for the similarity).
BUDGET_K = {True: 256, False: 1024}
BUDGET_BAR = 57
BUDGET_SEEDS = tuple(range(8))
DEGENERATE_K = 256
# (shape, max_error, seed) per model at which the mirror's refit counts one record fewer than the winner and is
# rejected: a threshold below the grid's rounding (tests/test_affine_cases.py checks that it is).
REJECTED = {False: ((65, 64, 128), 0.12, 7), True: ((65, 64, 128), 0.15, 3)}
CAP = 200
MAX_ERROR = 1.5
SPARE = 5  # position rows no record uses
ANGLE = np.deg2rad(17.0)
SHIFT = np.array([6.0, -4.0])
MODELS = (False, True)  # similarity
MODEL_IDS = ("affine", "similarity")


def sample_size(similarity):
    return 2 if similarity else 3


def true_map(similarity):
    """The true map (float64, 3 x 3, last row 0 0 1): x_train = A x_query + t."""
    c, s = np.cos(ANGLE), np.sin(ANGLE)
    R = np.array([[c, -s], [s, c]])
    A = 1.15 * R if similarity else R @ np.array([[1.2, 0.18], [0.0, 0.85]])
    centre = np.array([ec.SIDE / 2.0, ec.SIDE / 2.0])
    M = np.eye(3)
    M[:2, :2] = A
    M[:2, 2] = centre - A @ centre + SHIFT
    return M


def apply(M, xy):
    """The images (n, 2) of positions (n, 2) under the 3 x 3 M with the last row 0 0 1, in float64."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    return np.asarray(xy, np.float64) @ M[:2, :2].T + M[:2, 2]


def planted_pairs(rng, n, similarity, line=None):
    """n pairs under the true map: query and train positions (n, 2), on the grid and inside the square.  line: the
    query positions all have this y."""
    a, b = np.zeros((n, 2)), np.zeros((n, 2))
    done = 0
    while done < n:
        m = 2 * (n - done) + 8
        p = np.rint(rng.uniform(0, ec.SIDE, (m, 2)) * 4) / 4
        if line is not None:
            p[:, 1] = line
        s = np.rint(apply(true_map(similarity), p) * 4) / 4
        ok = np.flatnonzero(((p >= 0) & (p < ec.SIDE) & (s >= 0) & (s < ec.SIDE)).all(1))[: n - done]
        a[done:done + len(ok)], b[done:done + len(ok)] = p[ok], s[ok]
        done += len(ok)
    return a, b


def make(n_in, n_out, similarity, seed=0):
    """(matches, q_xy, t_xy, planted): the DMATCH_DTYPE list (n_in + n_out records), float32 positions
    (n + SPARE, 2) each, and per record whether it is a planted (true) pair."""
    from sift_amd import DMATCH_DTYPE

    rng = np.random.default_rng(7000 * n_in + n_out + seed + (500000 if similarity else 0))
    n = n_in + n_out
    a, b = planted_pairs(rng, n_in, similarity) if n_in else (np.zeros((0, 2)), np.zeros((0, 2)))
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


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(n_in, n_out, similarity):
    return _frozen(*make(n_in, n_out, similarity))


@functools.lru_cache(maxsize=None)
def capped(similarity):
    """CAPPED's list at the head of a buffer of CAP records; the tail holds records with valid indices of the same
    position arrays, which change the result if they are counted."""
    m, q_xy, t_xy, planted = case(*CAPPED[:2], similarity)
    buf = np.zeros(CAP, m.dtype)
    buf[:len(m)] = m
    rng = np.random.default_rng(5)
    buf["queryIdx"][len(m):] = rng.integers(0, len(q_xy), CAP - len(m))
    buf["trainIdx"][len(m):] = rng.integers(0, len(t_xy), CAP - len(m))
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def degenerate(similarity):
    """(matches, q_xy, t_xy, planted, kind): the (24, 9) list (kind 0), 12 more planted pairs whose query positions lie
    on the line y = 60 (kind 1), and 6 copies of one planted record (kind 2), shuffled: samples of three points on the
    line, or of two copies, are degenerate, every other sample is not."""
    m, q_xy, t_xy, planted = make(24, 9, similarity)
    rng = np.random.default_rng(77 + similarity)
    a, b = planted_pairs(rng, 12, similarity, line=60.0)
    line = np.zeros(12, m.dtype)
    line["queryIdx"], line["trainIdx"] = len(q_xy) + np.arange(12), len(t_xy) + np.arange(12)
    line["distance"] = 300 + np.arange(12)
    copies = np.repeat(m[np.flatnonzero(planted)[:1]], 6)
    q_xy, t_xy = np.r_[q_xy, a.astype(np.float32)], np.r_[t_xy, b.astype(np.float32)]
    both = np.r_[m, line, copies]
    flags = np.r_[planted, np.ones(18, bool)]
    order = rng.permutation(len(both))
    kind = np.r_[np.zeros(len(m), int), np.ones(12, int), np.full(6, 2)]
    return _frozen(both[order], q_xy, t_xy, flags[order], kind[order])


@functools.lru_cache(maxsize=None)
def reference(n_in, n_out, K, similarity, seed=0, max_error=MAX_ERROR):
    """sift_amd.cv.ransac_affine of a shape, computed once and shared; read-only."""
    from sift_amd import cv

    m, q_xy, t_xy, _ = case(n_in, n_out, similarity)
    r = cv.ransac_affine(m, q_xy, t_xy, max_error, K, seed, similarity)
    _frozen(*[v for v in r.values() if isinstance(v, np.ndarray)])
    return r


@functools.lru_cache(maxsize=None)
def refined(n_in, n_out, K, similarity, seed=0, rounds=1, max_error=MAX_ERROR):
    """sift_amd.cv.refine_affine on reference(...), computed once and shared; read-only."""
    from sift_amd import cv

    m, q_xy, t_xy, _ = case(n_in, n_out, similarity)
    r = cv.refine_affine(m, q_xy, t_xy, reference(n_in, n_out, K, similarity, seed, max_error), max_error, rounds,
                         similarity)
    _frozen(*[v for v in r.values() if isinstance(v, np.ndarray)])
    return r


def recovery(mask, planted):
    """(recall of the planted pairs, number of outlier pairs) among the records mask marks."""
    mask = np.asarray(mask, bool)
    n_in = int(planted.sum())
    return (float((mask & planted).sum()) / n_in if n_in else 1.0), int((mask & ~planted).sum())


def rms(A, m, q_xy, t_xy, planted):
    """The RMS transfer error (pixels, float64) of the planted pairs under the nine floats A."""
    q, t = q_xy[m["queryIdx"][planted]], t_xy[m["trainIdx"][planted]]
    d = apply(np.asarray(A, np.float64).reshape(3, 3), q) - t
    return float(np.sqrt((d * d).sum(1).mean()))


@functools.lru_cache(maxsize=None)
def chain_case(similarity, nq=65, nt=64):
    """(q, t, q_xy, t_xy, planted) for the matcher chain, built as homography_cases.chain_case is: descriptor sets of
    random integers 0..127 in which half of the smaller set's size worth of train rows are noisy copies of distinct
    query rows; a planted copy and its query are one pair of the true map, every other position is uniform on the
    grid."""
    rng = np.random.default_rng(3000 * nq + nt + similarity)
    q = rng.integers(0, 128, (nq, 128))
    t = rng.integers(0, 128, (nt, 128))
    k = min(nq, nt) // 2
    src, dst = rng.permutation(nq)[:k], rng.permutation(nt)[:k]
    amp = rng.integers(2, 9, k)
    t[dst] = np.clip(q[src] + rng.integers(-amp[:, None], amp[:, None] + 1, (k, 128)), 0, 255)
    q_xy = rng.integers(0, int(4 * ec.SIDE), (nq, 2)) * 0.25
    t_xy = rng.integers(0, int(4 * ec.SIDE), (nt, 2)) * 0.25
    q_xy[src], t_xy[dst] = planted_pairs(rng, k, similarity)
    return _frozen(q.astype(np.float32), t.astype(np.float32), q_xy.astype(np.float32), t_xy.astype(np.float32),
                   np.stack([src, dst], 1))
