"""Inputs shared by the pose tests (tests/test_pose_cases.py, tests/test_gpu_pose.py, tests/test_gpu_pose_cxx.py).

A scene is a known relative pose (R, t with |t| = 1, rotation angle below 0.4 rad), two different pinhole cameras,
`planted` points seen by both -- 300 are drawn, those with a depth in [0.5, 40] baselines in BOTH cameras are kept, and
the first `planted` of them used -- projected to float32 pixel positions, and the fundamental matrix of the ground
truth formed in float64, scaled to unit Frobenius norm and rounded to float32; sign = -1 negates it, which swaps R1 and
R2 among the candidates.  `unrelated` further records pair random positions.  The record is a VERIFY_RESULT_DTYPE-like
dict (F, hypothesis 0); the mask marks the planted records (`mask_all`: the unrelated ones too).  The rule under test
is sift_amd.cv.recover_pose (include/sift_hip.h, "Relative pose from a verified fundamental matrix").

SEEDS x SIGNS are the scenes of the CPU tests.  They were chosen so that, for every one of them, the rule's winner
counts every planted record and the three other candidates count none (tests/test_pose_cases.py asserts it), and so
that every candidate index 0..3 wins at least once.

POSE_TOL, the bound on the rotation angle and on the angle between the translations -- to the ground truth, to the
independent route, and between the poses from F and -F.  The independent route decomposes the same float64 E with
numpy.linalg.svd (cv::decomposeEssentialMat's construction) and takes the candidate nearest the truth.  Measured over
SEEDS x SIGNS, with angles taken as 2 asin(|dR|_F / (2 sqrt 2)) and atan2(|a x b|, a . b), which resolve an angle near
0 where arccos does not:
    the rule's float32 pose against the independent route:   rotation <= 2.4e-08 rad, translation <= 4.0e-08 rad
    the independent route against the ground truth:          rotation <= 6.4e-08 rad, translation <= 4.1e-08 rad
      (this is the float32 rounding of F and of the positions, which both routes share)
    the rule before its output rounding against the route:   rotation <= 8.6e-16 rad, translation <= 2.5e-16 rad
MEASURED is the largest of the first two lines and POSE_TOL = 16 x MEASURED; tests/test_pose_cases.py measures again
and requires the figures to stay at or below MEASURED.
"""
import functools

import numpy as np

SEEDS = (1, 2, 3, 4, 5, 6)
SIGNS = (1, -1)
DRAWN = 300
DEPTH = (0.5, 40.0)
MEASURED = 6.4e-8
POSE_TOL = 16 * MEASURED

# (planted, unrelated) of the GPU tests: an empty list, the minimal sample, one wave less one, one wave plus one
# unrelated, the CPU tests' list, and a list past the select kernel's 512-row chunks, ragged.
SHAPES = ((0, 0), (8, 0), (63, 0), (64, 1), (300, 60), (1100, 100))

# A rank-1 F: the outer product a e3^T.  E = (Kt^T a) e3^T then has one non-zero column in exact float64 arithmetic, so
# E^T E is diagonal with two zeros, every Jacobi pivot is skipped and s2 = 0: the rule's rank test, which asks for
# s2 > 0 and sets no threshold, sees it.  (An outer product whose E^T E only rounds to rank 1 leaves an s2 of rounding
# size, which that test does not call zero.)
RANK1 = np.outer([0.3, -0.5, 0.8], [0.0, 0.0, 1.0]).astype(np.float32).reshape(9)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], np.float64)
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def kmat(cam):
    fx, fy, cx, cy = (float(v) for v in np.asarray(cam, np.float32))
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def scene(seed, sign=1, planted=DRAWN, unrelated=0, mask_all=False):
    """A dict: matches (DMATCH_DTYPE), q_xy / t_xy (rows of x, y, float32), result (F, hypothesis), mask, cam_q, cam_t,
    R, t (the ground truth, float64), planted (the number of planted records, which come first); read-only."""
    from sift_amd import DMATCH_DTYPE

    rng = np.random.default_rng(1000 + seed)
    R = rotation(rng.normal(size=3), rng.uniform(0.05, 0.38))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t)
    cam_q = np.array([rng.uniform(600, 900), rng.uniform(600, 900), rng.uniform(300, 340), rng.uniform(220, 260)], np.float32)
    cam_t = np.array([rng.uniform(400, 600), rng.uniform(400, 600), rng.uniform(200, 440), rng.uniform(140, 340)], np.float32)
    Kq, Kt = kmat(cam_q), kmat(cam_t)
    kept = []
    while sum(len(k) for k in kept) < planted:
        X = np.stack([rng.uniform(-4, 4, DRAWN), rng.uniform(-3, 3, DRAWN), rng.uniform(1.5, 30, DRAWN)], 1)
        Y = X @ R.T + t
        ok = (X[:, 2] >= DEPTH[0]) & (X[:, 2] <= DEPTH[1]) & (Y[:, 2] >= DEPTH[0]) & (Y[:, 2] <= DEPTH[1])
        kept.append(X[ok])
    X = np.concatenate(kept)[:planted]
    Y = X @ R.T + t
    q = (X / X[:, 2:]) @ Kq.T
    p = (Y / Y[:, 2:]) @ Kt.T
    q_xy = np.concatenate([q[:, :2], rng.uniform(0, 640, (unrelated, 2))]).astype(np.float32)
    t_xy = np.concatenate([p[:, :2], rng.uniform(0, 480, (unrelated, 2))]).astype(np.float32)
    n = planted + unrelated
    perm = rng.permutation(n)  # the train rows are shuffled: a record's two indices differ
    t_rows = np.empty_like(t_xy)
    t_rows[perm] = t_xy
    m = np.zeros(n, DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"], m["distance"] = np.arange(n), perm, rng.uniform(0, 1, n).astype(np.float32)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)
    F = np.linalg.inv(Kt).T @ (tx @ R) @ np.linalg.inv(Kq)
    F = (sign * F / np.linalg.norm(F)).astype(np.float32).reshape(9)
    mask = np.zeros(n, np.uint8)
    mask[:n if mask_all else planted] = 1
    return _freeze({"matches": m, "q_xy": q_xy, "t_xy": t_rows, "result": {"F": F, "hypothesis": 0}, "F": F, "mask": mask,
                    "cam_q": cam_q, "cam_t": cam_t, "R": R, "t": t, "planted": planted})


@functools.lru_cache(maxsize=None)
def reference(seed, sign=1, planted=DRAWN, unrelated=0, mask_all=False, max_depth=50.0, max_cos_parallax=0.99998):
    """The rule's output for a scene; read-only."""
    from sift_amd import cv

    s = scene(seed, sign, planted, unrelated, mask_all)
    return _freeze(cv.recover_pose(s["matches"], s["q_xy"], s["t_xy"], s["result"], s["mask"], s["cam_q"], s["cam_t"],
                                   max_depth, max_cos_parallax))


def rotation_angle(Ra, Rb):
    """The angle of Ra Rb^T, from the chord |Ra - Rb|_F = 2 sqrt 2 sin(angle / 2)."""
    d = np.asarray(Ra, np.float64).reshape(3, 3) - np.asarray(Rb, np.float64).reshape(3, 3)
    return 2.0 * np.arcsin(min(1.0, np.linalg.norm(d) / (2.0 * np.sqrt(2.0))))


def vector_angle(a, b):
    a, b = np.asarray(a, np.float64).reshape(3), np.asarray(b, np.float64).reshape(3)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))


def svd_route(F, cam_q, cam_t, R_true, t_true):
    """The independent route: E = Kt^T F Kq by matrix products, numpy.linalg.svd, cv::decomposeEssentialMat's four
    candidates, and the one nearest the ground truth."""
    E = kmat(cam_t).T @ np.asarray(F, np.float64).reshape(3, 3) @ kmat(cam_q)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    cands = [(U @ W @ Vt, U[:, 2]), (U @ W.T @ Vt, U[:, 2]), (U @ W @ Vt, -U[:, 2]), (U @ W.T @ Vt, -U[:, 2])]
    return min(cands, key=lambda c: rotation_angle(c[0], R_true) + vector_angle(c[1], t_true))


def pose_bytes(d):
    """The 80 bytes of sift_hip_pose_result for a cv.recover_pose dict."""
    from sift_amd import POSE_RESULT_DTYPE

    r = np.zeros(1, POSE_RESULT_DTYPE)
    r["R"][0], r["t"][0], r["in_front"], r["with_parallax"] = d["R"], d["t"], d["in_front"], d["with_parallax"]
    r["counts"][0], r["candidate"], r["fit"] = d["counts"], d["candidate"], d["fit"]
    return r.tobytes()
