"""A bank of two-view scenes at frame size and under hard motions, with float64 truth, for the verifier family (verify,
score, refit, pose, projection): tests/test_geometry_bank.py holds sift_amd.cv (the numpy mirror of the device rules)
to independent float64 routes on it, tests/test_gpu_geometry_bank.py holds the device to the mirror byte for byte.

Every scene is generated in float64 and stored as float32 positions behind a DMATCH_DTYPE list that is shuffled and
indexes shuffled position arrays (the pattern of tests/verify_cases.make: SPARE rows no record uses, a distance per
record), and carries its ground truth: R, t (|t| = 1), the cameras (fx, fy, cx, cy), F or H, and the planted flags.
N_IN planted pairs, N_OUT pairs of independent uniform positions, K hypotheses, MAX_ERROR and SEED are the same for
every scene.  Gaussian position noise of SIGMA px is added on both sides of a fundamental scene unless it is
noise-free, and on the train side of a homography scene: the forward transfer error the rule scores is then that noise
whatever the map's scale (noise on a query position is carried over by H, four-fold under the zoom).

FUNDAMENTAL: the scenes of the fundamental matrix (see _F_SPECS for each one's motion); ILL_POSED is the fixed set
of those that are ill-posed for pose.  HOMOGRAPHY: the maps of the homography scenes, all on 1920 x 1200 but the last;
train positions are where the map puts them (outside the frame too, negative included), the outliers' train positions
are uniform over the planted ones' bounding box.  EDGES: 64-record (or shorter) lists without ground truth whose
values are huge, tiny, non-finite or degenerate.

The float64 routes below share no solver code with sift_amd.cv: the 8-point F and the 4-point H through
numpy.linalg.svd of the Hartley-normalised system (no rank-2 step, as the rule has none), the Sampson distance and
the forward transfer error, and a RANSAC route that draws the rule's samples (cv.ransac_samples /
cv.homography_samples, an integer rule), solves and scores in float64, breaks ties as the rule does and refits on its
inliers with cv.fundamental_lstsq / cv.homography_lstsq.  For the pose the route is tests/pose_cases.svd_route.

Bars (tests/test_geometry_bank.py).  B2: d = |f - f64| of the unit-norm 9-vectors up to sign is at most
256 u kappa, u = 2^-24, kappa = sigma_1 / sigma_8 of the float64 normalised 8 x 9 system -- the backward-error bound
of full-pivoting elimination on a 9-column system, of order n^2 u times the growth; 256 is about 3 n^2; vacuous above
kappa ~ 6.5e4.  The fundamental matrices are compared as the rule returns them.  The homographies are compared in the
normalised frame of their sample (in_the_normalised_frame): in pixel units the translation column of a unit-norm H
carries the float32 rounding of a 1000 px coordinate, about 6e-5 px, which is no solver error and exceeds u kappa
where kappa is below 10 (the identity scene: 637 u kappa in pixel units, 8.6 in the normalised frame).  B3: 1e-6 per
entry and det(G) < 1e-12 |G|^3 (tests/test_refit_cases.py).  B5: pose_cases.POSE_TOL.
B6: recall >= 0.95 and false pairs <= N_OUT / 8 after three refit rounds (tests/test_verify_cases.py).

Measured with the mirror (tests/test_geometry_bank.py prints them again):
    scene              B1 own sample  B2 max d/(u kappa)  B3 |refit - lstsq|  B6 recall, false: float64 route / mirror
    c1_752             0.00063 px     58.8                0                   1.000, 1 / 1.000, 1
    c2_1920            0.0016 px      44.6                0                   1.000, 0 / 1.000, 0
    c2_1920_clean      0.0016 px      39.3                0                   1.000, 0 / 1.000, 0
    big_4096           0.0042 px      8.69                0                   1.000, 1 / 1.000, 1
    forward            0.0011 px      123                 0                   1.000, 0 / 0.993, 0
    sideways           0.00097 px     72.4                0                   1.000, 2 / 1.000, 2
    rot30              0.0015 px      7.22                0                   1.000, 0 / 1.000, 0
    shallow            0.0046 px      30                  0                   1.000, 1 / 1.000, 1
    planar_exact       0.0016 px      139                 0.017 (no bar)      1.000, 4 / 1.000, 4
    small_baseline     0.0053 px      11.9                0                   1.000, 0 / 1.000, 0
    offset             0.043 px       20.5                0                   1.000, 0 / 1.000, 0
    identity           0.13 px        8.64                0                   0.987, 0 / 0.987, 0
    rot_pi             0.038 px       1.44                0                   0.987, 0 / 0.987, 0
    zoom_4             0.7 px         1.37                0                   0.987, 0 / 0.987, 0
    zoom_quarter       0.55 px        5.53                0                   0.993, 0 / 0.993, 0
    shift              0.35 px        6.07                0                   0.993, 0 / 0.993, 0
    perspective        0.43 px        1.37                0                   0.980, 0 / 0.980, 0
    mirror             0.21 px        2.33                0                   0.987, 0 / 0.987, 0
    perspective_4096   0.16 px        1.78                0                   0.987, 0 / 0.987, 0
    B5, pose from the refit of the planted records: (rotation, translation) rad to the route / to the truth
    c1_752             2.0e-08, 5.2e-09 / 6.2e-04, 1.1e-02
    c2_1920            1.8e-08, 6.9e-09 / 9.0e-04, 6.2e-04
    c2_1920_clean      1.8e-08, 7.5e-09 / 2.2e-08, 2.5e-08
    big_4096           2.5e-08, 7.0e-09 / 3.4e-05, 4.3e-04
    forward            2.3e-08, 2.8e-11 / 4.9e-04, 6.9e-04
    sideways           2.1e-08, 2.7e-10 / 1.6e-04, 9.3e-03
    rot30              2.9e-08, 5.0e-09 / 1.6e-03, 1.1e-03
    offset             2.1e-08, 1.0e-08 / 9.0e-04, 6.3e-04
B1 holds for the homography by the own-sample rule of include/sift_hip.h, which makes invalid two hypotheses of 779
otherwise valid ones (rot_pi 203 and zoom_4 125: one own pair each at 2.07 and 3.22 px; no float32 H can do better
there, see tests/test_geometry_bank.py).  B3 reads 0 where the refit and the float64 least squares round to the same nine float32 values.  B4: a 9th sweep changes no byte of the refit or
of decompose_essential on any scene, the ill-posed ones included.  small_baseline's chain gives the empty pose;
shallow and planar_exact give a pose that counts 133 and 75 of their records.  Value edges: x 2^-140, one_point and the
duplicate lists have no valid hypothesis; x 2^20 keeps 256 valid F hypotheses that count 5 records and no valid H
(at 2e9 px float32 resolves no 1.5 px, so none of the 75 solved samples counts itself);
in huge_and_inf the four records at 1e30 are inliers of the winner (both sides of the compare overflow to +inf, which
include/sift_hip.h now says) and the record at +inf is an inlier of nothing.
"""
import functools

import numpy as np

import epipolar_cases as ec
import homography_cases as hc
from verify_cases import SPARE, recovery  # noqa: F401  (the list pattern's spare rows; re-exported for the tests)

N_IN, N_OUT, K, MAX_ERROR, SEED, SIGMA = 150, 100, 256, 1.5, 0, 0.5
ROUNDS = 3
U = 2.0 ** -24
B2_FACTOR = 256.0
MIN_RECALL, MAX_FALSE = 0.95, N_OUT // 8
ILL_POSED = frozenset({"shallow", "planar_exact", "small_baseline"})
EDGE_N = 64

CAM_752 = (450.0, 450.0, 376.0, 240.0)
CAM_Q = (1150.0, 1170.0, 975.0, 590.0)   # the two cameras of the 1920 x 1200 scenes
CAM_T = (1210.0, 1190.0, 940.0, 615.0)
CAM_4096 = (2450.0, 2470.0, 2060.0, 1520.0)
OFFSET_Q, OFFSET_T = (-2000.0, 3000.0), (5000.0, -700.0)

# name: frame, cam_q, cam_t, rotation vector, t, depths, sigma, and the extras (plane: the points lie on
# homography_cases' plane; offset: added to every position of a side, and to that side's principal point)
_F_SPECS = {
    "c1_752": dict(frame=(752, 480), cam_q=CAM_752, cam_t=CAM_752, rvec=ec.RVEC, t=ec.T),
    "c2_1920": dict(),
    "c2_1920_clean": dict(sigma=0.0, like="c2_1920"),
    "big_4096": dict(frame=(4096, 3072), cam_q=CAM_4096, cam_t=CAM_4096),
    "forward": dict(t=(0.0, 0.0, 0.6)),                                   # the epipoles lie inside the frames
    "sideways": dict(t=(0.6, 0.0, 0.0), rvec=(5e-4, -8e-4, 3e-4)),       # the epipoles lie at infinity
    "rot30": dict(rvec=(0.1, 0.5, 0.1)),
    "shallow": dict(depth=(5.0, 5.05)),
    "planar_exact": dict(plane=True, sigma=0.0),
    "small_baseline": dict(t=tuple(0.05 * ec.T)),
    "offset": dict(like="c2_1920", offset=(OFFSET_Q, OFFSET_T)),
}
FUNDAMENTAL = tuple(_F_SPECS)


def _about(centre, M):
    C = np.array([[1.0, 0.0, centre[0]], [0.0, 1.0, centre[1]], [0.0, 0.0, 1.0]])
    return C @ np.asarray(M, np.float64) @ np.linalg.inv(C)


def _similarity(scale, angle):
    c, s = scale * np.cos(angle), scale * np.sin(angle)
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]


_PERSPECTIVE = [[1.0, 0.05, 0.0], [0.02, 1.0, 0.0], [4e-4, -3e-4, 1.0]]
_CENTRE = (960.0, 600.0)
# name: (frame, H)
_H_SPECS = {
    "identity": ((1920, 1200), np.eye(3)),
    "rot_pi": ((1920, 1200), _about(_CENTRE, _similarity(1.0, np.pi))),
    "zoom_4": ((1920, 1200), _about(_CENTRE, _similarity(4.0, 0.3))),
    "zoom_quarter": ((1920, 1200), _about(_CENTRE, _similarity(0.25, 0.3))),
    "shift": ((1920, 1200), np.array([[1.0, 0.0, 1900.0], [0.0, 1.0, -1100.0], [0.0, 0.0, 1.0]])),
    "perspective": ((1920, 1200), _about(_CENTRE, _PERSPECTIVE)),
    "mirror": ((1920, 1200), _about(_CENTRE, np.diag([-1.0, 1.0, 1.0]))),  # every sample flips its orientation
    "perspective_4096": ((4096, 3072), _about((2048.0, 1536.0), _PERSPECTIVE)),
}
HOMOGRAPHY = tuple(_H_SPECS)

EDGES = ("times_2p20", "times_2m20", "times_2m140", "huge_and_inf", "one_point", "query_on_a_line", "n8_duplicate",
         "n4_duplicate")
MODELS = ("fundamental", "homography")
FIELD = {"fundamental": "F", "homography": "H"}
SCENES = {"fundamental": FUNDAMENTAL, "homography": HOMOGRAPHY}


def kmat(cam):
    fx, fy, cx, cy = (float(v) for v in cam)
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _assemble(rng, a, b, box_q, box_t, n_out=N_OUT):
    """tests/verify_cases.make's list around planted positions a, b (n_in, 2): (matches, q_xy, t_xy, planted).  Every
    other position is uniform in its side's box (x0, y0, x1, y1)."""
    from sift_amd import DMATCH_DTYPE

    n_in = len(a)
    n = n_in + n_out
    rows = n + SPARE
    q_xy = rng.uniform(box_q[:2], box_q[2:], (rows, 2))
    t_xy = rng.uniform(box_t[:2], box_t[2:], (rows, 2))
    qrow, trow = rng.permutation(rows)[:n], rng.permutation(rows)[:n]  # record i's rows, before the list is shuffled
    q_xy[qrow[:n_in]], t_xy[trow[:n_in]] = a, b
    order = rng.permutation(n)
    m = np.zeros(n, DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"] = qrow[order], trow[order]
    m["distance"] = (100 + order).astype(np.float32)
    return m, q_xy.astype(np.float32), t_xy.astype(np.float32), order < n_in


@functools.lru_cache(maxsize=None)
def fundamental_scene(name):
    """A dict: matches, q_xy, t_xy, planted, cam_q, cam_t (float32), R, t (|t| = 1), F (3 x 3 float64 of unit norm,
    x_t^T F x_q = 0), frame, sigma; read-only."""
    spec = dict(_F_SPECS[name])
    like = spec.pop("like", name)  # the scene whose points this one repeats (with another noise or an offset)
    spec = {**_F_SPECS[like], **spec}
    frame = spec.get("frame", (1920, 1200))
    cam_q, cam_t = np.float64(spec.get("cam_q", CAM_Q)), np.float64(spec.get("cam_t", CAM_T))
    R = ec.rotation(np.float64(spec.get("rvec", ec.RVEC)))
    t = np.float64(spec.get("t", ec.T))
    depth, sigma = spec.get("depth", (3.0, 8.0)), spec.get("sigma", SIGMA)
    rng = np.random.default_rng(31000 + FUNDAMENTAL.index(like))
    Kq, Kt = kmat(cam_q), kmat(cam_t)
    a, b = np.zeros((0, 2)), np.zeros((0, 2))
    while len(a) < N_IN:
        uv = rng.uniform((0, 0), frame, (4 * N_IN, 2))
        rays = np.linalg.inv(Kq) @ np.c_[uv, np.ones(len(uv))].T
        z = hc.PLANE_D / (hc.PLANE_N @ rays) if spec.get("plane") else rng.uniform(*depth, len(uv))
        Y = Kt @ (R @ (rays * z) + t[:, None])
        s = (Y[:2] / Y[2]).T
        ok = (s >= 0).all(1) & (s < frame).all(1) & (Y[2] > 0) & (z > 0)
        a, b = np.r_[a, uv[ok]], np.r_[b, s[ok]]
    a, b = a[:N_IN], b[:N_IN]
    noise = rng.normal(0.0, 1.0, (2, N_IN, 2))  # drawn whatever sigma is: a clean scene is its noisy twin's points
    m, q_xy, t_xy, planted = _assemble(rng, a + sigma * noise[0], b + sigma * noise[1], (0, 0) + frame, (0, 0) + frame)
    oq, ot = spec.get("offset", ((0.0, 0.0), (0.0, 0.0)))
    q_xy, t_xy = (q_xy + np.float32(oq)).astype(np.float32), (t_xy + np.float32(ot)).astype(np.float32)
    cam_q, cam_t = cam_q + np.r_[0.0, 0.0, oq], cam_t + np.r_[0.0, 0.0, ot]
    F = np.linalg.inv(kmat(cam_t)).T @ _skew(t) @ R @ np.linalg.inv(kmat(cam_q))
    return _freeze(dict(name=name, model="fundamental", matches=m, q_xy=q_xy, t_xy=t_xy, planted=planted,
                        cam_q=cam_q.astype(np.float32), cam_t=cam_t.astype(np.float32), R=R, t=t / np.linalg.norm(t),
                        F=F / np.linalg.norm(F), frame=frame, sigma=sigma))


@functools.lru_cache(maxsize=None)
def homography_scene(name):
    """A dict: matches, q_xy, t_xy, planted, H (3 x 3 float64, H[2][2] = 1, x_t ~ H x_q), frame, sigma; read-only."""
    frame, H = _H_SPECS[name]
    H = np.asarray(H, np.float64) / H[2][2]
    rng = np.random.default_rng(32000 + HOMOGRAPHY.index(name))
    a = rng.uniform((0, 0), frame, (8 * N_IN, 2))
    a = a[np.c_[a, np.ones(len(a))] @ H[2] > 0.25][:N_IN]  # in front, clear of the horizon (it crosses the 4096 frame)
    b = transfer(H, a)
    box_t = tuple(b.min(0)) + tuple(b.max(0))
    noise = rng.normal(0.0, SIGMA, (N_IN, 2))  # on the train side, where the rule measures: see the module's text
    m, q_xy, t_xy, planted = _assemble(rng, a, b + noise, (0, 0) + frame, box_t)
    return _freeze(dict(name=name, model="homography", matches=m, q_xy=q_xy, t_xy=t_xy, planted=planted, H=H, frame=frame,
                        sigma=SIGMA))


def scene(model, name):
    return fundamental_scene(name) if model == "fundamental" else homography_scene(name)


@functools.lru_cache(maxsize=None)
def edge(name):
    """A value-edge list: a dict of matches, q_xy, t_xy (no ground truth); read-only.  The first EDGE_N records of
    c2_1920 and its position arrays, changed as the name says."""
    s = fundamental_scene("c2_1920")
    m, q, t = s["matches"][:EDGE_N].copy(), s["q_xy"].copy(), s["t_xy"].copy()
    qi, ti = m["queryIdx"], m["trainIdx"]
    if name.startswith("times_"):
        f = np.float32({"times_2p20": 2.0 ** 20, "times_2m20": 2.0 ** -20, "times_2m140": 2.0 ** -140}[name])
        q, t = q * f, t * f  # 2^-140: the positions are subnormal, their products underflow
    elif name == "huge_and_inf":
        q[qi[[3, 17, 29, 40]]] = 1e30
        t[ti[[3, 17, 29, 40]]] = 1e30
        q[qi[51]] = np.inf
        t[ti[51]] = np.inf
    elif name == "one_point":
        q[:], t[:] = q[qi[0]], t[ti[0]]
    elif name == "query_on_a_line":
        x = np.rint(q[:, 0] * 4) / 4
        q = np.stack([x, x], 1).astype(np.float32)  # y = x exactly: every signed area is an exact zero
    elif name in ("n8_duplicate", "n4_duplicate"):
        m = m[:8 if name == "n8_duplicate" else 4]
        q[m["queryIdx"][2]], t[m["trainIdx"][2]] = q[m["queryIdx"][0]], t[m["trainIdx"][0]]
    else:
        raise KeyError(name)
    return _freeze(dict(name=name, matches=m, q_xy=q, t_xy=t))


def points64(s, records=None):
    """(n, 4) float64 (qx, qy, tx, ty) of a scene's records (all, or those a bool mask marks): the stored float32
    positions, exactly."""
    m = s["matches"] if records is None else s["matches"][np.asarray(records, bool)]
    return np.c_[s["q_xy"][m["queryIdx"]], s["t_xy"][m["trainIdx"]]].astype(np.float64)


# --- the float64 routes

def _hartley(p):
    mean = p.mean(0)
    s = np.sqrt(2.0) / np.sqrt(((p - mean) ** 2).sum(1)).mean()
    return (p - mean) * s, np.array([[s, 0.0, -s * mean[0]], [0.0, s, -s * mean[1]], [0.0, 0.0, 1.0]])


def f8_svd(pts8):
    """(F (9,) of unit norm, kappa): the float64 8-point F of 8 pairs (8, 4) through the SVD of the normalised 8 x 9
    system, without a rank-2 step; kappa = sigma_1 / sigma_8 of that system."""
    (q, Tq), (t, Tt) = _hartley(pts8[:, :2]), _hartley(pts8[:, 2:])
    A = np.stack([t[:, 0] * q[:, 0], t[:, 0] * q[:, 1], t[:, 0], t[:, 1] * q[:, 0], t[:, 1] * q[:, 1], t[:, 1], q[:, 0],
                  q[:, 1], np.ones(8)], 1)
    _, sv, vt = np.linalg.svd(A)
    F = (Tt.T @ vt[8].reshape(3, 3) @ Tq).reshape(9)
    with np.errstate(divide="ignore"):
        return F / np.linalg.norm(F), float(sv[0] / sv[7])


def _area2(p, i, j, k):
    return (p[j, 0] - p[i, 0]) * (p[k, 1] - p[i, 1]) - (p[j, 1] - p[i, 1]) * (p[k, 0] - p[i, 0])


def h4_svd(pts4):
    """(H (9,) of unit norm with w > 0 at pair 0, kappa, oriented): the float64 4-point H of 4 pairs (4, 4) through
    the SVD of the normalised DLT system; oriented: the four point triples keep, or all flip, their orientation."""
    prod = [_area2(pts4[:, :2], *ijk) * _area2(pts4[:, 2:], *ijk) for ijk in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))]
    oriented = all(p > 0 for p in prod) or all(p < 0 for p in prod)
    (q, Tq), (t, Tt) = _hartley(pts4[:, :2]), _hartley(pts4[:, 2:])
    rows = []
    for (x, y), (u, v) in zip(q, t):
        rows += [[x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u], [0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, -v]]
    _, sv, vt = np.linalg.svd(np.array(rows))
    H = (np.linalg.inv(Tt) @ vt[8].reshape(3, 3) @ Tq).reshape(9)
    H = H / np.linalg.norm(H)
    if H[6] * pts4[0, 0] + H[7] * pts4[0, 1] + H[8] < 0:
        H = -H
    with np.errstate(divide="ignore"):
        return H, float(sv[0] / sv[7]), oriented


def in_the_normalised_frame(H, pts4):
    """Tt H Tq^-1 (9,): a homography of pixel positions carried into the Hartley frames of its sample (4, 4), where the
    condition number of the 4-point system is defined."""
    (_, Tq), (_, Tt) = _hartley(pts4[:, :2]), _hartley(pts4[:, 2:])
    return (Tt @ np.asarray(H, np.float64).reshape(3, 3) @ np.linalg.inv(Tq)).reshape(9)


def sampson(F, pts):
    """The Sampson distance (pixels) of (n, 4) pairs under F, in float64."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    xq, xt = np.c_[pts[:, :2], np.ones(len(pts))], np.c_[pts[:, 2:], np.ones(len(pts))]
    lq, lt = xq @ F.T, xt @ F
    return np.abs((xt * lq).sum(1)) / np.sqrt(lq[:, 0] ** 2 + lq[:, 1] ** 2 + lt[:, 0] ** 2 + lt[:, 1] ** 2)


def transfer(H, xy):
    """The images (n, 2) of positions (n, 2) under H, in float64."""
    p = np.c_[np.asarray(xy, np.float64), np.ones(len(xy))] @ np.asarray(H, np.float64).reshape(3, 3).T
    return p[:, :2] / p[:, 2:]


def transfer_error(H, pts):
    """The forward transfer error (pixels) of (n, 4) pairs under H, in float64; +inf where w is not > 0."""
    H = np.asarray(H, np.float64).reshape(3, 3)
    w = np.c_[pts[:, :2], np.ones(len(pts))] @ H[2]
    err = np.sqrt(((transfer(H, pts[:, :2]) - pts[:, 2:]) ** 2).sum(1))
    return np.where(w > 0, err, np.inf)


def residual(model, M, pts):
    return sampson(M, pts) if model == "fundamental" else transfer_error(M, pts)


def unit_distance(a, b):
    """|a - b| of two 9-vectors scaled to unit norm, up to sign."""
    a, b = np.asarray(a, np.float64).reshape(9), np.asarray(b, np.float64).reshape(9)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


@functools.lru_cache(maxsize=None)
def ransac64(model, name):
    """The float64 RANSAC route of a scene: a dict of models (K, 9), valid, counts, hypothesis, M (the winner), mask,
    and after ROUNDS least-squares refits on the inliers (kept while the count does not fall) refit and refit_mask."""
    from sift_amd import cv

    s = scene(model, name)
    pts = points64(s)
    n = len(pts)
    samples = (cv.ransac_samples if model == "fundamental" else cv.homography_samples)(n, K, SEED)
    models, valid = np.zeros((K, 9)), np.zeros(K, bool)
    for k in range(K):
        if model == "fundamental":
            models[k], kappa = f8_svd(pts[samples[k]])
            valid[k] = np.isfinite(kappa)
        else:
            models[k], kappa, oriented = h4_svd(pts[samples[k]])
            valid[k] = oriented and np.isfinite(kappa)
    passes = np.stack([residual(model, M, pts) <= MAX_ERROR for M in models]) & valid[:, None]
    counts = passes.sum(1)
    hyp = int(np.argmax(np.where(valid, counts, -1)))  # the first of the largest: ties to the lowest k
    M, mask = models[hyp], passes[hyp]
    lstsq = cv.fundamental_lstsq if model == "fundamental" else cv.homography_lstsq
    for _ in range(ROUNDS):
        if mask.sum() < (8 if model == "fundamental" else 4):
            break
        cand = np.asarray(lstsq(pts[mask, :2], pts[mask, 2:])).reshape(9)
        keep = residual(model, cand, pts) <= MAX_ERROR
        if keep.sum() < mask.sum():
            break
        M, mask = cand, keep
    return _freeze(dict(models=models, valid=valid, counts=counts, hypothesis=hyp, M=models[hyp], mask=passes[hyp],
                        refit=M, refit_mask=mask))


# --- the mirror's chain, computed once and shared

def rules(model):
    from sift_amd import cv

    if model == "fundamental":
        return cv.ransac_fundamental, cv.refit_fundamental, cv.refine_fundamental, cv.fundamental_lstsq
    return cv.ransac_homography, cv.refit_homography, cv.refine_homography, cv.homography_lstsq


def source(model, name):
    return edge(name) if name in EDGES else scene(model, name)


@functools.lru_cache(maxsize=None)
def verified(model, name, seed=SEED):
    """The mirror's ransac dict of a scene or value-edge list under a model; read-only."""
    s = source(model, name)
    with np.errstate(all="ignore"):
        return _freeze(rules(model)[0](s["matches"], s["q_xy"], s["t_xy"], MAX_ERROR, K, seed))


@functools.lru_cache(maxsize=None)
def refined(model, name, rounds=ROUNDS, seed=SEED):
    """The mirror's refine dict on verified(model, name, seed); read-only."""
    s = source(model, name)
    with np.errstate(all="ignore"):
        return _freeze(rules(model)[2](s["matches"], s["q_xy"], s["t_xy"], verified(model, name, seed), MAX_ERROR, rounds))


EDGE_CAMS = (np.float32(CAM_Q), np.float32(CAM_T))


@functools.lru_cache(maxsize=None)
def posed(name, rounds=ROUNDS):
    """The mirror's pose dict from the refined record of a fundamental scene or value-edge list; read-only."""
    from sift_amd import cv

    s = source("fundamental", name)
    r = refined("fundamental", name, rounds)
    cam_q, cam_t = (s["cam_q"], s["cam_t"]) if "cam_q" in s else EDGE_CAMS
    with np.errstate(all="ignore"):
        return _freeze(cv.recover_pose(s["matches"], s["q_xy"], s["t_xy"], r, r["mask"], cam_q, cam_t))
