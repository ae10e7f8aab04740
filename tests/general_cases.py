"""Inputs and float64 references shared by the general-path matcher tests (tests/test_match_general_cases.py on the
CPU, tests/test_gpu_match_general.py on the GPU) and by tools/general_path_accuracy.py.

The general path of the matcher (match_f16_block in csrc/sift_match_dev.h) takes every set that holds a value which is not
an integer 0..255.  The other matcher tests feed it values for which fp32 arithmetic is exact; the two families here
make fp32 round:

* ``sift_unrounded``: non-negative rows, L2-normalised, clipped at 0.2, renormalised, x512, cast to fp16 and not
  rounded to integers.  |q|^2 is about 262144, where fp32 resolves 1/32.
* ``learned``: Gaussian rows, L2-normalised, fp16; half the entries are negative, so sum |q_k t_k| far exceeds |q.t|.

Both have NQ = 300 queries and NT = 1100 train rows: k_match_single runs 9 splits of 4 tiles, the pair kernels 5 (2 in
the reverse direction) key-group splits, and the last tile is partial.  Planted in each family:

* 150 noisy copies of distinct query rows among the train rows (``planted``: (query, train) pairs);
* one exact duplicate, t[33] = q[1]; one double duplicate in different splits of every kernel, t[7] = t[900] = q[0];
  one duplicate in the last, partial tile, t[NT - 1] = q[2].

Every row has a position on the 0.25 grid of a 200 x 200 square (tests/guided_cases.py); a planted pair and each
duplicate are one 3-D point seen by the two cameras of tests/epipolar_cases.py, so they lie inside the band of
MAX_ERROR under its F and -- the disparity of that scene being below RADIUS -- inside each other's window.

The reference is D[i][t] = sum_k (q_k - t_k)^2 in float64 on the fp16 values, and the bound of include/sift_hip.h
B[i][t] = 136 * 2^-23 * (|q|^2 + |t|^2 + 2 sum_k |q_k| |t_k|).  A query is *decidable* when its three smallest
distances among its candidates are more than 2 max_t B[i][t] apart: only then are the indices pinned.

``fullrange()`` holds integer sets 0..255 of the same shape with the extreme rows (all 0, all 255, the 0/255
checkerboard and its complement, a single 255 spike) at the places where the integer keys are at the ends of their
range: train rows 255 and 511 (r = 255 inside a key group), NT - 1 (the partial tile, beside padding keys), different
splits, and among the queries.  Query FAR is an all-0 row whose window holds the two all-255 train rows only, so the
gated references contain d^2 = 128 * 255^2.
"""
import functools
import types

import numpy as np

import epipolar_cases as ec

NQ, NT = 300, 1100
RADIUS = 48.0
MAX_ERROR = ec.MAX_ERROR
FAMILIES = ("sift_unrounded", "learned")
FLT_MAX = np.finfo(np.float32).max
BOUND = 136 * 2.0 ** -23  # include/sift_hip.h: 127 additions + 9 combining operations, u = 2^-23
DUP_SINGLE, DUP_DOUBLE, DUP_LAST = (1, 33), (0, (7, 900)), (2, NT - 1)
MAX_D2 = 128 * 255 ** 2
GATES = ("none", "window", "band")


def _positions(rng, pairs):
    """Uniform grid positions for both sets; `pairs` (query row, train rows) are one scene point in both views."""
    q_xy = rng.integers(0, int(4 * ec.SIDE), (NQ, 2)) * 0.25
    t_xy = rng.integers(0, int(4 * ec.SIDE), (NT, 2)) * 0.25
    a, b = ec.project_pairs(rng, len(pairs))
    for (qi, ti), pa, pb in zip(pairs, a, b):
        q_xy[qi] = pa
        t_xy[ti] = pb  # ti may be a tuple of rows: the same position for each
    return q_xy.astype(np.float32), t_xy.astype(np.float32)


def make_family(family):
    """(q, t, q_xy, t_xy, planted): fp16 descriptor sets (NQ, 128) / (NT, 128), float32 positions, and the (150, 2)
    array of (query row, train row) noisy copies."""
    rng = np.random.default_rng({"sift_unrounded": 11, "learned": 12}[family])
    k = 150
    src = rng.permutation(np.arange(3, NQ))[:k]
    dst = rng.permutation(np.setdiff1d(np.arange(NT), [7, 33, 900, NT - 1]))[:k]
    amp = rng.uniform(0.25, 0.6, (k, 1))
    if family == "sift_unrounded":
        q = rng.gamma(0.7, 1.0, (NQ, 128))
        t = rng.gamma(0.7, 1.0, (NT, 128))
        t[dst] = q[src] * np.exp(amp * rng.standard_normal((k, 128)))

        def finish(v):
            v = v / np.linalg.norm(v, axis=1, keepdims=True)
            v = np.minimum(v, 0.2)
            return (512.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)
    elif family == "learned":
        q = rng.standard_normal((NQ, 128))
        t = rng.standard_normal((NT, 128))
        t[dst] = q[src] + amp * rng.standard_normal((k, 128))

        def finish(v):
            return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)
    else:
        raise ValueError(family)
    q, t = finish(q), finish(t)
    t[DUP_SINGLE[1]] = q[DUP_SINGLE[0]]
    t[list(DUP_DOUBLE[1])] = q[DUP_DOUBLE[0]]
    t[DUP_LAST[1]] = q[DUP_LAST[0]]
    pairs = [(int(s), int(d)) for s, d in zip(src, dst)] + [DUP_SINGLE, (DUP_DOUBLE[0], list(DUP_DOUBLE[1])), DUP_LAST]
    q_xy, t_xy = _positions(rng, pairs)
    return q, t, q_xy, t_xy, np.stack([src, dst], 1)


def distances(q, t):
    """D[i][t] = sum_k (q_k - t_k)^2 in float64, term by term (0 exactly for identical rows)."""
    a, b = np.asarray(q, np.float64), np.asarray(t, np.float64)
    D = np.empty((len(a), len(b)))
    for i0 in range(0, len(a), 64):
        D[i0:i0 + 64] = ((a[i0:i0 + 64, None, :] - b[None, :, :]) ** 2).sum(-1)
    return D


def bound(q, t):
    """B[i][t] of include/sift_hip.h."""
    a, b = np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(t, np.float64))
    return BOUND * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2.0 * (a @ b.T))


def gate_masks(q_xy, t_xy, F):
    from sift_amd import cv

    return {"none": np.ones((len(q_xy), len(t_xy)), bool), "window": cv.gate_mask(q_xy, t_xy, RADIUS),
            "band": cv.epipolar_mask(q_xy, t_xy, F, MAX_ERROR)}


def analyse(D, B, cand):
    """The float64 order of every query among its candidates: expect (n, 2) indices in (distance, index) order (-1:
    none), top (n, 3) smallest distances (inf: none), Bq (n,) and the decidable flags."""
    Dm = np.where(cand, D, np.inf)
    if Dm.shape[1] < 3:
        Dm = np.concatenate([Dm, np.full((len(Dm), 3 - Dm.shape[1]), np.inf)], 1)
    order = np.argsort(Dm, axis=1, kind="stable")[:, :3]
    top = np.take_along_axis(Dm, order, 1)
    expect = np.where(np.isfinite(top[:, :2]), order[:, :2], -1).astype(np.int32)
    Bq = B.max(1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isinf(top[:, 1:]), np.inf, top[:, 1:] - top[:, :-1])
    return types.SimpleNamespace(expect=expect, top=top, Bq=Bq, decidable=(gap[:, 0] > 2 * Bq) & (gap[:, 1] > 2 * Bq))


def measure_top2(idx2, d2, D, B, cand, ref=None):
    """A device top-2 (idx2 / d2, (n, 2)) against the contract of include/sift_hip.h, items 1 to 3.  Returns the
    figures (for profiles/general_path/accuracy.json) and `bad`, a dict of the rows that break each rule."""
    ref = ref or analyse(D, B, cand)
    n, nt = D.shape
    rows = np.arange(n)
    ncand = cand.sum(1)
    bad = {"negative": np.flatnonzero((d2 < 0).any(1)), "nan": np.flatnonzero(np.isnan(d2).any(1))}
    errs, ratios = [], []
    bad["none"] = bad["candidate"] = bad["bound"] = bad["index"] = np.zeros(0, np.int64)
    for k in (0, 1):
        has = ncand > k
        bad["none"] = np.union1d(bad["none"], rows[~has][(idx2[~has, k] != -1) | (d2[~has, k] != FLT_MAX)])
        j = idx2[has, k]
        ok = (j >= 0) & (j < nt)
        jj = np.where(ok, j, 0)
        ok &= cand[rows[has], jj]
        bad["candidate"] = np.union1d(bad["candidate"], rows[has][~ok])
        r, jj = rows[has][ok], jj[ok]
        err = np.abs(d2[r, k].astype(np.float64) - D[r, jj])
        errs.append(err)
        ratios.append(err / B[r, jj])
        bad["bound"] = np.union1d(bad["bound"], r[~(err <= B[r, jj])])
        bad["index"] = np.union1d(bad["index"], r[~(D[r, jj] <= ref.top[r, k] + 2 * ref.Bq[r])])
    two = ncand > 1
    bad["distinct"] = rows[two][idx2[two, 0] == idx2[two, 1]]
    differs = (idx2 != ref.expect).any(1)
    bad["decidable"] = np.flatnonzero(differs & ref.decidable)
    err, ratio = np.concatenate(errs), np.concatenate(ratios)
    stats = {"max_abs_err": float(err.max(initial=0.0)), "median_abs_err": float(np.median(err)) if len(err) else 0.0,
             "max_err_over_B": float(ratio.max(initial=0.0)), "negative_d2": int((d2 < 0).sum()),
             "nan_d2": int(np.isnan(d2).sum()), "decidable_share": float(ref.decidable.mean()),
             "undecidable_differing": int((differs & ~ref.decidable).sum())}
    return stats, bad


def check_top2(idx2, d2, D, B, cand, ref=None, label=""):
    """Assert items 1 to 3 of the contract; prints the figures first.  Returns them."""
    stats, bad = measure_top2(idx2, d2, D, B, cand, ref)
    print(label, stats)
    for rule, rows in bad.items():
        assert len(rows) == 0, (label, rule, rows[:8].tolist(), idx2[rows[:8]].tolist(), d2[rows[:8]].tolist())
    return stats


@functools.lru_cache(maxsize=None)
def case(family):
    """The sets of a family with, per direction ("fwd": q against t, "rev": t against q, under F^T), D, B and per
    gate the candidate mask and its float64 order.  Computed once and shared; every array is read-only."""
    q, t, q_xy, t_xy, planted = make_family(family)
    F = ec.fundamental()
    c = types.SimpleNamespace(family=family, q=q, t=t, q_xy=q_xy, t_xy=t_xy, F=F, planted=planted)
    D, B = distances(q, t), bound(q, t)
    c.fwd = types.SimpleNamespace(D=D, B=B, cand=gate_masks(q_xy, t_xy, F))
    c.rev = types.SimpleNamespace(D=np.ascontiguousarray(D.T), B=np.ascontiguousarray(B.T), cand=gate_masks(t_xy, q_xy, F.T))
    for d in (c.fwd, c.rev):
        d.ref = {g: analyse(d.D, d.B, d.cand[g]) for g in GATES}
        for a in [d.D, d.B] + list(d.cand.values()):
            a.setflags(write=False)
    for a in (q, t, q_xy, t_xy, F, planted):
        a.setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------------------------
# Full-range integer sets.
# ---------------------------------------------------------------------------------------------------------------
def extreme_rows():
    cb = np.tile([0.0, 255.0], 64)
    spike = np.zeros(128)
    spike[64] = 255
    return {"zero": np.zeros(128), "full": np.full(128, 255.0), "cb": cb, "cbc": 255.0 - cb, "spike": spike}


# Train rows: r = 255 inside a key group (255, 511), the partial tile (NT - 1), one row of every extreme kind in
# another split of the pair kernels (256 rows each) than its twin.
TRAIN_EXTREMES = {255: "full", 511: "zero", NT - 1: "full", 767: "zero", 256: "cb", 1023: "cb", 300: "cbc", 900: "cbc",
                  100: "spike", 1050: "spike"}
QUERY_EXTREMES = {0: "zero", 1: "full", 2: "cb", 3: "cbc", 4: "spike", 256: "zero", NQ - 1: "full"}
FAR = 5  # an all-0 query whose window holds train rows 255 and NT - 1 (all 255) and nothing else
MINUS_ZERO_QUERY, MINUS_ZERO_TRAIN = 40, 600  # rows that get a -0.0 in the general-path variant


def make_fullrange():
    rng = np.random.default_rng(13)
    ext = extreme_rows()

    def rows(n):
        v = rng.integers(0, 256, (n, 128)).astype(np.float64)
        sparse = np.minimum(rng.integers(0, 256, (n, 128)), 150) * (rng.random((n, 128)) >= 0.6)
        v[n // 2:] = sparse[n // 2:]
        return v

    q, t = rows(NQ), rows(NT)
    for i, name in TRAIN_EXTREMES.items():
        t[i] = ext[name]
    for i, name in QUERY_EXTREMES.items():
        q[i] = ext[name]
    q[FAR] = ext["zero"]
    q[MINUS_ZERO_QUERY, 17] = 0  # a zero to turn into -0.0
    t[MINUS_ZERO_TRAIN, 90] = 0
    q_xy, t_xy = _positions(rng, [(FAR, [255, NT - 1])])
    # Clear both windows: every other train row out of FAR's window, every other query out of the two rows' window.
    near = lambda xy, p: (np.abs(xy - p) <= RADIUS + 1).all(1)  # noqa: E731
    move = near(t_xy, q_xy[FAR])
    move[[255, NT - 1]] = False
    t_xy[move, 0] = (t_xy[move, 0] + ec.SIDE / 2) % ec.SIDE
    move = near(q_xy, t_xy[255])
    move[FAR] = False
    q_xy[move, 0] = (q_xy[move, 0] + ec.SIDE / 2) % ec.SIDE
    return q.astype(np.float32), t.astype(np.float32), q_xy, t_xy


@functools.lru_cache(maxsize=None)
def fullrange():
    """The full-range sets, F, and per direction and gate the int64 reference (sift_amd.cv.mask_top2): "none" is the
    all-true mask, "window" the window of RADIUS, "band" the epipolar band of MAX_ERROR inside that window."""
    from sift_amd import cv

    q, t, q_xy, t_xy = make_fullrange()
    F = ec.fundamental()
    c = types.SimpleNamespace(q=q, t=t, q_xy=q_xy, t_xy=t_xy, F=F)

    def refs(a, b, a_xy, b_xy, f):
        return {"none": cv.mask_top2(a, b, np.ones((len(a), len(b)), bool)),
                "window": cv.guided_top2(a, b, a_xy, b_xy, RADIUS),
                "band": cv.epipolar_top2(a, b, a_xy, b_xy, f, MAX_ERROR, RADIUS)}

    c.fwd, c.rev = refs(q, t, q_xy, t_xy, F), refs(t, q, t_xy, q_xy, F.T)
    for a in (q, t, q_xy, t_xy, F) + sum((r for d in (c.fwd, c.rev) for r in d.values()), ()):
        a.setflags(write=False)
    return c
