"""The batch shared by the batched guided-matching tests (tests/test_guided_batched_cases.py,
tests/test_gpu_match_guided_batched.py, tests/test_gpu_match_guided_batched_cxx.py).

One batch per gate, pair p built by the single-pair generators with its own seed:

* SHAPES: tests/guided_cases.py's seven shapes -- a single row on either side, a partial query block, two query blocks,
  several key groups with more than one split -- and two empty pairs, (0, 50) and (50, 0).
* window batch: make_guided(nq, nt, seed) per pair, the call's radius guided_cases.RADIUS.
* epipolar batch: make_epipolar(nq, nt, seed) per pair and F_p = fundamental() * SCALES[p], constants without a factor
  of two, so the nine floats differ between pairs in every mantissa; then three DEGENERATE pairs of 33 x 31 whose
  records are all zero, hold one +Inf and hold one NaN: sift_amd.cv.geometry_usable is False for them and they must
  come out empty.

The reference of pair p is sift_amd.cv.guided_top2 / epipolar_top2 of both directions (the reverse under F^T) --
nothing at all for a pair whose geometry is not usable -- and sift_amd.cv.filter_matches with img_idx = p.  Seeds are
chosen so that every pair of at least 33 queries has a query with two or more candidates and one with none
(tests/test_guided_batched_cases.py asserts it).
"""
import functools

import numpy as np

import epipolar_cases as ec
import guided_cases as gc

SHAPES = list(gc.SHAPES) + [(0, 50), (50, 0)]
DEGENERATE = ("zero", "inf", "nan")
SCALES = (1.0, 3.0, 0.7, 5.0, 1.3, 11.0, 0.9, 7.0, 1.7, 1.0, 1.0, 1.0)
WINDOW_SEEDS = tuple(range(11, 11 + len(SHAPES)))
EPIPOLAR_SEEDS = tuple(range(21, 21 + len(SHAPES) + len(DEGENERATE)))
FLT_MAX = gc.FLT_MAX


def _sliced(make, nq, nt, seed):
    """The generator's sets for a shape; an empty side is a 50 x 50 case cut to no rows (the generators need rows)."""
    if nq and nt:
        return make(nq, nt, seed)[:4]
    q, t, q_xy, t_xy = make(50, 50, seed)[:4]
    return q[:nq], t[:nt], q_xy[:nq], t_xy[:nt]


def nothing(n):
    return np.full((n, 2), -1, np.int32), np.full((n, 2), FLT_MAX, np.float32)


@functools.lru_cache(maxsize=None)
def window_batch():
    """A tuple of pairs: dict(q, t, q_xy, t_xy, fwd, rev), every array read-only."""
    from sift_amd import cv

    pairs = []
    for (nq, nt), seed in zip(SHAPES, WINDOW_SEEDS):
        q, t, q_xy, t_xy = _sliced(gc.make_guided, nq, nt, seed)
        fwd = cv.guided_top2(q, t, q_xy, t_xy, gc.RADIUS)
        rev = cv.guided_top2(t, q, t_xy, q_xy, gc.RADIUS)
        pairs.append(_frozen(dict(q=q, t=t, q_xy=q_xy, t_xy=t_xy, fwd=fwd, rev=rev)))
    return tuple(pairs)


def degenerate_F(kind):
    F = ec.fundamental().copy()
    if kind == "zero":
        F[:] = 0
        F[1, 1] = -0.0  # a negative zero is a zero
    elif kind == "inf":
        F[1, 1] = np.inf
    else:
        F[2, 1] = np.nan
    return F


@functools.lru_cache(maxsize=None)
def epipolar_batch():
    """A tuple of pairs: dict(q, t, q_xy, t_xy, F, usable, fwd, rev); the last three are DEGENERATE."""
    from sift_amd import cv

    shapes = SHAPES + [(33, 31)] * len(DEGENERATE)
    pairs = []
    for p, ((nq, nt), seed) in enumerate(zip(shapes, EPIPOLAR_SEEDS)):
        q, t, q_xy, t_xy = _sliced(ec.make_epipolar, nq, nt, seed)
        if p < len(SHAPES):
            F = (ec.fundamental() * np.float32(SCALES[p])).astype(np.float32)
        else:
            F = degenerate_F(DEGENERATE[p - len(SHAPES)])
        usable = cv.geometry_usable(F)
        if usable:
            fwd = cv.epipolar_top2(q, t, q_xy, t_xy, F, ec.MAX_ERROR)
            rev = cv.epipolar_top2(t, q, t_xy, q_xy, np.ascontiguousarray(F.T), ec.MAX_ERROR)
        else:
            fwd, rev = nothing(nq), nothing(nt)
        pairs.append(_frozen(dict(q=q, t=t, q_xy=q_xy, t_xy=t_xy, F=F, usable=usable, fwd=fwd, rev=rev)))
    return tuple(pairs)


def _frozen(pair):
    for v in pair.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return pair


def batch(kind):
    return window_batch() if kind == "window" else epipolar_batch()


def expected_top2(kind):
    """(idx2, d2, match) of the whole batch in sift_hip_match_batched's layout (ratio 0.8 on distances)."""
    from sift_amd import cv

    pairs = batch(kind)
    idx2 = np.concatenate([p["fwd"][0] for p in pairs])
    d2 = np.concatenate([p["fwd"][1] for p in pairs])
    return idx2, d2, np.where(cv._ratio_pass(idx2, d2, 0.8, False), idx2[:, 0], -1).astype(np.int32)


def expected_lists(kind, **filter):
    """Per pair the DMATCH_DTYPE records (imgIdx = p) of sift_amd.cv.filter_matches on its two top-2 arrays."""
    from sift_amd import cv

    return [cv.filter_matches(*p["fwd"], *p["rev"], img_idx=i, **filter) for i, p in enumerate(batch(kind))]


def geometry_records(stride_bytes):
    """The epipolar batch's nine floats per pair in records of stride_bytes: 36 packs them, 52 is a
    VERIFY_RESULT_DTYPE array (the other fields hold a pattern the kernel must not read as F)."""
    pairs = epipolar_batch()
    rec = np.full((len(pairs), stride_bytes // 4), 0x7FC00123, np.uint32)  # NaN patterns behind the nine floats
    for i, p in enumerate(pairs):
        rec[i, :9] = p["F"].reshape(-1).view(np.uint32)
    return rec
