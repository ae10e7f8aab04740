"""Inputs shared by the refit tests (tests/test_refit_cases.py, tests/test_gpu_refit.py), on top of
tests/verify_cases.py, tests/homography_cases.py and tests/verify_batched_cases.py, which are imported and not edited.

A case is a list (a buffer of cap records and the number that count), its positions, and the verified state a refine
call starts from: the sift_amd.cv.ransac_* dict of the records that count.  The rule under test is
sift_amd.cv.refine_fundamental / refine_homography (include/sift_hip.h, "Refit of the verified model").

SHAPES: every shape of the verify tests, the 2113-record list (past the accept kernel's 1024-row chunks), and SUM --
    2,100 planted + 400 others: about 2,100 fit records, eight and nine per slot of the rule's 256, so the sequential
    part of a slot and the tree over the slots both carry weight.
CAPPED: 129 counted records at the head of a buffer of 200 whose tail holds valid-looking records.
NAN: MAIN with the position of the first inlier's query row replaced by NaN after verification, and the record's
    inlier count lowered by that one record, so the refit -- which must skip the record -- can still be accepted.
No case had to be replaced for an unseparated smallest eigenvalue.
"""
import functools

import numpy as np

import verify_batched_cases as bc

MODELS = bc.MODELS
CASES = bc.CASES
FIELD = {"fundamental": "F", "homography": "H"}
NEED = bc.SAMPLE
MAX_ERROR = 1.5
SUM = (2100, 400, 64)
LARGE = (1800, 313, 64)
ROUNDS = (1, 3)


def shapes(model):
    return list(CASES[model].SHAPES) + [LARGE, SUM]


def rules(model):
    """(ransac, one fit, the whole refine operation, the float64 least-squares reference) of a model."""
    from sift_amd import cv

    if model == "fundamental":
        return cv.ransac_fundamental, cv.refit_fundamental, cv.refine_fundamental, cv.fundamental_lstsq
    return cv.ransac_homography, cv.refit_homography, cv.refine_homography, cv.homography_lstsq


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def verified(model, shape, seed=0):
    """The ransac dict of a shape (the verify tests' own reference where they have one); read-only."""
    mod = CASES[model]
    if shape in mod.SHAPES:
        return mod.reference(*shape, seed)
    m, q_xy, t_xy, _ = mod.case(*shape[:2])
    return _freeze(rules(model)[0](m, q_xy, t_xy, MAX_ERROR, shape[2], seed))


@functools.lru_cache(maxsize=None)
def refined(model, shape, rounds):
    """The rule's output for a shape; read-only."""
    m, q_xy, t_xy, _ = CASES[model].case(*shape[:2])
    return _freeze(rules(model)[2](m, q_xy, t_xy, verified(model, shape), MAX_ERROR, rounds))


@functools.lru_cache(maxsize=None)
def nan_case(model):
    """(matches, q_xy with one NaN row, t_xy, the verified dict with that record's count taken off, the record)."""
    mod = CASES[model]
    m, q_xy, t_xy, _ = mod.case(*mod.MAIN[:2])
    r = dict(verified(model, mod.MAIN))
    j = int(np.flatnonzero(r["mask"])[0])
    q = q_xy.copy()
    q[m["queryIdx"][j]] = np.nan
    q.setflags(write=False)
    r["inliers"] = r["inliers"] - 1
    return m, q, t_xy, r, j


def model_bytes(model, d):
    return np.asarray(d[FIELD[model]], np.float32).tobytes()


def slot_sum_by_the_book(values, fit):
    """The header's summation order, one scalar addition at a time (independent of sift_amd.cv's array code)."""
    slots = [0.0] * 256
    for j, (v, f) in enumerate(zip(values, fit)):
        if f:
            slots[j % 256] = slots[j % 256] + float(v)
    groups = []
    for g in range(4):
        s = slots[64 * g: 64 * g + 64]
        d = 32
        while d >= 1:
            for i in range(d):
                s[i] = s[i] + s[i + d]
            d //= 2
        groups.append(s[0])
    return (groups[0] + groups[1]) + (groups[2] + groups[3])
