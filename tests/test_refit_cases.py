"""The refit rule in numpy (sift_amd.cv.refit_* / refine_*; include/sift_hip.h, "Refit of the verified model"), on the
CPU: the mirror the device is held to byte for byte in tests/test_gpu_refit.py.

* Agreement with the float64 references.  On every case with >= 20 inliers one fit on the winner's inliers agrees with
  float32(cv.fundamental_lstsq(..., rank2=True)) / cv.homography_lstsq scaled to unit norm within 1e-6 absolute per
  entry after sign alignment: both are float64 solutions of the same well-separated problem (they differ by about
  1e-10), rounding a unit-norm entry to float32 moves it by at most 6e-8, and 1e-6 is 16 x that; a wrong column order
  or a missing denormalisation term shows at 1e-3 or more.  det: the float64 determinant of the normalised G after the
  rank-2 step is below 1e-12 |G|^3.
* The sweep count: a 9th sweep changes no float32 output on any case.
* The rule's own properties for every shape, and the summation order on the 2,500-record case.
"""
import numpy as np
import pytest

import refit_cases as rc

ALL = [(m, s) for m in rc.MODELS for s in rc.shapes(m)]
ALL_IDS = ["%s-%d+%d" % (m, s[0], s[1]) for m, s in ALL]
BIG = [(m, s) for m, s in ALL if s[0] >= 20]  # at least 20 planted pairs: at least 20 inliers
BIG_IDS = ["%s-%d+%d" % (m, s[0], s[1]) for m, s in BIG]


def points(model, shape):
    from sift_amd import cv

    m, q_xy, t_xy, _ = rc.CASES[model].case(*shape[:2])
    return cv._match_points(m, q_xy, t_xy)


@pytest.mark.parametrize("model,shape", BIG, ids=BIG_IDS)
def test_one_fit_agrees_with_the_float64_reference(model, shape):
    from sift_amd import cv

    r = rc.verified(model, shape)
    assert r["inliers"] >= 20
    pts, inl = points(model, shape), r["mask"] != 0
    fit, lstsq = rc.rules(model)[1], rc.rules(model)[3]
    got, valid = fit(pts, mask=r["mask"])
    assert valid and got.dtype == np.float32 and got.shape == (9,)
    ref = np.asarray(lstsq(pts[inl, :2], pts[inl, 2:]), np.float64).reshape(9)
    ref = (ref / np.linalg.norm(ref)).astype(np.float32)
    if np.dot(ref, got) < 0:
        ref = -ref
    err = float(np.abs(ref - got).max())
    print(model, shape, "max |refit - lstsq|", err)
    assert err <= 1e-6
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-6
    # through the records and their positions: the same bytes as through the gathered points
    m, q_xy, t_xy, _ = rc.CASES[model].case(*shape[:2])
    again, _ = fit(m, q_xy, t_xy, r["mask"])
    assert again.tobytes() == got.tobytes()
    if model == "fundamental":
        _, _, G = cv._refit("F", pts, r["mask"], detail=True)
        det = abs(float(np.linalg.det(G))) / float(np.linalg.norm(G)) ** 3
        print("det(G) / |G|^3", det)
        assert det < 1e-12
    else:  # w > 0 at the first fit record
        j0 = int(np.flatnonzero(inl)[0])
        assert float(got[6:] @ np.r_[pts[j0, :2], 1.0].astype(np.float64)) > 0


@pytest.mark.parametrize("model,shape", ALL, ids=ALL_IDS)
def test_one_more_sweep_changes_no_output(model, shape):
    from sift_amd import cv

    r = rc.verified(model, shape)
    pts = points(model, shape)
    name = rc.FIELD[model]
    a, va = cv._refit(name, pts, r["mask"])
    b, vb = cv._refit(name, pts, r["mask"], sweeps=cv.REFIT_SWEEPS + 1)
    assert va == vb and a.tobytes() == b.tobytes()
    assert cv.REFIT_SWEEPS == 8 and cv.REFIT_SLOTS == 256


@pytest.mark.parametrize("model,shape", ALL, ids=ALL_IDS)
def test_properties_of_the_rule(model, shape):
    m, q_xy, t_xy, _ = rc.CASES[model].case(*shape[:2])
    refine = rc.rules(model)[2]
    r0 = rc.verified(model, shape)
    r1, r3 = rc.refined(model, shape, 1), rc.refined(model, shape, 3)
    f = rc.FIELD[model]
    print(model, shape, "inliers", r0["inliers"], "->", r1["inliers"], "->", r3["inliers"], "accepted", r3["accepted"])
    # the count never decreases; the untouched fields stay; the list is the mask's
    assert r0["inliers"] <= r1["inliers"] <= r3["inliers"]
    for r in (r1, r3):
        assert (r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
            (r0["hypothesis"], r0["matches"], r0["valid_hypotheses"])
        assert r["inliers"] == int(r["mask"].sum()) or r["accepted"] == 0
        assert r["list"].tobytes() == m[r["mask"] != 0].tobytes()
        assert r[f].dtype == np.float32 and r["mask"].dtype == np.uint8
    # a rejected round changes no byte
    if r1["accepted"] == 0:
        assert rc.model_bytes(model, r1) == rc.model_bytes(model, r0) and r1["mask"].tobytes() == r0["mask"].tobytes()
        assert r1["inliers"] == r0["inliers"] and r3["accepted"] == 0
    # rounds = 3 is three calls with rounds = 1
    step, accepted = r0, 0
    for _ in range(3):
        step = refine(m, q_xy, t_xy, step, rc.MAX_ERROR, 1)
        accepted += step["accepted"]
    assert rc.model_bytes(model, step) == rc.model_bytes(model, r3) and step["mask"].tobytes() == r3["mask"].tobytes()
    assert (step["inliers"], accepted) == (r3["inliers"], r3["accepted"])
    # an empty record stays, whatever its mask says; so does a record the guided matchers would refuse
    if r0["hypothesis"] < 0:
        assert r1["accepted"] == 0 and not r1[f].any() and r1["inliers"] == 0
    for bad in (np.zeros(9, np.float32), np.r_[r0[f][:8], np.float32(np.nan)].astype(np.float32)):
        broken = dict(r0)
        broken[f] = bad
        out = refine(m, q_xy, t_xy, broken, rc.MAX_ERROR, 2)
        assert out["accepted"] == 0 and out[f].tobytes() == bad.tobytes() and out["mask"].tobytes() == r0["mask"].tobytes()
    emptied = dict(r0)
    emptied["hypothesis"] = -1
    out = refine(m, q_xy, t_xy, emptied, rc.MAX_ERROR, 1)
    assert out["accepted"] == 0 and rc.model_bytes(model, out) == rc.model_bytes(model, r0)


@pytest.mark.parametrize("model", rc.MODELS)
def test_fewer_fit_records_than_the_minimum_leave_the_input_unchanged(model):
    mod, need = rc.CASES[model], rc.NEED[model]
    m, q_xy, t_xy, _ = mod.case(*mod.MAIN[:2])
    fit, refine = rc.rules(model)[1], rc.rules(model)[2]
    r = dict(rc.verified(model, mod.MAIN))
    inl = np.flatnonzero(r["mask"])
    for keep in (need - 1, need):
        mask = np.zeros(len(m), np.uint8)
        mask[inl[:keep]] = 1
        got, valid = fit(m, q_xy, t_xy, mask)
        assert valid == (keep >= need) and got.any() == valid
        short = dict(r, mask=mask, inliers=keep)
        out = refine(m, q_xy, t_xy, short, rc.MAX_ERROR, 2)
        if keep < need:
            assert out["accepted"] == 0 and out["mask"].tobytes() == mask.tobytes() and out["inliers"] == keep
            assert rc.model_bytes(model, out) == rc.model_bytes(model, r)
    with pytest.raises(ValueError):
        refine(m, q_xy, t_xy, r, rc.MAX_ERROR, 0)
    with pytest.raises(ValueError):
        refine(m, q_xy, t_xy, r, rc.MAX_ERROR, 9)


@pytest.mark.parametrize("model", rc.MODELS)
def test_a_masked_record_with_a_nan_position_is_skipped(model):
    m, q_nan, t_xy, r, j = rc.nan_case(model)
    mod = rc.CASES[model]
    q_xy = mod.case(*mod.MAIN[:2])[1]
    fit, refine = rc.rules(model)[1], rc.rules(model)[2]
    got, valid = fit(m, q_nan, t_xy, r["mask"])
    without = r["mask"].copy()
    without[j] = 0
    want, _ = fit(m, q_xy, t_xy, without)  # the same fit set, no NaN anywhere
    assert valid and got.tobytes() == want.tobytes()
    out = refine(m, q_nan, t_xy, r, rc.MAX_ERROR, 1)
    assert out["mask"][j] == 0 or out["accepted"] == 0
    assert np.isfinite(out[rc.FIELD[model]]).all()


@pytest.mark.parametrize("model", rc.MODELS)
def test_records_beyond_count_never_enter(model):
    """The CAPPED buffer: a mask that marks tail records too gives the fit of the counted ones."""
    mod = rc.CASES[model]
    m, q_xy, t_xy, _ = mod.case(*mod.CAPPED[:2])
    buf, n = mod.capped(), len(m)
    r = rc.verified(model, mod.CAPPED)
    refine = rc.rules(model)[2]
    want = refine(buf[:n], q_xy, t_xy, r, rc.MAX_ERROR, 2)
    assert rc.model_bytes(model, want) == rc.model_bytes(model, rc.refined(model, mod.CAPPED, 2))
    long_mask = np.ones(len(buf), np.uint8)
    long_mask[:n] = r["mask"]
    got = refine(buf[:n], q_xy, t_xy, dict(r, mask=long_mask), rc.MAX_ERROR, 2)  # only mask[:n] is read
    assert rc.model_bytes(model, got) == rc.model_bytes(model, want) and got["mask"].tobytes() == want["mask"].tobytes()
    with_tail = rc.rules(model)[1](buf, q_xy, t_xy, long_mask)[0]
    assert with_tail.tobytes() != rc.rules(model)[1](buf[:n], q_xy, t_xy, r["mask"])[0].tobytes()  # the tail would show


def test_summation_order_on_more_records_than_one_slot_pass():
    """SUM: ~2,100 fit records over 256 slots.  The array code equals the header's order performed one scalar addition
    at a time, and differs from a plain left-to-right sum -- so the order is visible in these inputs."""
    from sift_amd import cv

    pts = points("fundamental", rc.SUM).astype(np.float64)
    fit = rc.verified("fundamental", rc.SUM)["mask"] != 0
    assert fit.sum() > 8 * 256 and len(pts) > 9 * 256
    col = pts[:, 0] * pts[:, 2] * 1e-3 + 0.1  # not exactly representable: the order shows
    got = cv._slot_sum(col[:, None], fit)[0]
    assert got == rc.slot_sum_by_the_book(col, fit)
    plain = 0.0
    for v in col[fit]:
        plain = plain + float(v)
    assert got != plain and abs(got - plain) < 1e-9 * abs(plain)
    two = cv._slot_sum_rows([col[:, None], (2 * col)[:, None]], fit)[0]
    inter = np.stack([col, 2 * col], 1).reshape(-1)
    slots = [0.0] * 256
    for j in np.flatnonzero(fit):
        slots[j % 256] = (slots[j % 256] + inter[2 * j]) + inter[2 * j + 1]
    assert two == rc.slot_sum_by_the_book(slots, np.ones(256, bool))
