"""The numpy mirror of affine and similarity verification (sift_amd.cv.affine_samples / similarity_samples /
affine_from_3 / similarity_from_2 / affine_inliers / ransac_affine / refit_affine / refine_affine): the reference
tests/test_gpu_affine.py holds the device to, checked here on its own terms against the float64 truth
sift_amd.cv.affine_lstsq, and the inputs of tests/affine_cases.py.  No GPU.
"""
import numpy as np
import pytest

import affine_cases as ac

MODELS = pytest.mark.parametrize("similarity", ac.MODELS, ids=ac.MODEL_IDS)


@MODELS
def test_samples(sift, similarity):
    from sift_amd import cv

    m = ac.sample_size(similarity)
    draw = cv.similarity_samples if similarity else cv.affine_samples
    for n in (m, 6, 64, 200, 65536):
        s = draw(n, 300, 3)
        assert s.dtype == np.int32 and s.shape == (300, m)
        assert s.min() >= 0 and s.max() < n and (np.diff(np.sort(s, axis=1), axis=1) > 0).all()
    assert (draw(m - 1, 4, 0) == -1).all() and draw(0, 4, 0).shape == (4, m)
    # one shared stream: the fundamental sampler's first m draws
    assert np.array_equal(draw(200, 64, 5), cv.ransac_samples(200, 64, 5)[:, :m])


@MODELS
def test_minimal_solvers_agree_with_lstsq_on_exact_samples(sift, similarity):
    """Samples whose images are exact in float32 (grid positions under a map with dyadic entries): the closed form
    equals the float64 least-squares map to float32 rounding."""
    from sift_amd import cv

    M = np.array([[1.25, -0.5, 6.0], [0.5, 1.25, -4.0], [0, 0, 1]]) if similarity else \
        np.array([[1.25, 0.375, 6.0], [-0.25, 0.75, -4.0], [0, 0, 1]])
    q = np.float32([[20, 30], [170.25, 25.5], [160, 180.75]])[: ac.sample_size(similarity)]
    t = ac.apply(M, q).astype(np.float32)
    assert np.array_equal(t.astype(np.float64), ac.apply(M, q))  # exact
    solve = cv.similarity_from_2 if similarity else cv.affine_from_3
    A, ok = solve(q, t)
    assert ok and A.dtype == np.float32 and A.shape == (9,) and A[6:].tolist() == [0, 0, 1]
    truth = cv.affine_lstsq(q, t, similarity)
    assert truth.dtype == np.float64 and truth.shape == (3, 3)
    assert np.abs(truth - M).max() < 1e-9
    assert np.abs(A.astype(np.float64).reshape(3, 3) - truth).max() < 2e-5  # tx, ty: a few ulp of 200 * 1.25
    if similarity:
        assert A[0] == A[4] and A[1] == -A[3]
    # float64 input is rounded to float32 once; the batched form is the single form
    A64, ok64 = solve(q.astype(np.float64), t.astype(np.float64))
    assert ok64 and A64.tobytes() == A.tobytes()
    Ab, okb = solve(np.stack([q, q[::-1]]), np.stack([t, t[::-1]]))
    assert Ab.shape == (2, 9) and okb.all() and Ab[0].tobytes() == A.tobytes()
    assert np.abs(Ab[1].astype(np.float64).reshape(3, 3) - truth).max() < 2e-5


def test_degenerate_samples_are_invalid(sift):
    from sift_amd import cv

    q = np.float32([[20, 30], [170, 25], [160, 180]])
    t = ac.apply(ac.true_map(False), q).astype(np.float32)
    assert cv.affine_from_3(q, t)[1]
    line = q.copy()
    line[2] = (q[0] + q[1]) / 2
    for a, b in ((line, t), (q, t[[0, 1, 1]]), (q[[0, 0, 2]], t)):  # a collinear triple, a repeated point either side
        A, ok = cv.affine_from_3(a, b)
        assert not ok and not A.any()
    mirrored = t.copy()
    mirrored[:, 0] = 200 - t[:, 0]  # a reflection is a valid sample
    A, ok = cv.affine_from_3(q, mirrored)
    assert ok and np.linalg.det(A.astype(np.float64).reshape(3, 3)) < 0
    bad = q.copy()
    bad[2, 1] = np.nan
    for a, b in ((bad, t), (q, np.where(np.isnan(bad), np.nan, t))):
        A, ok = cv.affine_from_3(a, b)
        assert not ok and not A.any()
        A, ok = cv.similarity_from_2(a[1:], b[1:])
        assert not ok and not A.any()
    assert cv.similarity_from_2(q[:2], t[:2])[1]
    for a, b in ((q[[0, 0]], t[:2]), (q[:2], t[[1, 1]])):
        A, ok = cv.similarity_from_2(a, b)
        assert not ok and not A.any()


def test_affine_inliers_hand_case(sift):
    """q = (7, 2), max_error = 2: under I train (9, 2) sits on the edge (dx dx == 4) and counts, (9.25, 2) does not,
    (7, 4) does."""
    from sift_amd import cv

    m = np.zeros(3, sift.DMATCH_DTYPE)
    m["trainIdx"] = [0, 1, 2]
    q_xy, t_xy = np.float32([[7, 2]]), np.float32([[9, 2], [9.25, 2], [7, 4]])
    eye = np.eye(3, dtype=np.float32)
    got = cv.affine_inliers(m, q_xy, t_xy, eye, 2.0)
    assert got.dtype == bool and got.tolist() == [True, False, True]
    assert not cv.affine_inliers(m, q_xy, t_xy, np.full(9, np.nan), 2.0).any()
    bad = np.zeros(4, sift.DMATCH_DTYPE)
    bad["queryIdx"] = [0, -1, 1, 0]
    bad["trainIdx"] = [0, 0, 0, 2 ** 30]
    assert cv.affine_inliers(bad, q_xy, t_xy, eye, 2.0).tolist() == [True, False, False, False]
    assert cv.affine_inliers(m[:0], q_xy, t_xy, eye, 1.0).shape == (0,)
    with pytest.raises(ValueError):
        cv.affine_inliers(m, q_xy, t_xy, np.zeros(8), 1.0)


@MODELS
def test_reference_of_every_shape_and_transfer_predicate_equality(sift, similarity):
    """Every shape's dict, dtypes and selection rule; and affine_inliers == transfer_inliers under every hypothesis of
    every shape, so the record stays interchangeable with a homography record."""
    from sift_amd import cv

    m_size = ac.sample_size(similarity)
    for n_in, n_out, K in ac.SHAPES + [ac.LARGE]:
        m, q_xy, t_xy, planted = ac.case(n_in, n_out, similarity)
        n = n_in + n_out
        r = ac.reference(n_in, n_out, K, similarity)
        assert set(r) == {"H", "inliers", "hypothesis", "matches", "valid_hypotheses", "mask", "list", "samples", "Hs",
                          "valid", "counts"}
        assert r["matches"] == n and r["samples"].shape == (K, m_size) and r["Hs"].shape == (K, 9)
        assert r["samples"].dtype == np.int32 and r["counts"].dtype == np.int32
        assert r["Hs"].dtype == np.float32 and r["H"].dtype == np.float32 and r["mask"].dtype == np.uint8
        pts = cv._match_points(m, q_xy, t_xy)
        assert np.array_equal(cv._affine_pass(pts, r["Hs"], ac.MAX_ERROR), cv._transfer_pass(pts, r["Hs"], ac.MAX_ERROR))
        if n < m_size:
            assert r["hypothesis"] == -1 and r["inliers"] == 0 and not r["H"].any() and len(r["list"]) == 0
            assert r["valid_hypotheses"] == 0 and not r["mask"].any() and len(r["mask"]) == n
            assert (r["samples"] == -1).all()
            continue
        k = r["hypothesis"]
        assert k >= 0 and r["valid"][k] and r["counts"][k] == r["counts"][r["valid"]].max()
        assert k == np.flatnonzero(r["valid"] & (r["counts"] == r["counts"][k]))[0]  # ties to the lowest k
        assert np.array_equal(r["list"], m[r["mask"] != 0])  # input records, input order
        assert np.array_equal(r["mask"] != 0, cv.affine_inliers(m, q_xy, t_xy, r["H"], ac.MAX_ERROR))
        assert np.array_equal(r["mask"] != 0, cv.transfer_inliers(m, q_xy, t_xy, r["H"], ac.MAX_ERROR))
        assert not r["Hs"][~r["valid"]].any() and not r["counts"][~r["valid"]].any()
        assert (r["Hs"][r["valid"]][:, 6:] == [0, 0, 1]).all()
    assert ac.reference(*ac.MAIN, similarity)["hypothesis"] != ac.reference(*ac.MAIN, similarity, 1)["hypothesis"] or \
        not np.array_equal(ac.reference(*ac.MAIN, similarity)["samples"], ac.reference(*ac.MAIN, similarity, 1)["samples"])


@MODELS
def test_true_map_separates_planted_from_unrelated(sift, similarity):
    from sift_amd import cv

    m, q_xy, t_xy, planted = ac.case(*ac.MAIN[:2], similarity)
    got = cv.affine_inliers(m, q_xy, t_xy, ac.true_map(similarity).astype(np.float32), ac.MAX_ERROR)
    assert np.array_equal(got, planted)


@MODELS
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_recovery_on_the_main_case(sift, similarity, seed):
    r = ac.reference(*ac.MAIN, similarity, seed)
    planted = ac.case(*ac.MAIN[:2], similarity)[3]
    recall, false = ac.recovery(r["mask"], planted)
    print("similarity", similarity, "seed", seed, "recall", recall, "false pairs", false)
    assert r["hypothesis"] >= 0 and r["inliers"] == int(r["mask"].sum()) == len(r["list"])
    assert recall >= 0.95 and false <= 10


@MODELS
def test_budget_bar(sift, similarity):
    """20 % planted pairs: the similarity finds at least 57 of the 60 with K = 256 on every seed 0..7, the affine map
    with K = 1024."""
    n_in, n_out, _ = ac.BUDGET
    planted = ac.case(n_in, n_out, similarity)[3]
    found = []
    for seed in ac.BUDGET_SEEDS:
        r = ac.reference(n_in, n_out, ac.BUDGET_K[similarity], similarity, seed)
        found.append(int((r["mask"].astype(bool) & planted).sum()))
    print("similarity", similarity, "K", ac.BUDGET_K[similarity], "planted pairs found", found)
    assert ac.BUDGET_K == {True: 256, False: 1024}
    assert min(found) >= ac.BUDGET_BAR


@MODELS
def test_degenerate_list_rejects_some_samples(sift, similarity):
    from sift_amd import cv

    m, q_xy, t_xy, planted, _ = ac.degenerate(similarity)
    assert len(m) == 24 + 9 + 12 + 6
    r = cv.ransac_affine(m, q_xy, t_xy, ac.MAX_ERROR, ac.DEGENERATE_K, 0, similarity)
    print("similarity", similarity, "valid", r["valid_hypotheses"], "of", ac.DEGENERATE_K)
    assert 0 < r["valid_hypotheses"] < ac.DEGENERATE_K
    assert ac.recovery(r["mask"], planted) == (1.0, 0)


@MODELS
@pytest.mark.parametrize("seed", range(8))
def test_refit_lowers_the_planted_rms_and_is_accepted(sift, similarity, seed):
    from sift_amd import cv

    m, q_xy, t_xy, planted = ac.case(*ac.MAIN[:2], similarity)
    r, f = ac.reference(*ac.MAIN, similarity, seed), ac.refined(*ac.MAIN, similarity, seed)
    before, after = ac.rms(r["H"], m, q_xy, t_xy, planted), ac.rms(f["H"], m, q_xy, t_xy, planted)
    print("similarity", similarity, "seed", seed, "rms", before, "->", after)
    assert f["accepted"] == 1 and f["inliers"] >= r["inliers"] and after < before
    assert f["H"].dtype == np.float32 and f["H"][6:].tolist() == [0, 0, 1] and f["mask"].dtype == np.uint8
    # the refit is the float64 least-squares map of the fit set, to float32 rounding
    pts = cv._match_points(m[r["mask"] != 0], q_xy, t_xy)
    truth = cv.affine_lstsq(pts[:, :2], pts[:, 2:], similarity)
    assert np.abs(f["H"].astype(np.float64).reshape(3, 3) - truth).max() < 1e-5
    two = cv.refine_affine(m, q_xy, t_xy, r, ac.MAX_ERROR, 2, similarity)
    assert two["accepted"] in (1, 2) and two["inliers"] >= f["inliers"]


@MODELS
def test_refit_edges(sift, similarity):
    """Below the minimum, on one line (affine) or at one point (similarity): no refit.  A rejected round changes
    nothing.  An empty record stays empty."""
    from sift_amd import cv

    m, q_xy, t_xy, planted, kind = ac.degenerate(similarity)
    pts = cv._match_points(m, q_xy, t_xy)
    few = np.zeros(len(m), np.uint8)
    few[np.flatnonzero(planted)[: ac.sample_size(similarity) - 1]] = 1
    A, ok = cv.refit_affine(pts, mask=few, similarity=similarity)
    assert not ok and not A.any()
    flat = kind == (2 if similarity else 1)
    assert flat.sum() == (6 if similarity else 12)
    A, ok = cv.refit_affine(pts, mask=flat.astype(np.uint8), similarity=similarity)
    assert not ok and not A.any()
    if similarity:  # a line is enough for a similarity
        A, ok = cv.refit_affine(pts, mask=(kind == 1).astype(np.uint8), similarity=True)
        assert ok and np.abs(A.astype(np.float64).reshape(3, 3) - ac.true_map(True)).max() < 0.5
    shape, max_error, seed = ac.REJECTED[similarity]
    r = ac.reference(*shape, similarity, seed, max_error)
    f = ac.refined(*shape, similarity, seed, 2, max_error)
    cm, cq, ct, _ = ac.case(*shape[:2], similarity)
    assert cv.refit_affine(cm, cq, ct, r["mask"], similarity)[1]  # a valid candidate that counts fewer
    assert f["accepted"] == 0 and f["H"].tobytes() == r["H"].tobytes() and np.array_equal(f["mask"], r["mask"])
    empty = cv.ransac_affine(cm[:1], cq, ct, ac.MAX_ERROR, 8, 0, similarity)
    e = cv.refine_affine(cm[:1], cq, ct, empty, ac.MAX_ERROR, 1, similarity)
    assert e["accepted"] == 0 and e["hypothesis"] == -1 and not e["H"].any()
    with pytest.raises(ValueError):
        cv.refine_affine(cm, cq, ct, r, max_error, 9, similarity)
    with pytest.raises(ValueError):
        cv.affine_lstsq(np.zeros((1, 2)), np.zeros((1, 2)), similarity)
