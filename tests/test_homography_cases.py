"""The numpy mirror of homography verification (sift_amd.cv.homography_samples / homography_from_4 / transfer_inliers /
ransac_homography / project_homography): the reference tests/test_gpu_homography.py holds the device to, checked here
on its own terms, and the inputs of tests/homography_cases.py.  No GPU.
"""
import numpy as np
import pytest

import homography_cases as hc

SEEDS = (0, 1, 2)


def unit(H):
    H = np.asarray(H, np.float64).reshape(-1)
    return H / np.linalg.norm(H)


@pytest.mark.parametrize("n", sorted({a + b for a, b, _ in hc.SHAPES if a + b >= 4} | {6, 64, 65, 65536}))
def test_samples_are_distinct_and_in_range(sift, n):
    from sift_amd import cv

    s = cv.homography_samples(n, 300, 3)
    assert s.dtype == np.int32 and s.shape == (300, 4)
    assert s.min() >= 0 and s.max() < n
    assert (np.diff(np.sort(s, axis=1), axis=1) > 0).all()  # 4 distinct indices in every row
    if n == 4:
        assert (np.sort(s, axis=1) == np.arange(4)).all()  # one possible sample set
    if n >= 64:
        assert len(np.unique(s)) > min(n, 1200) // 2  # the draws spread over the list


def test_samples_are_a_function_of_seed_k_n_only(sift):
    from sift_amd import cv

    a = cv.homography_samples(200, 64, 5)
    assert np.array_equal(a, cv.homography_samples(200, 64, 5))
    assert np.array_equal(a, cv.homography_samples(200, 512, 5)[:64])  # row k does not depend on K
    assert not np.array_equal(a, cv.homography_samples(200, 64, 6))
    assert not np.array_equal(a, cv.homography_samples(201, 64, 5))
    assert len({tuple(r) for r in a.tolist()}) == 64  # different k: different streams
    assert np.array_equal(cv.homography_samples(200, 8, 2 ** 32 + 5), a[:8])  # the seed is a uint32
    assert (cv.homography_samples(3, 4, 0) == -1).all() and cv.homography_samples(0, 4, 0).shape == (4, 4)
    # the fundamental sampler's first four draws: one shared stream, j = 0..3
    assert np.array_equal(a, cv.ransac_samples(200, 64, 5)[:, :4])


def test_solver_reproduces_the_true_homography(sift):
    """4 exact pairs (float64 images under H_true, rounded to float32 only): H_true up to scale to about 1e-4, the sign
    that puts sample 0 in front."""
    from sift_amd import cv

    Ht = hc.homography()
    q = np.float32([[20, 30], [170, 25], [160, 180], [30, 150]])
    t = hc.apply(Ht, q).astype(np.float32)
    H, ok = cv.homography_from_4(q, t)
    assert ok and H.dtype == np.float32 and H.shape == (9,)
    assert abs(np.linalg.norm(H.astype(np.float64)) - 1) < 1e-6
    assert np.abs(H.astype(np.float64) - unit(Ht)).max() < 1e-4
    assert (H[6] * q[0, 0] + H[7] * q[0, 1]) + H[8] > 0
    # float64 input is rounded to float32 once; every intermediate is float32 (the mirror asserts its own dtypes)
    H64, ok64 = cv.homography_from_4(q.astype(np.float64), t.astype(np.float64))
    assert ok64 and H64.dtype == np.float32 and H64.tobytes() == H.tobytes()
    # batched form = single form
    Hb, okb = cv.homography_from_4(np.stack([q, q[::-1]]), np.stack([t, t[::-1]]))
    assert Hb.shape == (2, 9) and okb.all() and Hb[0].tobytes() == H.tobytes()
    assert np.abs(Hb[1].astype(np.float64) - unit(Ht)).max() < 1e-4


def test_degenerate_samples_are_invalid(sift):
    from sift_amd import cv

    Ht = hc.homography()
    q = np.float32([[20, 30], [170, 25], [160, 180], [30, 150]])
    t = hc.apply(Ht, q).astype(np.float32)
    assert cv.homography_from_4(q, t)[1]
    line = q.copy()
    line[2] = (q[0] + q[1]) / 2  # three collinear query points: a zero area
    H, ok = cv.homography_from_4(line, t)
    assert not ok and not H.any()
    H, ok = cv.homography_from_4(q, t[[0, 1, 1, 3]])  # a repeated train point
    assert not ok and not H.any()
    flipped = t.copy()
    flipped[[0, 1]] = t[[1, 0]]  # two neighbouring train corners swapped: three triples flip, (0, 2, 3) does not
    H, ok = cv.homography_from_4(q, flipped)
    assert not ok and not H.any()
    mirrored = t.copy()
    mirrored[:, 0] = 200 - t[:, 0]  # a reflection flips all four orientations alike: a valid sample
    H, ok = cv.homography_from_4(q, mirrored)
    assert ok and np.linalg.det(H.astype(np.float64).reshape(3, 3)) < 0
    bad = q.copy()
    bad[3, 1] = np.nan
    for a, b in ((bad, t), (q, np.where(np.isnan(bad), np.nan, t))):
        H, ok = cv.homography_from_4(a, b)
        assert not ok and not H.any()


def test_transfer_inliers_hand_case(sift):
    """q = (7, 2), max_error = 2: under I train (9, 2) sits on the edge (dx dx == e2 w w == 4) and counts, (9.25, 2)
    does not, (7, 4) does; 2 I gives the same answers (the predicate is scale-free for w > 0); -I has w < 0: nothing."""
    from sift_amd import cv

    m = np.zeros(3, sift.DMATCH_DTYPE)
    m["trainIdx"] = [0, 1, 2]
    q_xy, t_xy = np.float32([[7, 2]]), np.float32([[9, 2], [9.25, 2], [7, 4]])
    eye = np.eye(3, dtype=np.float32)
    got = cv.transfer_inliers(m, q_xy, t_xy, eye, 2.0)
    assert got.dtype == bool and got.tolist() == [True, False, True]
    assert cv.transfer_inliers(m, q_xy, t_xy, 2 * eye, 2.0).tolist() == [True, False, True]
    assert cv.transfer_inliers(m, q_xy, t_xy, -eye, 2.0).tolist() == [False, False, False]
    assert not cv.transfer_inliers(m, q_xy, t_xy, np.zeros(9), 2.0).any()  # w == 0 is not in front
    assert not cv.transfer_inliers(m, q_xy, t_xy, np.full(9, np.nan), 2.0).any()
    pad = lambda a, s: np.c_[a, np.full((len(a), s - 2), np.nan, np.float32)]  # noqa: E731
    assert np.array_equal(cv.transfer_inliers(m, pad(q_xy, 3), pad(t_xy, 5), eye, 2.0), got)
    bad = np.zeros(4, sift.DMATCH_DTYPE)
    bad["queryIdx"] = [0, -1, 1, 0]
    bad["trainIdx"] = [0, 0, 0, 2 ** 30]
    assert cv.transfer_inliers(bad, q_xy, t_xy, eye, 2.0).tolist() == [True, False, False, False]
    assert cv.transfer_inliers(m[:0], q_xy, t_xy, eye, 1.0).shape == (0,)
    with pytest.raises(ValueError):
        cv.transfer_inliers(m, q_xy, t_xy, np.zeros(8), 1.0)


def test_true_homography_separates_planted_from_outliers(sift):
    from sift_amd import cv

    m, q_xy, t_xy, planted = hc.case(*hc.MAIN[:2])
    got = cv.transfer_inliers(m, q_xy, t_xy, unit(hc.homography()).astype(np.float32), hc.MAX_ERROR)
    assert np.array_equal(got, planted)  # all 120 planted and none of the 80 outlier pairs


def test_project_homography(sift):
    from sift_amd import cv

    Ht = hc.homography()
    xy = np.float32([[20, 30], [170, 25], [0, 0], [199.75, 199.75]])
    got = cv.project_homography(unit(Ht).astype(np.float32), xy)
    assert got.dtype == np.float32 and got.shape == (4, 2)
    assert np.abs(got - hc.apply(Ht, xy)).max() < 1e-3
    assert np.array_equal(cv.project_homography(unit(Ht).astype(np.float32), np.c_[xy, np.full(4, np.nan)]), got)
    # w <= 0 gives NaN: H = [I; (0, -1, 3)] has w = 3 - y
    H = np.float32([1, 0, 0, 0, 1, 0, 0, -1, 3])
    p = cv.project_homography(H, np.float32([[4, 1], [4, 3], [4, 5], [np.nan, 1]]))
    assert p[0].tolist() == [2.0, 0.5] and np.isnan(p[1:]).all()
    assert np.isnan(cv.project_homography(np.zeros(9), xy)).all()  # the empty result projects to nothing
    assert np.isnan(cv.project_homography(-unit(Ht), xy)).all()
    assert cv.project_homography(H, np.zeros((0, 2), np.float32)).shape == (0, 2)


@pytest.mark.parametrize("seed", SEEDS)
def test_recovery_on_the_main_case(sift, seed):
    """The winner's inliers hold >= 95 % of the 120 planted pairs and at most 10 of the 80 outlier pairs (the bars of
    the fundamental test; this mirror reaches 1.0 and 0)."""
    n_in, n_out, K = hc.MAIN
    r = hc.reference(n_in, n_out, K, seed)
    planted = hc.case(n_in, n_out)[3]
    recall, false = hc.recovery(r["mask"], planted)
    print("seed", seed, "recall", recall, "false pairs", false, "valid", r["valid_hypotheses"])
    assert r["hypothesis"] >= 0 and r["inliers"] == int(r["mask"].sum()) == len(r["list"])
    assert recall >= 0.95 and false <= 10
    assert 0 < r["valid_hypotheses"] < K // 2  # the orientation test rejects most samples of this list


def test_reference_of_every_shape(sift):
    from sift_amd import cv

    for n_in, n_out, K in hc.SHAPES + [hc.LARGE]:
        m, q_xy, t_xy, planted = hc.case(n_in, n_out)
        n = n_in + n_out
        if n > 8:
            assert (m["queryIdx"] != np.arange(n)).mean() > 0.8  # the indirection is exercised
        r = hc.reference(n_in, n_out, K)
        assert set(r) == {"H", "inliers", "hypothesis", "matches", "valid_hypotheses", "mask", "list", "samples", "Hs",
                          "valid", "counts"}
        assert r["matches"] == n and r["samples"].shape == (K, 4) and r["Hs"].shape == (K, 9)
        assert r["Hs"].dtype == np.float32 and r["H"].dtype == np.float32 and r["mask"].dtype == np.uint8
        if n < 4:
            assert r["hypothesis"] == -1 and r["inliers"] == 0 and not r["H"].any() and len(r["list"]) == 0
            assert r["valid_hypotheses"] == 0 and not r["mask"].any() and len(r["mask"]) == n
            assert (r["samples"] == -1).all()
            continue
        k = r["hypothesis"]
        assert k >= 0 and r["valid"][k] and r["counts"][k] == r["counts"][r["valid"]].max()
        tied = np.flatnonzero(r["valid"] & (r["counts"] == r["counts"][k]))
        assert k == tied[0] and len(tied) > 1  # ties to the lowest k, and there are ties
        assert np.array_equal(r["list"], m[r["mask"] != 0])  # input records, input order
        assert np.array_equal(r["mask"] != 0, cv.transfer_inliers(m, q_xy, t_xy, r["H"], hc.MAX_ERROR))
        assert not r["Hs"][~r["valid"]].any() and not r["counts"][~r["valid"]].any()
        assert np.array_equal(r["mask"] != 0, planted)  # recall 1, no false pair, on every shape
        if n_out:
            assert r["valid_hypotheses"] < K  # some samples fail the orientation test
    assert hc.reference(*hc.MAIN)["hypothesis"] != hc.reference(*hc.MAIN, 1)["hypothesis"]


def test_homography_lstsq_refits_the_inliers(sift):
    from sift_amd import cv

    m, q_xy, t_xy, planted = hc.case(*hc.MAIN[:2])
    pts = cv._match_points(m[planted], q_xy, t_xy)
    H = cv.homography_lstsq(pts[:, :2], pts[:, 2:])
    assert H.dtype == np.float64 and H.shape == (3, 3) and H[2, 2] == 1
    assert np.abs(hc.apply(H, pts[:, :2]) - pts[:, 2:]).max() < 0.25  # the 0.25 grid's rounding
    assert np.abs(hc.apply(H, pts[:, :2]) - hc.apply(hc.homography(), pts[:, :2])).max() < 0.1
    with pytest.raises(ValueError):
        cv.homography_lstsq(pts[:3, :2], pts[:3, 2:])
