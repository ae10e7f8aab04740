"""The numpy mirror of two-view verification (sift_amd.cv.ransac_samples / fundamental_from_8 / sampson_inliers /
ransac_fundamental): the reference tests/test_gpu_verify.py holds the device to, checked here on its own terms, and the
inputs of tests/verify_cases.py.  No GPU.
"""
import numpy as np
import pytest

import epipolar_cases as ec
import verify_cases as vc

SEEDS = (0, 1, 2)


def sampson64(F, pts):
    """The Sampson distance (pixels) of (n, 4) pairs (qx, qy, tx, ty) under F, in float64."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64)
    xq, xt = np.c_[p[:, :2], np.ones(len(p))], np.c_[p[:, 2:], np.ones(len(p))]
    lq, lt = xq @ F.T, xt @ F
    return np.abs((xt * lq).sum(1)) / np.sqrt(lq[:, 0] ** 2 + lq[:, 1] ** 2 + lt[:, 0] ** 2 + lt[:, 1] ** 2)


@pytest.mark.parametrize("n", sorted({a + b for a, b, _ in vc.SHAPES if a + b >= 8} | {10, 64, 65, 65536}))
def test_samples_are_distinct_and_in_range(sift, n):
    from sift_amd import cv

    s = cv.ransac_samples(n, 300, 3)
    assert s.dtype == np.int32 and s.shape == (300, 8)
    assert s.min() >= 0 and s.max() < n
    assert (np.diff(np.sort(s, axis=1), axis=1) > 0).all()  # 8 distinct indices in every row
    if n == 8:
        assert (np.sort(s, axis=1) == np.arange(8)).all()  # one possible sample set
    if n >= 64:
        assert len(np.unique(s)) > min(n, 2400) // 2  # the draws spread over the list


def test_samples_are_a_function_of_seed_k_n_only(sift):
    from sift_amd import cv

    a = cv.ransac_samples(200, 64, 5)
    assert np.array_equal(a, cv.ransac_samples(200, 64, 5))
    assert np.array_equal(a, cv.ransac_samples(200, 512, 5)[:64])  # row k does not depend on K
    assert not np.array_equal(a, cv.ransac_samples(200, 64, 6))
    assert not np.array_equal(a, cv.ransac_samples(201, 64, 5))
    assert len({tuple(r) for r in a.tolist()}) == 64  # different k: different streams
    assert np.array_equal(cv.ransac_samples(200, 8, 2 ** 32 + 5), a[:8])  # the seed is a uint32
    assert (cv.ransac_samples(7, 4, 0) == -1).all() and cv.ransac_samples(0, 4, 0).shape == (4, 8)


def test_solver_fits_its_own_sample(sift):
    """For every valid hypothesis of the main case over 1024 hypotheses the float64 Sampson distance of each of its
    own 8 pairs is <= 0.01 px.  Measured with this mirror: 1024 of 1024 valid, worst 1.99e-4 px, median 2.0e-5."""
    from sift_amd import cv

    m, q_xy, t_xy, _ = vc.case(*vc.MAIN[:2])
    pts = cv._match_points(m, q_xy, t_xy)
    samples = cv.ransac_samples(len(m), 1024, 0)
    F, valid = cv.fundamental_from_8(pts[samples][:, :, :2], pts[samples][:, :, 2:])
    assert F.dtype == np.float32 and F.shape == (1024, 9) and valid.dtype == bool
    assert valid.sum() >= 1000
    assert np.allclose(np.sqrt((F[valid].astype(np.float64) ** 2).sum(1)), 1, atol=1e-6)
    worst = max(sampson64(F[k], pts[samples[k]]).max() for k in np.flatnonzero(valid))
    print("worst own-sample Sampson distance", worst)
    assert worst <= 0.01
    # the single-hypothesis form is the batched one
    f0, ok0 = cv.fundamental_from_8(pts[samples[0]][:, :2], pts[samples[0]][:, 2:])
    assert f0.dtype == np.float32 and ok0 == valid[0] and f0.tobytes() == F[0].tobytes()


def test_degenerate_samples_are_invalid(sift):
    from sift_amd import cv

    rng = np.random.default_rng(1)
    q = rng.uniform(0, 200, (8, 2)).astype(np.float32)
    t = rng.uniform(0, 200, (8, 2)).astype(np.float32)
    assert cv.fundamental_from_8(q, t)[1]
    same = np.repeat(q[:1], 8, 0)  # all points equal: mean distance 0, s = inf
    F, ok = cv.fundamental_from_8(same, t)
    assert not ok and not F.any()
    bad = q.copy()
    bad[3, 1] = np.nan
    F, ok = cv.fundamental_from_8(bad, t)
    assert not ok and not F.any()
    dup = q.copy()
    dup[1], tdup = dup[0], t.copy()
    tdup[1] = tdup[0]  # two identical rows: a zero pivot at the last step
    F, ok = cv.fundamental_from_8(dup, tdup)
    assert not ok and not F.any()


@pytest.mark.parametrize("seed", SEEDS)
def test_recovery_on_the_main_case(sift, seed):
    """The winner's inliers hold >= 95 % of the 120 planted pairs and at most 10 of the 80 outlier pairs."""
    n_in, n_out, K = vc.MAIN
    r = vc.reference(n_in, n_out, K, seed)
    planted = vc.case(n_in, n_out)[3]
    recall, false = vc.recovery(r["mask"], planted)
    print("seed", seed, "recall", recall, "false pairs", false)
    assert r["hypothesis"] >= 0 and r["inliers"] == int(r["mask"].sum()) == len(r["list"])
    assert recall >= 0.95 and false <= 10


def test_reference_of_every_shape(sift):
    from sift_amd import cv

    for n_in, n_out, K in vc.SHAPES:
        m, q_xy, t_xy, planted = vc.case(n_in, n_out)
        n = n_in + n_out
        if n > 8:
            assert (m["queryIdx"] != np.arange(n)).mean() > 0.8  # the indirection is exercised
        r = vc.reference(n_in, n_out, K)
        assert r["matches"] == n and r["samples"].shape == (K, 8) and r["Fs"].shape == (K, 9)
        if n < 8:
            assert r["hypothesis"] == -1 and r["inliers"] == 0 and not r["F"].any() and len(r["list"]) == 0
            assert r["valid_hypotheses"] == 0 and not r["mask"].any() and len(r["mask"]) == n
            continue
        k = r["hypothesis"]
        assert k >= 0 and r["valid"][k] and r["counts"][k] == r["counts"][r["valid"]].max()
        assert k == np.flatnonzero(r["valid"] & (r["counts"] == r["counts"][k]))[0]  # ties to the lowest k
        assert np.array_equal(r["list"], m[r["mask"] != 0])  # input records, input order
        assert np.array_equal(r["mask"] != 0, cv.sampson_inliers(m, q_xy, t_xy, r["F"], vc.MAX_ERROR))
        assert not r["Fs"][~r["valid"]].any() and not r["counts"][~r["valid"]].any()
        assert r["inliers"] >= 8 or n_in < 9
    assert vc.reference(*vc.MAIN)["hypothesis"] != vc.reference(*vc.MAIN, 1)["hypothesis"]


def test_sampson_inliers_hand_case_and_bad_records(sift):
    from sift_amd import cv

    h = ec.HAND
    m = np.zeros(3, sift.DMATCH_DTYPE)
    m["trainIdx"] = [0, 1, 2]
    got = cv.sampson_inliers(m, h["q_xy"], h["t_xy"], h["F"], h["max_error"])
    assert got.dtype == bool and got.tolist() == h["mask"][0]  # (4, 1) sits on the edge: inclusive
    diag = cv.epipolar_mask(h["q_xy"][m["queryIdx"]], h["t_xy"][m["trainIdx"]], h["F"], h["max_error"]).diagonal()
    assert np.array_equal(got, diag)
    assert np.array_equal(cv.sampson_inliers(m, ec.with_stride(h["q_xy"], 3), ec.with_stride(h["t_xy"], 5), h["F"],
                                             h["max_error"]), got)
    bad = np.zeros(4, sift.DMATCH_DTYPE)
    bad["queryIdx"] = [0, -1, 1, 0]
    bad["trainIdx"] = [0, 0, 0, 2 ** 30]
    assert cv.sampson_inliers(bad, h["q_xy"], h["t_xy"], h["F"], h["max_error"]).tolist() == [True, False, False, False]
    assert not cv.sampson_inliers(m, h["q_xy"], h["t_xy"], np.full(9, np.nan), h["max_error"]).any()
    assert cv.sampson_inliers(m[:0], h["q_xy"], h["t_xy"], h["F"], 1.0).shape == (0,)


def test_fundamental_lstsq_refits_the_inliers(sift):
    from sift_amd import cv

    n_in, n_out, K = vc.MAIN
    m, q_xy, t_xy, planted = vc.case(n_in, n_out)
    inl = m[planted]
    pts = cv._match_points(inl, q_xy, t_xy)
    F = cv.fundamental_lstsq(pts[:, :2], pts[:, 2:])
    assert F.dtype == np.float64 and F.shape == (3, 3) and abs(np.linalg.norm(F) - 1) < 1e-12
    assert np.linalg.svd(F)[1][2] < 1e-12  # rank 2
    assert np.median(sampson64(F, pts)) < 0.2  # the 0.25 grid's rounding
    assert np.linalg.svd(cv.fundamental_lstsq(pts[:, :2], pts[:, 2:], rank2=False))[1][2] > 0
    with pytest.raises(ValueError):
        cv.fundamental_lstsq(pts[:7, :2], pts[:7, 2:])
