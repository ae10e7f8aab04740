"""sift_amd.cv.ransac_essential / essential_from_5 (the rule of include/sift_hip.h, "Essential-matrix verification",
in numpy) against the ground truth of tests/essential_cases.py, on the CPU.  The independent route is numpy's own
linear algebra (det, matrix products, norms) on the float64 E the solver formed.  tests/test_gpu_essential.py holds
the device to this mirror byte for byte.
"""
import numpy as np
import pytest

import essential_cases as ec

SCENES = [("general", s) for s in ec.SEEDS] + [("plane", s) for s in ec.PLANE_SEEDS]
IDS = ["%s%d" % k for k in SCENES]


def unit(E, valid):
    n = np.linalg.norm(E, axis=2)
    return E / np.where(valid, n, 1.0)[:, :, None]


def test_minimal_sample_constraints():
    """Every valid slot of every sample of the general scenes: the five sample residuals, det E and the cubic
    constraint, on the unit-norm E, within 16 x the measured figure -- and the figure has not grown."""
    worst = 0.0
    for seed in ec.SEEDS:
        F, valid, E, z, q, t = ec.solved("general", seed)
        assert valid.any(1).sum() > ec.K // 2
        vi = np.nonzero(valid)
        res, det, cub = ec.constraint_figures(unit(E, valid)[vi], q[vi[0]], t[vi[0]])
        print("seed", seed, "slots", len(vi[0]), "residual %.3g det %.3g cubic %.3g" % (res.max(), det.max(), cub.max()))
        assert res.max() <= ec.CONSTRAINT_TOL and det.max() <= ec.CONSTRAINT_TOL and cub.max() <= ec.CONSTRAINT_TOL
        worst = max(worst, res.max(), det.max(), cub.max())
    assert worst <= ec.MEASURED_CONSTRAINT, worst


def test_every_clean_sample_holds_the_true_essential_matrix():
    """A condition, not a share: every sample whose five records are planted has a slot within CLEAN_TOL of [t]x R, up
    to sign and scale -- on the general scenes and on the plane-dominant ones."""
    worst = 0.0
    for kind, seed in SCENES:
        s, r = ec.get(kind, seed), ec.reference(kind, seed)
        F, valid, E, z, _, _ = ec.solved(kind, seed)
        clean = ec.clean_samples(r["samples"], s["planted"])
        d = ec.nearest_true(E, valid, ec.true_essential(s))
        print(kind, seed, "clean samples", int(clean.sum()), "worst %.3g" % d[clean].max())
        assert clean.sum() >= 32
        assert (d[clean] <= ec.CLEAN_TOL).all(), np.flatnonzero(clean & (d > ec.CLEAN_TOL))
        worst = max(worst, d[clean].max())
    assert worst <= ec.MEASURED_CLEAN, worst


def test_root_order_slot_numbering_and_invalid_slots():
    from sift_amd import cv

    for kind, seed in SCENES[:2] + SCENES[-1:]:
        r = ec.reference(kind, seed)
        F, valid, E, z, _, _ = ec.solved(kind, seed)
        # slots fill from 0 and their roots ascend
        for k in range(ec.K):
            zs = z[k][valid[k]]
            assert (np.diff(zs) > 0).all(), (k, zs)
        assert not F[~valid].any() and F[valid].any(1).all()
        # ransac_essential's model rows are the samples' slots, row 10 k + r
        assert r["Fs"].shape == (10 * ec.K, 9) and r["Fs"].tobytes() == F.reshape(-1, 9).tobytes()
        assert np.array_equal(r["valid"], valid.reshape(-1)) and r["valid_hypotheses"] == int(valid.sum())
        assert r["counts"].shape == (10 * ec.K,) and not r["counts"][~r["valid"]].any()
        nrm = np.linalg.norm(F[valid].astype(np.float64), axis=1)
        assert np.abs(nrm - 1).max() < 1e-6
        k, slot = divmod(r["hypothesis"], 10)
        assert valid[k, slot] and r["F"].tobytes() == F[k, slot].tobytes()
        assert r["inliers"] == r["counts"].max() == int(r["mask"].sum())
        assert r["hypothesis"] == int(np.flatnonzero(r["valid"] & (r["counts"] == r["inliers"]))[0])  # ties: lowest slot
        # a valid gap can only be a root whose model was not finite; on these scenes there is none
        assert all(valid[k, :valid[k].sum()].all() for k in range(ec.K))


def test_sampler():
    from sift_amd import cv

    for n, K, seed in ((5, 64, 0), (6, 64, 3), (360, 256, 0), (360, 256, 7), (1200, 65, 1)):
        s = cv.essential_samples(n, K, seed)
        assert s.shape == (K, 5) and s.dtype == np.int32 and s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 5 for row in s.tolist())
        assert np.array_equal(s, cv.essential_samples(n, K, seed))
        assert np.array_equal(s[:17], cv.essential_samples(n, 17, seed))  # row k is a function of (seed, k, n)
        assert np.array_equal(s, cv._samples(n, K, seed, 5))
        if n > 5:  # (n = 5: every row is a permutation of the five, and rows of two seeds can agree)
            assert not np.array_equal(s, cv.essential_samples(n, K, seed + 1))
    assert (cv.essential_samples(4, 8, 0) == -1).all()
    assert sorted(cv.essential_samples(5, 1, 0)[0].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("kind,seed", SCENES, ids=IDS)
def test_end_to_end_counts_every_planted_record_and_recovers_the_pose(kind, seed):
    """300 planted + 60 unrelated at K = 256: every planted record is counted, and cv.recover_pose on the record and
    mask gives the ground truth within POSE_TOL (looser than pose_cases.POSE_TOL: the minimal model is not refit)."""
    import pose_cases as pc

    s, r = ec.get(kind, seed), ec.reference(kind, seed)
    assert r["matches"] == 360 and r["mask"][:s["planted"]].all()
    assert r["mask"][s["planted"]:].sum() <= 2 and r["inliers"] == int(r["mask"].sum())
    assert ec.clean_samples(r["samples"], s["planted"])[r["hypothesis"] // 10]
    pose, ra, ta = ec.pose_error(kind, seed)
    print(kind, seed, "slot", r["hypothesis"], "rotation %.3g translation %.3g" % (ra, ta), "candidate", pose["candidate"])
    assert pose["candidate"] >= 0 and pose["in_front"] >= s["planted"]
    assert ra <= ec.POSE_TOL and ta <= ec.POSE_TOL
    assert max(ra, ta) <= ec.MEASURED_POSE
    assert ec.POSE_TOL > pc.POSE_TOL


def test_plane_scene_is_plane_dominant_in_the_recovered_structure():
    """The points cv.recover_pose triangulates from cv.ransac_essential's record on a plane scene: a plane fitted to
    the 240 records meant to lie on one leaves a residual of rounding size against the scene's depth, and the 60 others
    lie off it by baselines -- 80 % of the structure is one plane, and the solver was not stopped by it."""
    for seed in ec.PLANE_SEEDS:
        s = ec.plane_scene(seed)
        pose, _, _ = ec.pose_error("plane", seed)
        X = pose["points"][:s["planted"]].astype(np.float64)
        on = s["on_plane"]
        assert on.sum() == 240 and len(on) == 300 and np.isfinite(X).all()
        c = X[on].mean(0)
        normal = np.linalg.svd(X[on] - c)[2][2]
        dist = np.abs((X - c) @ normal)
        print("seed", seed, "on the plane: max %.3g, off it: median %.3g" % (dist[on].max(), np.median(dist[~on])))
        assert dist[on].max() < 1e-3 * np.linalg.norm(c)
        assert np.median(dist[~on]) > 1.0 and (dist[~on] > 100 * dist[on].max()).mean() > 0.9


def test_budget():
    """75 planted + 225 unrelated, RANSAC seeds 0..7: no K of {64 .. 1024} counts every planted record on every seed --
    at 25 % true pairs a 5-point sample is clean once in 1024 draws.  Pinned: the seeds that do at each K, and what
    each seed counts at K = 1024: 44 .. 75 of the 75.  (cv.ransac_fundamental at its limit of 4096 hypotheses, the
    nearest it comes to as many scored models, counts 22 .. 34 on seven of the eight seeds and 75 on one; README.)"""
    from sift_amd import cv

    s = ec.scene(ec.BUDGET_SCENE, *ec.BUDGET_SHAPE)
    planted = ec.BUDGET_SHAPE[0]
    full, found = [], None
    for K in ec.BUDGET_KS:
        counted = [int(cv.ransac_essential(s["matches"], s["q_xy"], s["t_xy"], s["cam_q"], s["cam_t"], ec.MAX_ERROR, K,
                                           seed)["mask"][:planted].sum()) for seed in ec.BUDGET_SEEDS]
        print("K", K, "planted records counted per seed", counted)
        full.append(sum(c == planted for c in counted))
        if found is None and full[-1] == len(ec.BUDGET_SEEDS):
            found = K
    assert found == ec.BUDGET_K
    assert tuple(full) == ec.BUDGET_FULL
    assert tuple(counted) == ec.BUDGET_PLANTED_1024


def edge(matches, q_xy, t_xy, K=16):
    from sift_amd import cv

    cam = np.float32([700, 710, 320, 240])
    return cv.ransac_essential(matches, q_xy, t_xy, cam, cam, ec.MAX_ERROR, K, 0)


def empty(r, n, K=16):
    return (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, n, 0) and not r["F"].any() \
        and not r["mask"].any() and len(r["list"]) == 0 and not r["valid"].any() and not r["Fs"].any() \
        and r["Fs"].shape == (10 * K, 9)


def test_edges():
    from sift_amd import DMATCH_DTYPE, cv

    s = ec.scene(ec.SEEDS[0])
    m, q, t = s["matches"], s["q_xy"], s["t_xy"]
    for n in (0, 4):
        r = edge(m[:n], q, t)
        assert empty(r, n) and (r["samples"] == -1).all()
    r = cv.ransac_essential(m[:5], q, t, s["cam_q"], s["cam_t"], ec.MAX_ERROR, 16, 0)
    assert r["matches"] == 5 and r["hypothesis"] >= 0 and r["inliers"] == 5  # a model through its own five
    assert (np.sort(r["samples"], 1) == np.arange(5)).all()
    # two identical records: the 5 x 9 system has rank 4, a zero pivot, no model
    two = m[[0, 1, 2, 3, 3]]
    r = cv.ransac_essential(two, q, t, s["cam_q"], s["cam_t"], ec.MAX_ERROR, 16, 0)
    F, valid = cv.essential_from_5(q[two["queryIdx"]], t[two["trainIdx"]], s["cam_q"], s["cam_t"])
    assert F.shape == (10, 9) and valid.shape == (10,)
    assert not valid.any() and not F.any() and empty(r, 5)
    # five collinear points on both sides: never an exception, and whatever is flagged valid is finite
    line = np.zeros(5, DMATCH_DTYPE)
    line["queryIdx"] = line["trainIdx"] = np.arange(5)
    lq = np.float32([[100 + 50 * i, 80 + 30 * i] for i in range(5)])
    lt = np.float32([[90 + 40 * i, 60 + 35 * i] for i in range(5)])
    r = edge(line, lq, lt)
    assert np.isfinite(r["Fs"]).all() and not r["Fs"][~r["valid"]].any() and r["matches"] == 5
    # a NaN position and an out-of-range index: the record counts for nothing, a sample that holds it has no model
    qn = q.copy()
    qn[m["queryIdx"][7], 1] = np.nan
    bad = m.copy()
    bad["trainIdx"][11] = len(t)
    for mm, qq in ((m, qn), (bad, q)):
        r = cv.ransac_essential(mm, qq, t, s["cam_q"], s["cam_t"], ec.MAX_ERROR, 256, 0)
        row = 7 if mm is m else 11
        assert not r["mask"][row] and r["hypothesis"] >= 0
        hit = (r["samples"] == row).any(1)
        assert hit.any() and not r["valid"].reshape(-1, 10)[hit].any()
        assert np.isfinite(r["Fs"]).all()
    with pytest.raises(ValueError):
        cv.ransac_essential(m, q, t, [0, 700, 320, 240], s["cam_t"])
