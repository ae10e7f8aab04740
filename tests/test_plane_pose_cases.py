"""The plane pose rule (sift_amd.cv.recover_pose_homography; include/sift_hip.h, "Relative pose from a verified
homography") on the scenes of tests/plane_pose_cases.py, without a GPU: it recovers the planted pose, normal and
distance, all four candidates win somewhere, a plane's second valid pose shows as a tie in the counts, the outputs are a
rotation and unit vectors, every candidate reproduces the normalised homography, 8 sweeps are enough, -H and degenerate
inputs give the empty result, and unrelated records move the counts but not the winner.  The measured figures behind
PLANE_POSE_TOL are measured again here.
"""
import numpy as np
import pytest

import plane_pose_cases as pc

F32 = float(np.finfo(np.float32).eps)
ALL_SEEDS = pc.UNIQUE_SEEDS + pc.TIED_SEEDS


def truth(s):
    return s["R"], s["t"], s["n"], s["d"]


def full_candidates(r, planted):
    return [k for k in range(4) if r["counts"][k] == planted]


def figures(seed):
    """(rule to route, route to truth, rule to truth), each (rotation, translation, normal, relative distance); the
    rule's candidate is the winner, or for a tied scene the tied candidate nearest the truth."""
    s, r = pc.scene(seed), pc.reference(seed)
    cands = pc.candidate_tuples(r["candidates"])
    mine = pc.nearest([cands[k] for k in full_candidates(r, s["planted"])], *truth(s))[0]
    route = pc.svd_route(s["H"], s["cam_q"], s["cam_t"], *truth(s))
    return pc.errors(mine, *route), pc.errors(route, *truth(s)), pc.errors(mine, *truth(s))


@pytest.mark.parametrize("seed", pc.UNIQUE_SEEDS)
def test_unique_winner_counts_every_planted_record_and_strictly_more_than_the_others(seed):
    s, r = pc.scene(seed), pc.reference(seed)
    k = int(r["candidate"])
    assert 0 <= k <= 3 and r["fit"] == s["planted"] == pc.DRAWN
    assert r["counts"][k] == s["planted"] == r["in_front"], r["counts"]
    assert all(int(c) < s["planted"] for i, c in enumerate(r["counts"]) if i != k), r["counts"]
    assert r["mask"].all() and np.array_equal(r["list"], s["matches"])
    assert 0 < r["with_parallax"] <= r["in_front"]
    assert np.isfinite(r["points"]).all() and (r["points"][:, 2] > 0).all()
    c = r["candidates"][k]
    assert c["R"].tobytes() == r["R"].tobytes() and c["t"].tobytes() == r["t"].tobytes()
    assert c["normal"].tobytes() == r["normal"].tobytes() and c["distance"] == r["distance"]


def test_every_candidate_wins_somewhere():
    assert len(pc.UNIQUE_SEEDS) >= 6 and len(pc.TIED_SEEDS) >= 2
    assert {int(pc.reference(seed)["candidate"]) for seed in pc.UNIQUE_SEEDS} == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", pc.TIED_SEEDS)
def test_tied_scenes_have_exactly_two_full_candidates_and_the_first_wins(seed):
    s, r = pc.scene(seed), pc.reference(seed)
    full = full_candidates(r, s["planted"])
    assert len(full) == 2 and int(r["candidate"]) == full[0] and r["in_front"] == s["planted"], r["counts"]
    assert all(int(r["counts"][k]) < s["planted"] for k in range(4) if k not in full)


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_pose_and_plane_are_the_planted_ones_within_the_tolerance(seed):
    to_route, _, to_truth = figures(seed)
    print(f"seed {seed}: rule to route {['%.2e' % v for v in to_route]}, to truth {['%.2e' % v for v in to_truth]}, "
          f"PLANE_POSE_TOL {pc.PLANE_POSE_TOL:.2e}")
    assert max(to_truth) <= pc.PLANE_POSE_TOL and max(to_route) <= pc.PLANE_POSE_TOL


@pytest.mark.parametrize("seed", pc.UNIQUE_SEEDS)
def test_the_unique_winner_is_the_planted_pose(seed):
    s, r = pc.scene(seed), pc.reference(seed)
    e = pc.errors((r["R"], r["t"], r["normal"], r["distance"]), *truth(s))
    assert max(e) <= pc.PLANE_POSE_TOL, e


def test_measured_figures_stay_below_the_recorded_figure():
    """PLANE_POSE_TOL is 16 x MEASURED; MEASURED bounds the rule against the independent route and that route against
    the ground truth over all scenes (tests/plane_pose_cases.py records the figures)."""
    worst = max(max(max(a), max(b)) for a, b, _ in (figures(seed) for seed in ALL_SEEDS))
    print(f"largest measured figure {worst:.2e}, MEASURED {pc.MEASURED:.2e}")
    assert worst <= pc.MEASURED and pc.PLANE_POSE_TOL == 16 * pc.MEASURED


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_R_is_a_rotation_and_t_and_normal_are_unit_vectors(seed):
    r = pc.reference(seed)
    for c in list(r["candidates"]) + [r]:
        R = np.asarray(c["R"]).astype(np.float64).reshape(3, 3)
        # nine float32 roundings of entries of size <= 1: each row of R R^T - I and det - 1 move by a few ulps
        assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * F32
        assert abs(np.linalg.det(R) - 1.0) <= 4 * F32
        assert abs(np.linalg.norm(np.asarray(c["t"]).astype(np.float64)) - 1.0) <= 2 * F32
        assert abs(np.linalg.norm(np.asarray(c["normal"]).astype(np.float64)) - 1.0) <= 2 * F32
    assert r["R"].dtype == np.float32 and r["normal"].dtype == np.float32 and r["points"].dtype == np.float32
    assert np.asarray(r["distance"]).dtype == np.float32


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_every_candidate_reproduces_the_normalised_homography(seed):
    from sift_amd import cv

    s = pc.scene(seed)
    A = cv.calibrated_homography(s["H"], s["cam_q"], s["cam_t"])
    cands = cv.decompose_homography(A)
    assert len(cands) == 4
    Hn = A / np.linalg.svd(A, compute_uv=False)[1]
    for R, t, n, dist in cands:
        # float64 rounding of a handful of operations on entries of size about 1; the Jacobi routine's eigenvectors
        # are orthogonal to a few ulps
        assert np.abs(Hn - (R + np.outer(t, n) / dist)).max() <= 64 * np.finfo(np.float64).eps
    assert np.array_equal(cands[0][0], cands[2][0]) and np.array_equal(cands[0][1], -cands[2][1])
    assert np.array_equal(cands[1][2], -cands[3][2]) and cands[1][3] == cands[3][3]


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_a_ninth_sweep_changes_no_output(seed):
    from sift_amd import cv

    s, r = pc.scene(seed), pc.reference(seed)
    nine = cv.recover_pose_homography(s["matches"], s["q_xy"], s["t_xy"], s["result"], s["mask"], s["cam_q"], s["cam_t"],
                                      sweeps=9)
    assert pc.plane_pose_bytes(nine) == pc.plane_pose_bytes(r)
    assert nine["candidates"].tobytes() == r["candidates"].tobytes()
    assert nine["points"].tobytes() == r["points"].tobytes() and np.array_equal(nine["mask"], r["mask"])


def empty_ok(r, n, fit, decomposed=False):
    assert r["candidate"] == -1 and r["fit"] == fit and r["in_front"] == 0 and r["with_parallax"] == 0
    assert not r["R"].any() and not r["t"].any() and not r["counts"].any()
    assert not r["normal"].any() and r["distance"] == 0
    assert bool(r["candidates"].view(np.uint8).any()) == decomposed
    assert r["mask"].shape == (n,) and not r["mask"].any() and len(r["list"]) == 0
    assert r["points"].shape == (n, 3) and r["points"].view(np.uint32).tolist() == [[0x7FC00000] * 3] * n


def test_negated_H_gives_fit_zero_and_the_empty_result():
    from sift_amd import cv

    s = pc.scene(pc.UNIQUE_SEEDS[0])
    r = cv.recover_pose_homography(s["matches"], s["q_xy"], s["t_xy"], {"H": -s["H"], "hypothesis": 0}, s["mask"],
                                   s["cam_q"], s["cam_t"])
    empty_ok(r, len(s["matches"]), 0, decomposed=True)  # the candidates exist; no record is a fit record


def test_degenerate_inputs_give_the_empty_result():
    from sift_amd import cv

    seed = pc.UNIQUE_SEEDS[0]
    s = pc.scene(seed)
    n = len(s["matches"])

    def run(H=s["H"], hypothesis=0, mask=s["mask"], q_xy=s["q_xy"], matches=s["matches"]):
        return cv.recover_pose_homography(matches, q_xy, s["t_xy"], {"H": H, "hypothesis": hypothesis}, mask, s["cam_q"],
                                          s["cam_t"])

    empty_ok(run(hypothesis=-1), n, n)                                  # an empty record: w is still H's
    empty_ok(run(H=np.zeros(9, np.float32)), n, 0)                      # zero H: w = 0 for every record
    for bad in (np.nan, np.inf):                                        # non-finite H (an entry w does not read)
        H = s["H"].copy()
        H[4] = bad
        empty_ok(run(H=H), n, n)
    H = s["H"].copy()
    H[8] = np.nan                                                       # a NaN w is no fit record
    empty_ok(run(H=H), n, 0)
    empty_ok(run(H=pc.RANK1), n, n)                                     # rank 1: A^T A exactly diagonal, w2 = 0
    empty_ok(run(mask=np.zeros(n, np.uint8)), n, 0, decomposed=True)    # a mask of zeros
    empty_ok(run(matches=s["matches"][:0], mask=np.zeros(0, np.uint8)), 0, 0, decomposed=True)
    # masked records with NaN positions or indices outside the arrays are no fit records
    q = s["q_xy"].copy()
    q[:5] = np.nan
    m = s["matches"].copy()
    m["trainIdx"][5:9] = n + 7
    m["queryIdx"][9:11] = -1
    r = run(q_xy=q, matches=m)
    assert r["candidate"] == pc.reference(seed)["candidate"] and r["fit"] == n - 11 == r["in_front"]
    assert not r["mask"][:11].any() and r["mask"][11:].all() and np.isnan(r["points"][:11]).all()
    q[:] = np.nan
    empty_ok(run(q_xy=q), n, 0, decomposed=True)


def test_a_pure_rotation_is_a_plane_at_a_very_large_distance():
    """H = Kt R Kq^-1, t = 0.  The written rule sets no threshold on w1 - w3: after the float32 rounding of H the three
    eigenvalues differ by rounding, so the decomposition exists -- it is not the empty result.  The rotation is
    recovered, every candidate's distance exceeds 1e4 baselines, and no record has parallax."""
    from sift_amd import cv

    s = pc.scene(pc.UNIQUE_SEEDS[0])
    Kq, Kt = pc.kmat(s["cam_q"]), pc.kmat(s["cam_t"])
    H = Kt @ s["R"] @ np.linalg.inv(Kq)
    H = (H / np.linalg.norm(H)).astype(np.float32).reshape(9)
    q = s["q_xy"].astype(np.float64)
    rays = np.concatenate([q, np.ones((len(q), 1))], 1) @ np.linalg.inv(Kq).T @ s["R"].T @ Kt.T
    ok = rays[:, 2] > 0
    t_xy = np.zeros((len(q), 2), np.float32)
    t_xy[ok] = (rays[ok, :2] / rays[ok, 2:]).astype(np.float32)
    m = s["matches"].copy()
    m["trainIdx"] = m["queryIdx"]
    r = cv.recover_pose_homography(m, s["q_xy"], t_xy, {"H": H, "hypothesis": 0}, ok.astype(np.uint8), s["cam_q"],
                                   s["cam_t"])
    assert r["fit"] == int(ok.sum()) > 0
    assert r["candidates"].view(np.uint8).any() and (r["candidates"]["distance"] > 1e4).all()
    for c in r["candidates"]:
        assert pc.rotation_angle(c["R"], s["R"]) <= pc.PLANE_POSE_TOL
    assert r["with_parallax"] == 0


@pytest.mark.parametrize("seed", pc.TIED_SEEDS)
def test_unrelated_records_may_break_a_tie_but_change_no_candidate(seed):
    """In a tied scene a few unrelated records in front under one of the two may decide between them: the winner stays
    one of the two, and the candidates' bytes do not depend on the list."""
    clean, noisy = pc.reference(seed), pc.reference(seed, pc.DRAWN, 60, True)
    assert int(noisy["candidate"]) in full_candidates(clean, pc.DRAWN)
    assert noisy["candidates"].tobytes() == clean["candidates"].tobytes()
    c = noisy["candidates"][int(noisy["candidate"])]
    assert c["R"].tobytes() == noisy["R"].tobytes() and c["normal"].tobytes() == noisy["normal"].tobytes()


@pytest.mark.parametrize("seed", pc.UNIQUE_SEEDS)
def test_unrelated_records_change_the_counts_but_not_the_bytes_of_the_pose(seed):
    clean, noisy = pc.reference(seed), pc.reference(seed, pc.DRAWN, 60, True)
    k = int(clean["candidate"])
    assert int(noisy["candidate"]) == k and pc.DRAWN <= noisy["fit"] <= pc.DRAWN + 60
    assert not np.array_equal(noisy["counts"], clean["counts"])
    assert noisy["counts"][k] >= pc.DRAWN and noisy["mask"][:pc.DRAWN].all()
    for key in ("R", "t", "normal"):
        assert noisy[key].tobytes() == clean[key].tobytes()
    assert noisy["distance"] == clean["distance"] and noisy["candidates"].tobytes() == clean["candidates"].tobytes()


def test_thresholds_split_the_set():
    seed = pc.UNIQUE_SEEDS[0]
    s = pc.scene(seed)
    full = pc.reference(seed)
    depth = np.sort(full["points"][:, 2].astype(np.float64))
    near = pc.reference(seed, pc.DRAWN, 0, False, float(depth[len(depth) // 2]))
    assert 0 < near["in_front"] < full["in_front"]
    far = pc.reference(seed, pc.DRAWN, 0, False, float("inf"))
    assert far["in_front"] == full["in_front"]
    # the median cosine between the two rays of a record under the winner, by the steps
    from sift_amd import cv

    kq, kt = s["cam_q"].astype(np.float64), s["cam_t"].astype(np.float64)
    xq = (s["q_xy"].astype(np.float64) - kq[2:]) / kq[:2]
    xt = (s["t_xy"][s["matches"]["trainIdx"]].astype(np.float64) - kt[2:]) / kt[:2]
    cosine = cv.triangulate_depths(full["R"].astype(np.float64), full["t"].astype(np.float64), xq, xt)[3]
    tight = pc.reference(seed, pc.DRAWN, 0, False, 50.0, float(np.float32(np.median(cosine))))
    assert 0 < tight["with_parallax"] < full["with_parallax"] and tight["in_front"] == full["in_front"]
    assert len(s["matches"]) == pc.DRAWN


def test_steps_are_exposed_and_consistent():
    from sift_amd import cv

    seed = pc.UNIQUE_SEEDS[1]
    s, r = pc.scene(seed), pc.reference(seed)
    A = cv.calibrated_homography(s["H"], s["cam_q"], s["cam_t"])
    assert A.dtype == np.float64 and A.shape == (3, 3)
    ref = np.linalg.inv(pc.kmat(s["cam_t"])) @ s["H"].astype(np.float64).reshape(3, 3) @ pc.kmat(s["cam_q"])
    assert np.abs(A - ref).max() <= 1e-12 * np.abs(ref).max()
    cands = cv.decompose_homography(A)
    R, t, n, dist = cands[int(r["candidate"])]
    assert R.astype(np.float32).tobytes() == r["R"].tobytes() and t.astype(np.float32).tobytes() == r["t"].tobytes()
    assert n.astype(np.float32).tobytes() == r["normal"].tobytes() and np.float32(dist) == r["distance"]
    assert cv.decompose_homography(np.outer([1.0, 2.0, 3.0], [0.0, 0.0, 1.0])) == []
    assert cv.decompose_homography(np.eye(3)) == []  # w1 - w3 = 0
    # the third row of A on the normalised query ray is the w of H on the pixel
    kq = [float(v) for v in s["cam_q"]]
    x, y = (float(v) for v in s["q_xy"][0])
    w_a = A[2, 0] * ((x - kq[2]) / kq[0]) + A[2, 1] * ((y - kq[3]) / kq[1]) + A[2, 2]
    w_h = float(s["H"][6]) * x + float(s["H"][7]) * y + float(s["H"][8])
    assert abs(w_a - w_h) <= 1e-12 * abs(w_h) and w_h > 0
