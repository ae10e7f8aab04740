"""The pose rule (sift_amd.cv.recover_pose; include/sift_hip.h, "Relative pose from a verified fundamental matrix") on
the scenes of tests/pose_cases.py, without a GPU: it recovers the planted pose, all four candidates win somewhere, F and
-F agree, the outputs are a rotation and a unit vector, 8 sweeps are enough, degenerate inputs give the empty result, and
unrelated records move the counts but not the winner.  The measured angles behind POSE_TOL are measured again here.
"""
import numpy as np
import pytest

import pose_cases as pc

SCENES = [(seed, sign) for seed in pc.SEEDS for sign in pc.SIGNS]
F32 = float(np.finfo(np.float32).eps)


def angles(seed, sign):
    """(rule to route, route to truth, rule to truth), each (rotation, translation)."""
    s, r = pc.scene(seed, sign), pc.reference(seed, sign)
    Rs, ts = pc.svd_route(s["F"], s["cam_q"], s["cam_t"], s["R"], s["t"])
    return ((pc.rotation_angle(r["R"], Rs), pc.vector_angle(r["t"], ts)),
            (pc.rotation_angle(Rs, s["R"]), pc.vector_angle(ts, s["t"])),
            (pc.rotation_angle(r["R"], s["R"]), pc.vector_angle(r["t"], s["t"])))


@pytest.mark.parametrize("seed,sign", SCENES)
def test_winner_counts_every_planted_record_and_the_others_none(seed, sign):
    s, r = pc.scene(seed, sign), pc.reference(seed, sign)
    k = int(r["candidate"])
    assert 0 <= k <= 3 and r["fit"] == s["planted"] == pc.DRAWN
    assert r["counts"][k] == s["planted"] == r["in_front"], r["counts"]
    assert [int(c) for i, c in enumerate(r["counts"]) if i != k] == [0, 0, 0], r["counts"]
    assert r["mask"].all() and np.array_equal(r["list"], s["matches"])
    assert 0 < r["with_parallax"] <= r["in_front"]
    assert np.isfinite(r["points"]).all() and (r["points"][:, 2] > 0).all()


def test_every_candidate_wins_somewhere():
    assert {int(pc.reference(seed, sign)["candidate"]) for seed, sign in SCENES} == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", pc.SEEDS)
def test_negated_F_gives_the_same_pose_through_the_swapped_candidate(seed):
    a, b = pc.reference(seed, 1), pc.reference(seed, -1)
    assert int(a["candidate"]) ^ 1 == int(b["candidate"])  # -F swaps R1 and R2
    assert pc.rotation_angle(a["R"], b["R"]) <= pc.POSE_TOL and pc.vector_angle(a["t"], b["t"]) <= pc.POSE_TOL
    assert np.array_equal(a["mask"], b["mask"]) and a["in_front"] == b["in_front"]


@pytest.mark.parametrize("seed,sign", SCENES)
def test_pose_is_the_planted_one_within_the_tolerance(seed, sign):
    to_route, _, to_truth = angles(seed, sign)
    print(f"seed {seed} sign {sign}: rule to route {to_route[0]:.2e} {to_route[1]:.2e} rad, to truth {to_truth[0]:.2e} "
          f"{to_truth[1]:.2e} rad, POSE_TOL {pc.POSE_TOL:.2e}")
    assert max(to_truth) <= pc.POSE_TOL and max(to_route) <= pc.POSE_TOL


def test_measured_angles_stay_below_the_recorded_figure():
    """POSE_TOL is 16 x MEASURED; MEASURED bounds the rule against the independent route and that route against the
    ground truth over all scenes (tests/pose_cases.py records the figures)."""
    worst = max(max(max(a), max(b)) for a, b, _ in (angles(seed, sign) for seed, sign in SCENES))
    print(f"largest measured angle {worst:.2e} rad, MEASURED {pc.MEASURED:.2e}")
    assert worst <= pc.MEASURED and pc.POSE_TOL == 16 * pc.MEASURED


@pytest.mark.parametrize("seed,sign", SCENES)
def test_R_is_a_rotation_and_t_a_unit_vector(seed, sign):
    r = pc.reference(seed, sign)
    R = r["R"].astype(np.float64).reshape(3, 3)
    # nine float32 roundings of entries of size <= 1: each row of R R^T - I and det - 1 move by a few ulps
    assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * F32
    assert abs(np.linalg.det(R) - 1.0) <= 4 * F32
    assert abs(np.linalg.norm(r["t"].astype(np.float64)) - 1.0) <= 2 * F32
    assert r["R"].dtype == np.float32 and r["t"].dtype == np.float32 and r["points"].dtype == np.float32


@pytest.mark.parametrize("seed,sign", SCENES)
def test_a_ninth_sweep_changes_no_output(seed, sign):
    from sift_amd import cv

    s, r = pc.scene(seed, sign), pc.reference(seed, sign)
    nine = cv.recover_pose(s["matches"], s["q_xy"], s["t_xy"], s["result"], s["mask"], s["cam_q"], s["cam_t"], sweeps=9)
    assert pc.pose_bytes(nine) == pc.pose_bytes(r)
    assert nine["points"].tobytes() == r["points"].tobytes() and np.array_equal(nine["mask"], r["mask"])


def empty_ok(r, n, fit):
    assert r["candidate"] == -1 and r["fit"] == fit and r["in_front"] == 0 and r["with_parallax"] == 0
    assert not r["R"].any() and not r["t"].any() and not r["counts"].any()
    assert r["mask"].shape == (n,) and not r["mask"].any() and len(r["list"]) == 0
    assert r["points"].shape == (n, 3) and r["points"].view(np.uint32).tolist() == [[0x7FC00000] * 3] * n


def test_degenerate_inputs_give_the_empty_result():
    from sift_amd import cv

    s = pc.scene(1)
    n = len(s["matches"])

    def run(F=s["F"], hypothesis=0, mask=s["mask"], q_xy=s["q_xy"], matches=s["matches"]):
        return cv.recover_pose(matches, q_xy, s["t_xy"], {"F": F, "hypothesis": hypothesis}, mask, s["cam_q"], s["cam_t"])

    empty_ok(run(hypothesis=-1), n, n)                                  # an empty record
    empty_ok(run(F=np.zeros(9, np.float32)), n, n)                      # zero F
    for bad in (np.nan, np.inf):                                        # non-finite F
        F = s["F"].copy()
        F[4] = bad
        empty_ok(run(F=F), n, n)
    empty_ok(run(F=pc.RANK1), n, n)                                     # rank 1
    empty_ok(run(mask=np.zeros(n, np.uint8)), n, 0)                     # a mask of zeros
    empty_ok(run(matches=s["matches"][:0], mask=np.zeros(0, np.uint8)), 0, 0)
    # masked records with NaN positions or indices outside the arrays are no fit records
    q = s["q_xy"].copy()
    q[:5] = np.nan
    m = s["matches"].copy()
    m["trainIdx"][5:9] = n + 7
    m["queryIdx"][9:11] = -1
    r = run(q_xy=q, matches=m)
    assert r["candidate"] == pc.reference(1)["candidate"] and r["fit"] == n - 11 == r["in_front"]
    assert not r["mask"][:11].any() and r["mask"][11:].all() and np.isnan(r["points"][:11]).all()
    q[:] = np.nan
    empty_ok(run(q_xy=q), n, 0)


@pytest.mark.parametrize("seed,sign", SCENES)
def test_unrelated_records_change_the_counts_but_not_the_winner(seed, sign):
    clean, noisy = pc.reference(seed, sign), pc.reference(seed, sign, pc.DRAWN, 60, True)
    k = int(clean["candidate"])
    assert int(noisy["candidate"]) == k and noisy["fit"] == pc.DRAWN + 60
    assert not np.array_equal(noisy["counts"], clean["counts"])
    assert noisy["counts"][k] >= pc.DRAWN and noisy["mask"][:pc.DRAWN].all()
    assert noisy["R"].tobytes() == clean["R"].tobytes() and noisy["t"].tobytes() == clean["t"].tobytes()


def test_thresholds_split_the_set():
    s = pc.scene(1)
    full = pc.reference(1)
    depth = np.sort(full["points"][:, 2].astype(np.float64))
    near = pc.reference(1, 1, pc.DRAWN, 0, False, float(depth[len(depth) // 2]))
    assert 0 < near["in_front"] < full["in_front"] and near["candidate"] == full["candidate"]
    far = pc.reference(1, 1, pc.DRAWN, 0, False, float("inf"))
    assert far["in_front"] == full["in_front"]
    tight = pc.reference(1, 1, pc.DRAWN, 0, False, 50.0, 0.999)
    assert 0 < tight["with_parallax"] < full["with_parallax"] and tight["in_front"] == full["in_front"]
    assert len(s["matches"]) == pc.DRAWN


def test_steps_are_exposed_and_consistent():
    from sift_amd import cv

    s, r = pc.scene(2), pc.reference(2)
    E = cv.essential_from_fundamental(s["F"], s["cam_q"], s["cam_t"])
    assert E.dtype == np.float64 and E.shape == (3, 3)
    ref = pc.kmat(s["cam_t"]).T @ s["F"].astype(np.float64).reshape(3, 3) @ pc.kmat(s["cam_q"])
    assert np.abs(E - ref).max() <= 1e-12 * np.abs(ref).max()
    cands = cv.decompose_essential(E)
    assert len(cands) == 4 and np.array_equal(cands[0][0], cands[2][0]) and np.array_equal(cands[0][1], -cands[2][1])
    R, t = cands[int(r["candidate"])]
    assert R.astype(np.float32).tobytes() == r["R"].tobytes() and t.astype(np.float32).tobytes() == r["t"].tobytes()
    assert cv.decompose_essential(np.outer([1.0, 2.0, 3.0], [3.0, 2.0, 1.0])) == []
    a, b, det, cosine = cv.triangulate_depths(R, t, np.array([[0.1, -0.2]]), np.array([[0.05, 0.1]]))
    assert a.shape == b.shape == det.shape == cosine.shape == (1,)
