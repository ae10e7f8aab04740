"""The verifier family on the GPU (csrc/verify.hip, refit.hip, pose.hip) on the scenes and value-edge lists of
tests/geometry_bank.py: frame-sized coordinates, hard motions, huge, tiny, non-finite and degenerate positions.

The bar is that of tests/test_gpu_verify.py, test_gpu_homography.py, test_gpu_refit.py, test_gpu_pose.py and
test_gpu_verify_batched.py, whose helpers run and compare here: every output equals the numpy mirror (sift_amd.cv) as
raw bytes, outputs start as 0x5A so that what is not written shows.  tests/test_geometry_bank.py holds the mirror itself
to float64 truth on the same inputs.  Per scene or list: verify (samples, models, valid, counts, result, mask, out,
out_count), the score of the float64 route's models rounded to float32, refine with 1 and 3 rounds, the pose from the
refined record (F) or the projection of the query positions through the refined H; then one batched verify call per
model over all of the model's scenes and lists, pair p against the rule and the single call with seed + p.
"""
import numpy as np
import pytest

import epipolar_cases as ec
import geometry_bank as gb
import test_gpu_homography as th
import test_gpu_pose as tp
import test_gpu_refit as tr
import test_gpu_verify as tv
import test_gpu_verify_batched as tb

pytestmark = pytest.mark.gpu
FILL = tv.FILL

NAMES = {m: gb.SCENES[m] + gb.EDGES for m in gb.MODELS}
CASES = [(m, n) for m in gb.MODELS for n in NAMES[m]]
IDS = ["%s-%s" % c for c in CASES]
SCORED = {"fundamental": "c2_1920", "homography": "perspective"}  # a value-edge list has no route: these scenes' models


def inputs(model, name):
    s = gb.source(model, name)
    return s["matches"], s["q_xy"], s["t_xy"]


def route_models(model, name):
    """The float64 route's K models rounded to float32 (unit norm, finite)."""
    M = gb.ransac64(model, SCORED[model] if name in gb.EDGES else name)["models"].astype(np.float32)
    assert np.isfinite(M).all() and M.shape == (gb.K, 9)
    return M


@pytest.mark.parametrize("model,name", CASES, ids=IDS)
def test_verify_equals_the_mirror(sift, model, name):
    m, q_xy, t_xy = inputs(model, name)
    ref = gb.verified(model, name)
    mod = tv if model == "fundamental" else th
    got = mod.verify(sift, m, q_xy, t_xy, gb.K, seed=gb.SEED, max_error=gb.MAX_ERROR)
    print(model, name, "winner", ref["hypothesis"], "inliers", ref["inliers"], "valid", ref["valid_hypotheses"])
    mod.check_against(got, ref, len(m), m)
    invalid = ~got["valid"].astype(bool)
    models = got[gb.FIELD[model] + "s"].view(np.uint32)
    assert not models[invalid].any() and not got["counts"][invalid].any()  # an invalid hypothesis is zeros, bit for bit
    assert (got["result"]["hypothesis"] == -1) == (got["result"]["valid_hypotheses"] == 0)


@pytest.mark.parametrize("model,name", CASES, ids=IDS)
def test_score_of_the_float64_models_equals_the_mirror(sift, model, name):
    from sift_amd import cv

    m, q_xy, t_xy = inputs(model, name)
    M = route_models(model, name)
    predicate = cv._sampson_pass if model == "fundamental" else cv._transfer_pass
    with np.errstate(all="ignore"):
        want = predicate(cv._match_points(m, q_xy, t_xy), M, gb.MAX_ERROR).sum(1).astype(np.int32)
    got = (tv if model == "fundamental" else th).score(sift, m, q_xy, t_xy, M, gb.MAX_ERROR)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    if name not in gb.EDGES:
        assert want.max() >= gb.N_IN // 2  # the route's winner is among them: the counts are no zeros


@pytest.mark.parametrize("rounds", (1, gb.ROUNDS))
@pytest.mark.parametrize("model,name", CASES, ids=IDS)
def test_refine_equals_the_mirror(sift, model, name, rounds):
    m, q_xy, t_xy = inputs(model, name)
    ref = gb.refined(model, name, rounds)
    got = tr.refine(sift, model, m, q_xy, t_xy, gb.verified(model, name), rounds, max_error=gb.MAX_ERROR)
    print(model, name, "rounds", rounds, "inliers", gb.verified(model, name)["inliers"], "->", ref["inliers"], "accepted",
          ref["accepted"])
    tr.check(sift, model, got, ref, m, len(m))


@pytest.mark.parametrize("name", NAMES["fundamental"])
def test_pose_from_the_refined_record_equals_the_mirror(sift, name):
    s = gb.source("fundamental", name)
    r, ref = gb.refined("fundamental", name), gb.posed(name)
    cam_q, cam_t = (s["cam_q"], s["cam_t"]) if "cam_q" in s else gb.EDGE_CAMS
    scene = dict(matches=s["matches"], q_xy=s["q_xy"], t_xy=s["t_xy"], mask=r["mask"], cam_q=cam_q, cam_t=cam_t,
                 result={"F": r["F"], "hypothesis": r["hypothesis"]})
    got = tp.pose(sift, scene)
    print(name, "fit", ref["fit"], "counts", ref["counts"], "candidate", ref["candidate"], "parallax", ref["with_parallax"])
    tp.check(got, ref, s["matches"], len(s["matches"]))
    tp.the_inputs_stay(sift, got, scene)
    if name in gb.FUNDAMENTAL and name not in gb.ILL_POSED:
        assert ref["candidate"] >= 0 and ref["in_front"] >= gb.N_IN - 2


@pytest.mark.parametrize("name", NAMES["homography"])
def test_projection_through_the_refined_h_equals_the_mirror(sift, name):
    from sift_amd import cv

    s = gb.source("homography", name)
    H = gb.refined("homography", name)["H"]
    xy = s["q_xy"]
    with np.errstate(all="ignore"):
        want = cv.project_homography(H, xy)
    dH, dxy = tv.dev(sift, H), tv.dev(sift, xy)
    out = tv.dev(sift, np.full(8 * (len(xy) + 1), FILL, np.uint8))
    sift.project_homography_device(dH.value, dxy.value, len(xy), out.value, 2, 2)
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    got = out.to_numpy(np.float32, (len(xy) + 1, 2))
    assert got[:len(xy)].tobytes() == want.tobytes()
    assert (got[len(xy)].view(np.uint8) == FILL).all()  # the row behind the last is untouched
    if name in gb.HOMOGRAPHY:
        planted = s["q_xy"][s["matches"]["queryIdx"][s["planted"]]]
        assert np.isfinite(cv.project_homography(H, planted)).all()  # in front, every one


class BankBatch:
    """Every scene and list of a model as the pairs of one batch, as tests/test_gpu_verify_batched.Inputs lays one out."""

    def __init__(self, sift, model, stride=(2, 2)):
        self.sift, self.model, self.stride, self.K, self.seed = sift, model, stride, gb.K, gb.SEED
        self.names = NAMES[model]
        self.host = [dict(zip(("buf", "q_xy", "t_xy"), inputs(model, n))) for n in self.names]
        self.caps = [len(p["buf"]) for p in self.host]
        self.row0 = np.concatenate([[0], np.cumsum(self.caps)]).astype(int)
        self.P, self.rows = len(self.host), int(self.row0[-1])
        self.dm = tv.dev(sift, np.concatenate([p["buf"] for p in self.host]))
        self.dc = tv.dev(sift, np.int32(self.caps))
        self.dxy = [(tv.dev(sift, ec.with_stride(p["q_xy"], stride[0])), tv.dev(sift, ec.with_stride(p["t_xy"], stride[1])))
                    for p in self.host]
        self.pairs = [(d[0].value, len(p["q_xy"]), d[1].value, len(p["t_xy"]), cap)
                      for p, d, cap in zip(self.host, self.dxy, self.caps)]


@pytest.mark.parametrize("model", gb.MODELS)
def test_one_batch_of_every_scene_equals_the_rule_and_the_single_calls(sift, model):
    inp = BankBatch(sift, model)
    v = sift.Verifier(inp.rows, gb.K, inp.P)
    got = tb.run(inp, v)
    f = gb.FIELD[model]
    for p, name in enumerate(inp.names):
        ref = gb.verified(model, name, gb.SEED + p)
        r, a, cap = got["results"][p], int(inp.row0[p]), inp.caps[p]
        assert r[f].tobytes() == ref[f].tobytes(), (p, name)
        assert (r["inliers"], r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
            (ref["inliers"], ref["hypothesis"], cap, ref["valid_hypotheses"]), (p, name)
        rows = got["out"][a:a + cap]
        assert got["out_counts"][p] == ref["inliers"] and rows[:ref["inliers"]].tobytes() == ref["list"].tobytes(), (p, name)
        assert (rows[ref["inliers"]:].view(np.uint8) == FILL).all(), (p, name)
        assert np.array_equal(got["mask"][a:a + cap], ref["mask"]), (p, name)
    assert (got["results"][inp.P:].view(np.uint8) == FILL).all() and (got["out_counts"][inp.P:].view(np.uint8) == FILL).all()
    assert (got["out"][inp.rows:].view(np.uint8) == FILL).all() and (got["mask"][inp.rows:] == FILL).all()
    assert tb.same_bytes(got, tb.singles(inp, v))
    winners = [gb.verified(model, n, gb.SEED + p)["hypothesis"] for p, n in enumerate(inp.names)]
    assert winners[1:len(gb.SCENES[model])] != [gb.verified(model, n)["hypothesis"] for n in gb.SCENES[model][1:]]  # p shows
