"""Homography verification and projection on the GPU (sift_hip_verify_homography_*, sift_hip_score_homography_device,
sift_hip_project_homography_device; kernels in csrc/verify.hip).

The bar: what every hypothesis drew, solved and counted, the result record, the mask, the inlier list and its count
equal sift_amd.cv.ransac_homography, and projected positions sift_amd.cv.project_homography (the rule of
include/sift_hip.h in numpy float32), as raw bytes.  The inputs are tests/homography_cases.py;
tests/test_homography_cases.py checks the mirror itself on the CPU.
"""
import numpy as np
import pytest

import epipolar_cases as ec
import homography_cases as hc
import verify_cases as vc

pytestmark = pytest.mark.gpu
FILL = 0x5A  # the outputs start as this byte: what the device does not write stays visible


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


def verify(sift, matches, q_xy, t_xy, K, seed=0, count=None, cap=None, max_error=hc.MAX_ERROR, stride=(2, 2), v=None,
           nq=None, nt=None):
    """verify_homography_device on uploaded data; everything it writes, and the verifier's hypotheses, on the host."""
    cap = len(matches) if cap is None else cap
    v = v or sift.Verifier(max(cap, 1), K)
    dm = dev(sift, matches) if len(matches) else None
    dq, dt = dev(sift, ec.with_stride(q_xy, stride[0])), dev(sift, ec.with_stride(t_xy, stride[1]))
    dc = dev(sift, np.int32([count])) if count is not None else None
    res = dev(sift, np.full(52, FILL, np.uint8))
    out = dev(sift, np.full(16 * max(cap, 1), FILL, np.uint8))
    cnt = dev(sift, np.full(4, FILL, np.uint8))
    mask = dev(sift, np.full(max(cap, 1), FILL, np.uint8))
    v.verify_homography_device(dm.value if dm else 0, dc.value if dc else 0, cap, dq.value,
                               len(q_xy) if nq is None else nq, dt.value, len(t_xy) if nt is None else nt, res.value,
                               out.value, cnt.value, mask.value, max_error, K, seed, stride[0], stride[1])
    samples, H, valid, counts = v.homography_hypotheses()  # synchronises
    return dict(result=res.to_numpy(sift.HOMOGRAPHY_RESULT_DTYPE, (1,))[0],
                out=out.to_numpy(sift.DMATCH_DTYPE, (max(cap, 1),)), out_count=int(cnt.to_numpy(np.int32, (1,))[0]),
                mask=mask.to_numpy(np.uint8, (max(cap, 1),)), samples=samples, Hs=H, valid=valid, counts=counts)


def check_against(got, ref, cap, buf):
    """Every output of a verify call against cv.ransac_homography of the records that count."""
    n = ref["matches"]
    assert got["samples"].shape == ref["samples"].shape and np.array_equal(got["samples"], ref["samples"])
    assert np.array_equal(got["valid"], ref["valid"]), np.flatnonzero(got["valid"] != ref["valid"])[:8]
    bad = np.flatnonzero((got["Hs"].view(np.uint32) != ref["Hs"].view(np.uint32)).any(1))
    assert got["Hs"].dtype == ref["Hs"].dtype and len(bad) == 0, (bad[:8], got["Hs"][bad[:1]], ref["Hs"][bad[:1]])
    assert np.array_equal(got["counts"], ref["counts"]), np.flatnonzero(got["counts"] != ref["counts"])[:8]
    r = got["result"]
    assert r["H"].tobytes() == ref["H"].tobytes()
    assert (r["inliers"], r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
        (ref["inliers"], ref["hypothesis"], n, ref["valid_hypotheses"])
    assert got["out_count"] == ref["inliers"]
    assert got["out"][:ref["inliers"]].tobytes() == ref["list"].tobytes()
    assert got["out"][:ref["inliers"]].tobytes() == buf[:n][ref["mask"] != 0].tobytes()  # input records, input order
    assert (got["out"][ref["inliers"]:].view(np.uint8) == FILL).all()  # nothing behind the list is written
    assert np.array_equal(got["mask"][:n], ref["mask"]) and not got["mask"][n:cap].any()


@pytest.mark.parametrize("shape", hc.SHAPES, ids=lambda s: "%d+%d" % s[:2])
def test_shapes(sift, shape):
    n_in, n_out, K = shape
    m, q_xy, t_xy, planted = hc.case(n_in, n_out)
    ref = hc.reference(n_in, n_out, K)
    if shape == hc.CAPPED:  # the list at the head of a larger buffer, its length on the device
        buf, cap, count = hc.capped(), hc.CAP, len(m)
    else:
        buf, cap, count = m, len(m), None
    got = verify(sift, buf, q_xy, t_xy, K, count=count, cap=cap)
    print(shape, "winner", ref["hypothesis"], "inliers", ref["inliers"], "valid", ref["valid_hypotheses"])
    check_against(got, ref, cap, buf)
    if n_in + n_out < 4:
        assert got["result"]["hypothesis"] == -1 and got["out_count"] == 0 and not got["result"]["H"].any()
        assert (got["samples"] == -1).all() and not got["valid"].any()
    elif n_out:
        assert 0 < ref["valid_hypotheses"] < K  # the orientation test rejected some samples, on the device too


def test_more_matches_than_one_tile(sift):
    """2113 matches: past the score kernel's LDS tile (2048) and the select kernel's 1024-match chunks, one past a wave
    multiple."""
    n_in, n_out, K = hc.LARGE
    m, q_xy, t_xy, planted = hc.case(n_in, n_out)
    ref = hc.reference(n_in, n_out, K)
    got = verify(sift, m, q_xy, t_xy, K)
    check_against(got, ref, len(m), m)
    assert ref["hypothesis"] >= 0 and ref["inliers"] > 1024  # the list itself spans two chunks of the compaction


def test_two_runs_give_identical_bytes_and_seeds_differ(sift):
    n_in, n_out, K = hc.MAIN
    m, q_xy, t_xy, _ = hc.case(n_in, n_out)
    v = sift.Verifier(len(m), K)
    a = verify(sift, m, q_xy, t_xy, K, v=v)
    b = verify(sift, m, q_xy, t_xy, K, v=v)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes() if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    c = verify(sift, m, q_xy, t_xy, K, seed=1, v=v)
    assert c["result"]["hypothesis"] != a["result"]["hypothesis"]
    assert not np.array_equal(c["samples"], a["samples"])
    check_against(c, hc.reference(n_in, n_out, K, 1), len(m), m)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_recovery_on_the_device(sift, seed):
    """Asserted on the device's own result, not through the mirror: >= 95 % of the 120 planted pairs, at most 10 of
    the 80 outlier pairs."""
    n_in, n_out, K = hc.MAIN
    m, q_xy, t_xy, planted = hc.case(n_in, n_out)
    got = verify(sift, m, q_xy, t_xy, K, seed=seed)
    recall, false = hc.recovery(got["mask"][:len(m)], planted)
    print("seed", seed, "recall", recall, "false pairs", false, "valid", got["result"]["valid_hypotheses"])
    assert got["result"]["hypothesis"] >= 0 and got["result"]["inliers"] == got["out_count"]
    assert recall >= 0.95 and false <= 10


@pytest.mark.parametrize("strides", [(2, 2), (3, 3), (5, 2), (3, 5)])
def test_strides_give_identical_results(sift, strides):
    n_in, n_out, K = 24, 9, 256
    m, q_xy, t_xy, _ = hc.case(n_in, n_out)
    got = verify(sift, m, q_xy, t_xy, K, stride=strides)
    check_against(got, hc.reference(n_in, n_out, K), len(m), m)


def score(sift, matches, q_xy, t_xy, Hs, max_error, count=None, cap=None):
    cap = len(matches) if cap is None else cap
    Hs = np.ascontiguousarray(np.asarray(Hs, np.float32).reshape(-1, 9))
    v = sift.Verifier(max(cap, 1), len(Hs))
    dm, dq, dt, dH = dev(sift, matches), dev(sift, q_xy), dev(sift, t_xy), dev(sift, Hs)
    dc = dev(sift, np.int32([count])) if count is not None else None
    out = dev(sift, np.full(len(Hs), -77, np.int32))
    v.score_homography_device(dm.value, dc.value if dc else 0, cap, dq.value, len(q_xy), dt.value, len(t_xy), dH.value,
                              len(Hs), max_error, out.value, 2, 2)
    return out.to_numpy(np.int32, (len(Hs),))


def test_score_on_hand_made_hypotheses(sift):
    from sift_amd import cv

    n_in, n_out, _ = hc.MAIN
    m, q_xy, t_xy, planted = hc.case(n_in, n_out)
    Ht = hc.homography().reshape(-1)
    Ht = (Ht / np.linalg.norm(Ht)).astype(np.float32)
    Hs = np.stack([Ht, -Ht, np.full(9, np.nan, np.float32), hc.reference(*hc.MAIN)["H"]])
    want = [int(cv.transfer_inliers(m, q_xy, t_xy, h, hc.MAX_ERROR).sum()) for h in Hs]
    got = score(sift, m, q_xy, t_xy, Hs, hc.MAX_ERROR)
    assert got.tolist() == want
    assert want[0] == n_in and want[1] == 0 and want[2] == 0 and want[3] == hc.reference(*hc.MAIN)["inliers"]
    # a count on the device clamps the list
    head = score(sift, m, q_xy, t_xy, Hs[:1], hc.MAX_ERROR, count=50)
    assert head.tolist() == [int(cv.transfer_inliers(m[:50], q_xy, t_xy, Ht, hc.MAX_ERROR).sum())]
    # the hand-written case: q = (7, 2), max_error 2; (9, 2) sits on the edge, dx dx == e2 w w == 4, and counts
    hm = np.zeros(3, sift.DMATCH_DTYPE)
    hm["trainIdx"] = [0, 1, 2]
    hq, ht = np.float32([[7, 2]]), np.float32([[9, 2], [9.25, 2], [7, 4]])
    eye = np.eye(3, dtype=np.float32).reshape(-1)
    assert score(sift, hm, hq, ht, [eye, 2 * eye, -eye], 2.0).tolist() == [2, 2, 0]
    assert score(sift, hm[:1], hq, ht, [eye], 2.0).tolist() == [1]
    assert score(sift, hm[1:2], hq, ht, [eye], 2.0).tolist() == [0]
    assert score(sift, hm[2:], hq, ht, [eye], 2.0).tolist() == [1]


def test_bad_records_and_nan_positions_are_inliers_of_nothing(sift):
    from sift_amd import cv

    n_in, n_out, K = hc.MAIN
    m, q_xy, t_xy, _ = hc.case(n_in, n_out)
    bad = m.copy()
    rows = np.arange(0, len(m), 7)
    bad["queryIdx"][rows[0::3]] = -1
    bad["queryIdx"][rows[1::3]] = len(q_xy)
    bad["trainIdx"][rows[2::3]] = 2 ** 30
    ref = cv.ransac_homography(bad, q_xy, t_xy, hc.MAX_ERROR, K, 0)
    got = verify(sift, bad, q_xy, t_xy, K)
    check_against(got, ref, len(bad), bad)
    assert not got["mask"][rows].any() and ref["hypothesis"] >= 0
    assert not got["valid"][np.isin(got["samples"], rows).any(1)].any()  # a hypothesis that samples one is invalid
    # the position arrays' declared lengths are the bound, not their allocations
    short = cv.ransac_homography(m, q_xy[:150], t_xy, hc.MAX_ERROR, K, 0)
    got = verify(sift, m, q_xy, t_xy, K, nq=150)
    check_against(got, short, len(m), m)
    assert not got["mask"][m["queryIdx"] >= 150].any()
    # NaN positions behave the same
    qn, tn = q_xy.copy(), t_xy.copy()
    qn[m["queryIdx"][rows[0::2]], 0] = np.nan
    tn[m["trainIdx"][rows[1::2]], 1] = np.nan
    ref = cv.ransac_homography(m, qn, tn, hc.MAX_ERROR, K, 0)
    got = verify(sift, m, qn, tn, K)
    check_against(got, ref, len(m), m)
    assert not got["mask"][rows].any() and ref["hypothesis"] >= 0
    assert not got["valid"][np.isin(got["samples"], rows).any(1)].any()


def test_count_clamps_and_short_lists_are_empty_results(sift):
    from sift_amd import cv

    n_in, n_out, K = 24, 9, 256
    m, q_xy, t_xy, _ = hc.case(n_in, n_out)
    ref = hc.reference(n_in, n_out, K)
    check_against(verify(sift, m, q_xy, t_xy, K, count=10 ** 6), ref, len(m), m)  # *count > cap clamps to cap
    check_against(verify(sift, m, q_xy, t_xy, K, count=None), ref, len(m), m)  # count = null uses cap
    for count in (3, 0, -3):  # n < 4 and n = 0: the empty result, status 0
        n = max(count, 0)
        got = verify(sift, m, q_xy, t_xy, K, count=count)
        check_against(got, cv.ransac_homography(m[:n], q_xy, t_xy, hc.MAX_ERROR, K, 0), len(m), m)
        r = got["result"]
        assert (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, n, 0)
        assert not r["H"].any() and got["out_count"] == 0 and not got["mask"][:len(m)].any()
    # cap == 0 with null pointers
    v = sift.Verifier(16, 64)
    res, cnt = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    v.verify_homography_device(0, 0, 0, 0, 0, 0, 0, res.value, 0, cnt.value, 0, hypotheses=64)
    r = res.to_numpy(sift.HOMOGRAPHY_RESULT_DTYPE, (1,))[0]
    assert (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, 0, 0) and not r["H"].any()
    assert int(cnt.to_numpy(np.int32, (1,))[0]) == 0
    H, inl, hyp = v.verify_homography_host(0, 0, 0, 0, 0, 0, 0, hypotheses=64)
    assert H.shape == (3, 3) and not H.any() and len(inl) == 0 and hyp == -1


def test_limits_of_a_real_verifier_and_the_host_forms(sift):
    n_in, n_out, K = 24, 9, 256
    m, q_xy, t_xy, _ = hc.case(n_in, n_out)
    ref = hc.reference(n_in, n_out, K)
    v = sift.Verifier(len(m), K)
    dm, dq, dt = dev(sift, m), dev(sift, ec.with_stride(q_xy, 3)), dev(sift, ec.with_stride(t_xy, 3))
    res = dev(sift, np.zeros(52, np.uint8))
    args = (dq.value, len(q_xy), dt.value, len(t_xy))
    with pytest.raises(sift.SiftHipError, match="max_matches"):
        v.verify_homography_device(dm.value, 0, len(m) + 1, *args, res.value, hypotheses=K)
    with pytest.raises(sift.SiftHipError, match="hypotheses"):
        v.verify_homography_device(dm.value, 0, len(m), *args, res.value, hypotheses=K + 1)
    with pytest.raises(sift.SiftHipError, match="alias"):
        v.verify_homography_device(dm.value, 0, len(m), *args, res.value, out_ptr=dm.value + 16, hypotheses=K)
    H, inl, hyp = v.verify_homography_host(dm.value, 0, len(m), *args, hypotheses=K)
    assert H.dtype == np.float32 and H.tobytes() == ref["H"].tobytes() and hyp == ref["hypothesis"]
    assert inl.tobytes() == ref["list"].tobytes()
    rec, inl2, mask = v.verify_homography_host(dm.value, 0, len(m), *args, hypotheses=K, full=True)
    assert rec["valid_hypotheses"] == ref["valid_hypotheses"] and np.array_equal(mask, ref["mask"])
    assert inl2.tobytes() == inl.tobytes()
    # the one-shot function uploads the list itself
    H2, inl3, hyp2 = sift.verifyHomography(m, dq.value, dt.value, len(q_xy), len(t_xy), hypotheses=K)
    assert H2.tobytes() == H.tobytes() and inl3.tobytes() == inl.tobytes() and hyp2 == hyp


def test_each_getter_belongs_to_its_model_and_the_fundamental_path_is_unchanged(sift):
    n_in, n_out, K = vc.MAIN
    fm, fq, ft, _ = vc.case(n_in, n_out)
    hm, hq, ht, _ = hc.case(*hc.MAIN[:2])
    v = sift.Verifier(max(len(fm), len(hm)), K)
    for getter in (v.hypotheses, v.homography_hypotheses):  # no verify call has run
        with pytest.raises(sift.SiftHipError):
            getter()
    got = verify(sift, hm, hq, ht, K, v=v)
    check_against(got, hc.reference(*hc.MAIN), len(hm), hm)
    with pytest.raises(sift.SiftHipError, match="other model"):
        v.hypotheses()
    # a fundamental call after a homography call on the same verifier: the parent's bytes
    dm, dq, dt = dev(sift, fm), dev(sift, fq), dev(sift, ft)
    res = dev(sift, np.full(52, FILL, np.uint8))
    out, cnt = dev(sift, np.full(16 * len(fm), FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    mask = dev(sift, np.full(len(fm), FILL, np.uint8))
    v.verify_device(dm.value, 0, len(fm), dq.value, len(fq), dt.value, len(ft), res.value, out.value, cnt.value,
                    mask.value, vc.MAX_ERROR, K, 0, 2, 2)
    samples, F, valid, counts = v.hypotheses()
    ref = vc.reference(n_in, n_out, K)
    assert np.array_equal(samples, ref["samples"]) and F.tobytes() == ref["Fs"].tobytes()
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(valid, ref["valid"])
    r = res.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0]
    assert r["F"].tobytes() == ref["F"].tobytes() and r["hypothesis"] == ref["hypothesis"]
    assert (r["inliers"], r["matches"], r["valid_hypotheses"]) == (ref["inliers"], len(fm), ref["valid_hypotheses"])
    n = int(cnt.to_numpy(np.int32, (1,))[0])
    assert n == ref["inliers"] and out.to_numpy(sift.DMATCH_DTYPE, (len(fm),))[:n].tobytes() == ref["list"].tobytes()
    assert np.array_equal(mask.to_numpy(np.uint8, (len(fm),)), ref["mask"])
    with pytest.raises(sift.SiftHipError, match="other model"):
        v.homography_hypotheses()


PROJECT_H = np.float32([0.6, -0.02, 3.0, 0.03, 0.55, -2.0, 1 / 2048, -1 / 256, 0.5])  # w = 0 along y = 128 + x / 8


def project_input(n, stride, seed=3):
    """n rows of `stride` floats: positions on the 0.25 grid of the square (rows on both sides of PROJECT_H's w = 0
    line, some on it), every further column a marker value."""
    rng = np.random.default_rng(seed + n)
    xy = np.full((n, stride), 777.0, np.float32)
    xy[:, :2] = rng.integers(0, int(4 * ec.SIDE), (n, 2)) * 0.25
    if n > 2:
        xy[1, :2] = (0.0, 128.0)  # w == 0 exactly
        xy[2, :2] = (np.nan, 10.0)
    return xy


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("strides", [(3, 2), (2, 2), (3, 3)], ids=lambda s: "%dto%d" % s)
def test_projection_equals_the_mirror(sift, n, strides):
    """(3 -> 2) apart, (2 -> 2) in place, (3 -> 3) apart: the output's x, y equal cv.project_homography byte for byte,
    rows with w <= 0 (or NaN) are NaN, and nothing else is written -- the columns beyond y keep the fill (apart) or the
    input's marker (in place), as does the row behind the last."""
    from sift_amd import cv

    stride, out_stride = strides
    in_place = stride == out_stride == 2
    xy = project_input(n, stride)
    want = cv.project_homography(PROJECT_H, xy)
    dH, dxy = dev(sift, PROJECT_H), dev(sift, np.r_[xy, np.full((1, stride), 555.0, np.float32)])
    dout = dxy if in_place else dev(sift, np.full(4 * out_stride * (n + 1), FILL, np.uint8))
    sift.project_homography_device(dH.value, dxy.value, n, dout.value, stride, out_stride)
    sift.lib().sift_hip_device_sync()
    got = dout.to_numpy(np.float32, (n + 1, out_stride))
    assert got[:n, :2].tobytes() == want.tobytes()
    if n > 2:
        w = (PROJECT_H[6] * xy[:, 0] + PROJECT_H[7] * xy[:, 1]) + PROJECT_H[8]
        assert np.isnan(got[:n, :2][~(w > 0)]).all() and np.isnan(got[1, :2]).all() and np.isnan(got[2, :2]).all()
        assert (~(w > 0)).sum() > n // 8 and np.isfinite(got[:n, :2][w > 0]).all()
    behind = np.full(out_stride, 555.0, np.float32) if in_place else np.full(4 * out_stride, FILL, np.uint8).view(np.float32)
    assert got[n].tobytes() == behind.tobytes()  # the row behind the last is untouched
    if out_stride > 2:
        assert (got[:n, 2:].view(np.uint8) == FILL).all()  # columns beyond y are untouched
    if not in_place:
        assert dxy.to_numpy(np.float32, (n + 1, stride))[:n].tobytes() == xy.tobytes()  # the input is only read


def test_projection_in_place_keeps_further_columns_and_a_zero_h_projects_nothing(sift):
    from sift_amd import cv

    xy = project_input(300, 3)
    dH, dxy = dev(sift, PROJECT_H), dev(sift, xy)
    sift.project_homography_device(dH.value, dxy.value, 300, dxy.value, 3, 3)  # in place with stride 3
    sift.lib().sift_hip_device_sync()
    got = dxy.to_numpy(np.float32, (300, 3))
    assert got[:, :2].tobytes() == cv.project_homography(PROJECT_H, xy).tobytes() and (got[:, 2] == 777.0).all()
    dZ, out = dev(sift, np.zeros(13, np.float32)), dev(sift, np.zeros((300, 2), np.float32))  # the empty result record
    dxy2 = dev(sift, xy)
    sift.project_homography_device(dZ.value, dxy2.value, 300, out.value)
    sift.lib().sift_hip_device_sync()
    assert np.isnan(out.to_numpy(np.float32, (300, 2))).all()
    with pytest.raises(sift.SiftHipError, match="overlap"):
        sift.project_homography_device(dH.value, dxy.value, 300, dxy.value + 4, 3, 3)


def test_chain_on_one_stream(sift):
    """match_list_device -> verify_homography_device (its count taken from the list's device counter) ->
    project_homography_device (H = the result record's device address) -> match_list_guided_device on the projected
    positions, on one stream with no host synchronisation and no read-back between the calls.  Every stage equals the
    same step through the numpy mirrors."""
    import torch

    from sift_amd import cv

    q, t, q_xy, t_xy, planted = hc.chain_case(65, 64)
    nq, nt, K, radius = len(q), len(t), 256, 2.0
    up = lambda rows: dev(sift, rows.astype(np.float16).view(np.uint16))  # noqa: E731
    dq, dt, dqxy, dtxy = up(q), up(t), dev(sift, ec.with_stride(q_xy, 3)), dev(sift, ec.with_stride(t_xy, 3))
    m, v = sift.Matcher(max(nq, nt), max(nq, nt), max_pairs=2), sift.Verifier(nq, K)
    lst, cnt = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    res = dev(sift, np.full(52, FILL, np.uint8))
    inl, icnt = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    proj = dev(sift, np.full(8 * nq, FILL, np.uint8))
    out2, cnt2 = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    warm, wcnt = dev(sift, np.zeros(16 * nq, np.uint8)), dev(sift, np.zeros(4, np.uint8))
    # the matcher's first list calls allocate: both kinds once, outside the chain
    m.match_list_device(dq.value, nq, dt.value, nt, warm.value, wcnt.value)
    m.match_list_guided_device(dq.value, nq, dt.value, nt, dqxy.value, dtxy.value, radius, warm.value, wcnt.value, 3, 3)
    sift.lib().sift_hip_device_sync()
    s = torch.cuda.Stream()
    m.match_list_device(dq.value, nq, dt.value, nt, lst.value, cnt.value, stream=s.cuda_stream)
    v.verify_homography_device(lst.value, cnt.value, nq, dqxy.value, nq, dtxy.value, nt, res.value, inl.value, icnt.value,
                               0, hc.MAX_ERROR, K, 0, 3, 3, stream=s.cuda_stream)
    sift.project_homography_device(res.value, dqxy.value, nq, proj.value, 3, 2, stream=s.cuda_stream)
    m.match_list_guided_device(dq.value, nq, dt.value, nt, proj.value, dtxy.value, radius, out2.value, cnt2.value, 2, 3,
                               stream=s.cuda_stream)
    s.synchronize()
    # the mirrors
    every = np.ones((nq, nt), bool)
    fwd, rev = cv.mask_top2(q, t, every), cv.mask_top2(t, q, every.T)
    putative = cv.filter_matches(fwd[0], fwd[1], rev[0], rev[1])
    ref = cv.ransac_homography(putative, q_xy, t_xy, hc.MAX_ERROR, K, 0)
    assert ref["hypothesis"] >= 0 and len(putative) >= 16 and ref["inliers"] >= 16
    n1 = int(cnt.to_numpy(np.int32, (1,))[0])
    assert lst.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n1].tobytes() == putative.tobytes()
    r = res.to_numpy(sift.HOMOGRAPHY_RESULT_DTYPE, (1,))[0]
    assert r["H"].tobytes() == ref["H"].tobytes() and r["hypothesis"] == ref["hypothesis"] and r["matches"] == n1
    n2 = int(icnt.to_numpy(np.int32, (1,))[0])
    assert inl.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n2].tobytes() == ref["list"].tobytes()
    want_proj = cv.project_homography(ref["H"], q_xy)
    assert proj.to_numpy(np.float32, (nq, 2)).tobytes() == want_proj.tobytes()
    gf = cv.guided_top2(q, t, want_proj, t_xy, radius)
    gr = cv.guided_top2(t, q, t_xy, want_proj, radius)
    guided = cv.filter_matches(gf[0], gf[1], gr[0], gr[1])
    n3 = int(cnt2.to_numpy(np.int32, (1,))[0])
    assert out2.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n3].tobytes() == guided.tobytes()
    # every planted pair comes back: its query, carried over by H, lies inside its train row's window
    assert set(map(tuple, planted.tolist())) <= {(a, b) for a, b in zip(guided["queryIdx"], guided["trainIdx"])}
