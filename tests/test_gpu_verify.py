"""Two-view verification on the GPU (sift_hip_verify_*, sift_hip_score_*; kernels in csrc/verify.hip).

The bar: what every hypothesis drew, solved and counted, the result record, the mask, the inlier list and its count
equal sift_amd.cv.ransac_fundamental (the rule of include/sift_hip.h in numpy float32) as raw bytes.  The inputs are
tests/verify_cases.py; tests/test_verify_cases.py checks the mirror itself on the CPU.
"""
import numpy as np
import pytest

import epipolar_cases as ec
import verify_cases as vc

pytestmark = pytest.mark.gpu
FILL = 0x5A  # the outputs start as this byte: what the device does not write stays visible


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


def verify(sift, matches, q_xy, t_xy, K, seed=0, count=None, cap=None, max_error=vc.MAX_ERROR, stride=(2, 2), v=None,
           nq=None, nt=None):
    """verify_device on uploaded data; everything it writes, and the verifier's hypotheses, back on the host."""
    cap = len(matches) if cap is None else cap
    v = v or sift.Verifier(max(cap, 1), K)
    dm = dev(sift, matches) if len(matches) else None
    dq, dt = dev(sift, ec.with_stride(q_xy, stride[0])), dev(sift, ec.with_stride(t_xy, stride[1]))
    dc = dev(sift, np.int32([count])) if count is not None else None
    res = dev(sift, np.full(52, FILL, np.uint8))
    out = dev(sift, np.full(16 * max(cap, 1), FILL, np.uint8))
    cnt = dev(sift, np.full(4, FILL, np.uint8))
    mask = dev(sift, np.full(max(cap, 1), FILL, np.uint8))
    v.verify_device(dm.value if dm else 0, dc.value if dc else 0, cap, dq.value, len(q_xy) if nq is None else nq,
                    dt.value, len(t_xy) if nt is None else nt, res.value, out.value, cnt.value, mask.value, max_error, K,
                    seed, stride[0], stride[1])
    samples, F, valid, counts = v.hypotheses()  # synchronises
    return dict(result=res.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0], out=out.to_numpy(sift.DMATCH_DTYPE, (max(cap, 1),)),
                out_count=int(cnt.to_numpy(np.int32, (1,))[0]), mask=mask.to_numpy(np.uint8, (max(cap, 1),)),
                samples=samples, Fs=F, valid=valid, counts=counts)


def check_against(got, ref, cap, buf):
    """Every output of a verify call against cv.ransac_fundamental of the records that count."""
    n = ref["matches"]
    assert np.array_equal(got["samples"], ref["samples"])
    assert np.array_equal(got["valid"], ref["valid"]), np.flatnonzero(got["valid"] != ref["valid"])[:8]
    bad = np.flatnonzero((got["Fs"].view(np.uint32) != ref["Fs"].view(np.uint32)).any(1))
    assert got["Fs"].dtype == ref["Fs"].dtype and len(bad) == 0, (bad[:8], got["Fs"][bad[:1]], ref["Fs"][bad[:1]])
    assert np.array_equal(got["counts"], ref["counts"]), np.flatnonzero(got["counts"] != ref["counts"])[:8]
    r = got["result"]
    assert r["F"].tobytes() == ref["F"].tobytes()
    assert (r["inliers"], r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
        (ref["inliers"], ref["hypothesis"], n, ref["valid_hypotheses"])
    assert got["out_count"] == ref["inliers"]
    assert got["out"][:ref["inliers"]].tobytes() == ref["list"].tobytes()
    assert got["out"][:ref["inliers"]].tobytes() == buf[:n][ref["mask"] != 0].tobytes()  # input records, input order
    assert (got["out"][ref["inliers"]:].view(np.uint8) == FILL).all()  # nothing behind the list is written
    assert np.array_equal(got["mask"][:n], ref["mask"]) and not got["mask"][n:cap].any()


@pytest.mark.parametrize("shape", vc.SHAPES, ids=lambda s: "%d+%d" % s[:2])
def test_shapes(sift, shape):
    n_in, n_out, K = shape
    m, q_xy, t_xy, planted = vc.case(n_in, n_out)
    ref = vc.reference(n_in, n_out, K)
    if shape == vc.CAPPED:  # the list at the head of a larger buffer, its length on the device
        buf, cap, count = vc.capped(), vc.CAP, len(m)
    else:
        buf, cap, count = m, len(m), None
    got = verify(sift, buf, q_xy, t_xy, K, count=count, cap=cap)
    print(shape, "winner", ref["hypothesis"], "inliers", ref["inliers"], "valid", ref["valid_hypotheses"])
    check_against(got, ref, cap, buf)
    if n_in + n_out < 8:
        assert got["result"]["hypothesis"] == -1 and got["out_count"] == 0 and not got["result"]["F"].any()
        assert (got["samples"] == -1).all() and not got["valid"].any()


def test_more_matches_than_one_tile(sift):
    """2113 matches: past the score kernel's LDS tile (2048) and the select kernel's 1024-match chunks, one past a wave
    multiple."""
    from sift_amd import cv

    m, q_xy, t_xy, planted = vc.case(1800, 313)
    ref = cv.ransac_fundamental(m, q_xy, t_xy, vc.MAX_ERROR, 64, 0)
    got = verify(sift, m, q_xy, t_xy, 64)
    check_against(got, ref, len(m), m)
    assert ref["hypothesis"] >= 0 and ref["inliers"] > 1024  # the list itself spans two chunks of the compaction


def test_two_runs_give_identical_bytes_and_seeds_differ(sift):
    n_in, n_out, K = vc.MAIN
    m, q_xy, t_xy, _ = vc.case(n_in, n_out)
    v = sift.Verifier(len(m), K)
    a = verify(sift, m, q_xy, t_xy, K, v=v)
    b = verify(sift, m, q_xy, t_xy, K, v=v)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes() if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    c = verify(sift, m, q_xy, t_xy, K, seed=1, v=v)
    assert c["result"]["hypothesis"] != a["result"]["hypothesis"]
    assert not np.array_equal(c["samples"], a["samples"])
    check_against(c, vc.reference(n_in, n_out, K, 1), len(m), m)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_recovery_on_the_device(sift, seed):
    """Asserted on the device's own result, not through the mirror: >= 95 % of the 120 planted pairs, at most 10 of
    the 80 outlier pairs."""
    n_in, n_out, K = vc.MAIN
    m, q_xy, t_xy, planted = vc.case(n_in, n_out)
    got = verify(sift, m, q_xy, t_xy, K, seed=seed)
    recall, false = vc.recovery(got["mask"][:len(m)], planted)
    print("seed", seed, "recall", recall, "false pairs", false)
    assert got["result"]["hypothesis"] >= 0 and got["result"]["inliers"] == got["out_count"]
    assert recall >= 0.95 and false <= 10


@pytest.mark.parametrize("strides", [(2, 2), (3, 3), (5, 2), (3, 5)])
def test_strides_give_identical_results(sift, strides):
    n_in, n_out, K = 24, 9, 256
    m, q_xy, t_xy, _ = vc.case(n_in, n_out)
    got = verify(sift, m, q_xy, t_xy, K, stride=strides)
    check_against(got, vc.reference(n_in, n_out, K), len(m), m)


def score(sift, matches, q_xy, t_xy, Fs, max_error, count=None, cap=None):
    cap = len(matches) if cap is None else cap
    Fs = np.ascontiguousarray(np.asarray(Fs, np.float32).reshape(-1, 9))
    v = sift.Verifier(max(cap, 1), len(Fs))
    dm, dq, dt, dF = dev(sift, matches), dev(sift, q_xy), dev(sift, t_xy), dev(sift, Fs)
    dc = dev(sift, np.int32([count])) if count is not None else None
    out = dev(sift, np.full(len(Fs), -77, np.int32))
    v.score_device(dm.value, dc.value if dc else 0, cap, dq.value, len(q_xy), dt.value, len(t_xy), dF.value, len(Fs),
                   max_error, out.value, 2, 2)
    return out.to_numpy(np.int32, (len(Fs),))


def test_score_on_hand_made_hypotheses(sift):
    from sift_amd import cv

    n_in, n_out, _ = vc.MAIN
    m, q_xy, t_xy, planted = vc.case(n_in, n_out)
    Ft = ec.fundamental().reshape(-1)
    Fs = np.stack([Ft, -Ft, np.full(9, np.nan, np.float32), vc.reference(*vc.MAIN)["F"]])
    want = [int(cv.sampson_inliers(m, q_xy, t_xy, f, vc.MAX_ERROR).sum()) for f in Fs]
    got = score(sift, m, q_xy, t_xy, Fs, vc.MAX_ERROR)
    assert got.tolist() == want and want[0] == want[1] >= n_in and want[2] == 0 and want[3] == vc.reference(*vc.MAIN)["inliers"]
    # a count on the device clamps the list
    head = score(sift, m, q_xy, t_xy, Fs[:1], vc.MAX_ERROR, count=50)
    assert head.tolist() == [int(cv.sampson_inliers(m[:50], q_xy, t_xy, Ft, vc.MAX_ERROR).sum())]
    # the hand-written case: (4, 1) sits on the edge, r r == e2 (nq + nr) == 9, and counts
    h = ec.HAND
    hm = np.zeros(3, sift.DMATCH_DTYPE)
    hm["trainIdx"] = [0, 1, 2]
    assert score(sift, hm, h["q_xy"], h["t_xy"], [h["F"], -h["F"]], h["max_error"]).tolist() == [2, 2]
    assert score(sift, hm[:1], h["q_xy"], h["t_xy"], [h["F"]], h["max_error"]).tolist() == [1]
    assert score(sift, hm[1:2], h["q_xy"], h["t_xy"], [h["F"]], h["max_error"]).tolist() == [0]


def test_bad_records_and_nan_positions_are_inliers_of_nothing(sift):
    from sift_amd import cv

    n_in, n_out, K = vc.MAIN
    m, q_xy, t_xy, _ = vc.case(n_in, n_out)
    bad = m.copy()
    rows = np.arange(0, len(m), 7)
    bad["queryIdx"][rows[0::3]] = -1
    bad["queryIdx"][rows[1::3]] = len(q_xy)
    bad["trainIdx"][rows[2::3]] = 2 ** 30
    ref = cv.ransac_fundamental(bad, q_xy, t_xy, vc.MAX_ERROR, K, 0)
    got = verify(sift, bad, q_xy, t_xy, K)
    check_against(got, ref, len(bad), bad)
    assert not got["mask"][rows].any() and ref["valid_hypotheses"] < K and ref["hypothesis"] >= 0
    assert not got["valid"][np.isin(got["samples"], rows).any(1)].any()  # a hypothesis that samples one is invalid
    # the position arrays' declared lengths are the bound, not their allocations
    short = cv.ransac_fundamental(m, q_xy[:150], t_xy, vc.MAX_ERROR, K, 0)
    got = verify(sift, m, q_xy, t_xy, K, nq=150)
    check_against(got, short, len(m), m)
    assert not got["mask"][m["queryIdx"] >= 150].any()
    # NaN positions behave the same
    qn, tn = q_xy.copy(), t_xy.copy()
    qn[m["queryIdx"][rows[0::2]], 0] = np.nan
    tn[m["trainIdx"][rows[1::2]], 1] = np.nan
    ref = cv.ransac_fundamental(m, qn, tn, vc.MAX_ERROR, K, 0)
    got = verify(sift, m, qn, tn, K)
    check_against(got, ref, len(m), m)
    assert not got["mask"][rows].any() and ref["hypothesis"] >= 0


def test_count_clamps_and_short_lists_are_empty_results(sift):
    n_in, n_out, K = 24, 9, 256
    m, q_xy, t_xy, _ = vc.case(n_in, n_out)
    ref = vc.reference(n_in, n_out, K)
    check_against(verify(sift, m, q_xy, t_xy, K, count=10 ** 6), ref, len(m), m)  # *count > cap clamps to cap
    check_against(verify(sift, m, q_xy, t_xy, K, count=None), ref, len(m), m)  # count = null uses cap
    from sift_amd import cv

    for count in (7, 0, -3):  # n < 8 and n = 0: the empty result, status 0
        n = max(count, 0)
        got = verify(sift, m, q_xy, t_xy, K, count=count)
        check_against(got, cv.ransac_fundamental(m[:n], q_xy, t_xy, vc.MAX_ERROR, K, 0), len(m), m)
        r = got["result"]
        assert (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, n, 0)
        assert not r["F"].any() and got["out_count"] == 0 and not got["mask"][:len(m)].any()
    # cap == 0 with null pointers
    v = sift.Verifier(16, 64)
    res, cnt = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    v.verify_device(0, 0, 0, 0, 0, 0, 0, res.value, 0, cnt.value, 0, hypotheses=64)
    r = res.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0]
    assert (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, 0, 0) and not r["F"].any()
    assert int(cnt.to_numpy(np.int32, (1,))[0]) == 0
    F, inl, hyp = v.verify_host(0, 0, 0, 0, 0, 0, 0, hypotheses=64)
    assert F.shape == (3, 3) and not F.any() and len(inl) == 0 and hyp == -1


def test_limits_of_a_real_verifier_and_the_host_forms(sift):
    n_in, n_out, K = 24, 9, 256
    m, q_xy, t_xy, _ = vc.case(n_in, n_out)
    ref = vc.reference(n_in, n_out, K)
    v = sift.Verifier(len(m), K)
    dm, dq, dt = dev(sift, m), dev(sift, ec.with_stride(q_xy, 3)), dev(sift, ec.with_stride(t_xy, 3))
    res = dev(sift, np.zeros(52, np.uint8))
    with pytest.raises(sift.SiftHipError, match="max_matches"):
        v.verify_device(dm.value, 0, len(m) + 1, dq.value, len(q_xy), dt.value, len(t_xy), res.value, hypotheses=K)
    with pytest.raises(sift.SiftHipError, match="hypotheses"):
        v.verify_device(dm.value, 0, len(m), dq.value, len(q_xy), dt.value, len(t_xy), res.value, hypotheses=K + 1)
    with pytest.raises(sift.SiftHipError, match="alias"):
        v.verify_device(dm.value, 0, len(m), dq.value, len(q_xy), dt.value, len(t_xy), res.value, out_ptr=dm.value + 16,
                        hypotheses=K)
    with pytest.raises(sift.SiftHipError):
        v.hypotheses()  # no verify call has run
    F, inl, hyp = v.verify_host(dm.value, 0, len(m), dq.value, len(q_xy), dt.value, len(t_xy), hypotheses=K)
    assert F.dtype == np.float32 and F.tobytes() == ref["F"].tobytes() and hyp == ref["hypothesis"]
    assert inl.tobytes() == ref["list"].tobytes()
    rec, inl2, mask = v.verify_host(dm.value, 0, len(m), dq.value, len(q_xy), dt.value, len(t_xy), hypotheses=K, full=True)
    assert rec["valid_hypotheses"] == ref["valid_hypotheses"] and np.array_equal(mask, ref["mask"])
    # the one-shot function uploads the list itself
    F2, inl3, hyp2 = sift.verifyFundamental(m, dq.value, dt.value, len(q_xy), len(t_xy), hypotheses=K)
    assert F2.tobytes() == F.tobytes() and inl3.tobytes() == inl.tobytes() and hyp2 == hyp


@pytest.mark.parametrize("model", ["fundamental", "homography"])
def test_host_form_leaves_the_rows_past_the_inliers_as_they_were(sift, model):
    """sift_hip_verify_*_host on the C ABI with the caller's out_host prefilled: the first `inliers` rows are the
    rule's list, every byte behind them is the caller's still (the Python host forms hand in a fresh array and return
    its head, so they cannot see this).  cap 12 with a device count of 9: the mask is cap bytes, zero from n on."""
    import ctypes

    from sift_amd import cv

    cap, count, K = 12, 9, 16
    m, q_xy, t_xy, _ = vc.case(9, 3)
    assert len(m) == cap
    rule, field, dtype = {"fundamental": (cv.ransac_fundamental, "F", sift.VERIFY_RESULT_DTYPE),
                          "homography": (cv.ransac_homography, "H", sift.HOMOGRAPHY_RESULT_DTYPE)}[model]
    ref = rule(m[:count], q_xy, t_xy, vc.MAX_ERROR, K, 0)
    n = int(ref["inliers"])
    assert 0 < n < count
    v = sift.Verifier(cap, K)
    dm, dq, dt, dc = dev(sift, m), dev(sift, q_xy), dev(sift, t_xy), dev(sift, np.int32([count]))
    rec, out, mask = np.zeros(1, dtype), np.full(16 * cap, FILL, np.uint8), np.full(cap, FILL, np.uint8)
    fn = getattr(sift.lib(), f"sift_hip_verify_{model}_host")
    p = sift._VerifyParams(K, 0, vc.MAX_ERROR)
    rc = fn(v._v, dm.value, dc.value, cap, dq.value, 2, len(q_xy), dt.value, 2, len(t_xy), ctypes.byref(p),
            ctypes.cast(rec.ctypes.data, fn.argtypes[11]), out.ctypes.data, mask.ctypes.data)
    assert rc == 0, sift.lib().sift_hip_last_error()
    assert rec[field][0].tobytes() == ref[field].tobytes()
    assert (rec["inliers"][0], rec["hypothesis"][0], rec["matches"][0]) == (n, ref["hypothesis"], count)
    assert out[:16 * n].tobytes() == ref["list"].tobytes()
    assert (out[16 * n:] == FILL).all()
    assert np.array_equal(mask[:count], ref["mask"]) and not mask[count:].any()


def test_chain_on_one_stream(sift):
    """match_list_device -> verify_device (its count taken from the list's device counter) on one stream with no host
    synchronisation in between; F is read back once and match_list_epipolar_device follows.  Equal to the same three
    steps through the numpy mirrors."""
    import torch

    from sift_amd import cv

    q, t, q_xy, t_xy, _, _, _, _ = ec.case(65, 64)
    nq, nt, K = len(q), len(t), 256
    up = lambda rows: dev(sift, rows.astype(np.float16).view(np.uint16))  # noqa: E731
    dq, dt, dqxy, dtxy = up(q), up(t), dev(sift, ec.with_stride(q_xy, 3)), dev(sift, ec.with_stride(t_xy, 3))
    m, v = sift.Matcher(max(nq, nt), max(nq, nt), max_pairs=2), sift.Verifier(nq, K)
    lst, cnt = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    res = dev(sift, np.full(52, FILL, np.uint8))
    inl, icnt = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    warm, wcnt = dev(sift, np.zeros(16 * nq, np.uint8)), dev(sift, np.zeros(4, np.uint8))
    m.match_list_device(dq.value, nq, dt.value, nt, warm.value, wcnt.value)  # the matcher's first list call allocates
    sift.lib().sift_hip_device_sync()
    s = torch.cuda.Stream()
    m.match_list_device(dq.value, nq, dt.value, nt, lst.value, cnt.value, stream=s.cuda_stream)
    v.verify_device(lst.value, cnt.value, nq, dqxy.value, nq, dtxy.value, nt, res.value, inl.value, icnt.value, 0,
                    vc.MAX_ERROR, K, 0, 3, 3, stream=s.cuda_stream)
    s.synchronize()
    r = res.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0]  # the one read-back
    out2, cnt2 = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    m.match_list_epipolar_device(dq.value, nq, dt.value, nt, dqxy.value, dtxy.value, r["F"], vc.MAX_ERROR, out2.value,
                                 cnt2.value, stream=s.cuda_stream)
    s.synchronize()
    # the mirrors
    every = np.ones((nq, nt), bool)
    fwd, rev = cv.mask_top2(q, t, every), cv.mask_top2(t, q, every.T)
    putative = cv.filter_matches(fwd[0], fwd[1], rev[0], rev[1])
    ref = cv.ransac_fundamental(putative, q_xy, t_xy, vc.MAX_ERROR, K, 0)
    assert ref["hypothesis"] >= 0 and len(putative) >= 8
    n1 = int(cnt.to_numpy(np.int32, (1,))[0])
    assert lst.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n1].tobytes() == putative.tobytes()
    assert r["F"].tobytes() == ref["F"].tobytes() and r["hypothesis"] == ref["hypothesis"] and r["matches"] == n1
    n2 = int(icnt.to_numpy(np.int32, (1,))[0])
    assert inl.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n2].tobytes() == ref["list"].tobytes()
    gf = cv.epipolar_top2(q, t, q_xy, t_xy, ref["F"], vc.MAX_ERROR)
    gr = cv.epipolar_top2(t, q, t_xy, q_xy, ref["F"].reshape(3, 3).T, vc.MAX_ERROR)
    guided = cv.filter_matches(gf[0], gf[1], gr[0], gr[1])
    n3 = int(cnt2.to_numpy(np.int32, (1,))[0])
    assert out2.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n3].tobytes() == guided.tobytes()
