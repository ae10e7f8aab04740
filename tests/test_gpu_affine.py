"""Affine and similarity verification on the GPU (sift_hip_verify_affine_*, sift_hip_score_affine_device,
sift_hip_refine_affine_*; k_verify_hypotheses_a and the AffinePass instantiations in csrc/verify.hip, k_refit_fit_a in
csrc/refit.hip), both models.

The bar: what every hypothesis drew, solved and counted, the result record, the mask, the inlier list and its count
equal sift_amd.cv.ransac_affine, and a refit equals sift_amd.cv.refine_affine (the rule of include/sift_hip.h in
numpy), as raw bytes, for single and batched calls.  The inputs are tests/affine_cases.py; tests/test_affine_cases.py
checks the mirror itself on the CPU.
"""
import numpy as np
import pytest

import affine_cases as ac
import epipolar_cases as ec
import homography_cases as hc
import verify_cases as vc

pytestmark = pytest.mark.gpu
MODELS = pytest.mark.parametrize("similarity", ac.MODELS, ids=ac.MODEL_IDS)
FILL = 0x5A  # the outputs start as this byte: what the device does not write stays visible


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


class Job:
    """A list and its positions on the device, with prefilled outputs: verify_affine_device and refine_affine_device
    on them, and everything they wrote on the host."""

    def __init__(self, sift, similarity, matches, q_xy, t_xy, K, count=None, cap=None, stride=(2, 2), v=None, nq=None,
                 nt=None):
        self.sift, self.similarity, self.K, self.stride = sift, similarity, K, stride
        self.cap = cap = len(matches) if cap is None else cap
        self.v = v or sift.Verifier(max(cap, 1), K)
        self.dm = dev(sift, matches) if len(matches) else None
        self.dq, self.dt = dev(sift, ec.with_stride(q_xy, stride[0])), dev(sift, ec.with_stride(t_xy, stride[1]))
        self.dc = dev(sift, np.int32([count])) if count is not None else None
        self.nq, self.nt = len(q_xy) if nq is None else nq, len(t_xy) if nt is None else nt
        self.res = dev(sift, np.full(52, FILL, np.uint8))
        self.mask = dev(sift, np.full(max(cap, 1), FILL, np.uint8))
        self.fresh()

    def fresh(self):
        s = self.sift
        self.out = dev(s, np.full(16 * max(self.cap, 1), FILL, np.uint8))
        self.cnt, self.acc = dev(s, np.full(4, FILL, np.uint8)), dev(s, np.full(4, FILL, np.uint8))

    def list_args(self):
        return (self.dm.value if self.dm else 0, self.dc.value if self.dc else 0, self.cap, self.dq.value, self.nq,
                self.dt.value, self.nt)

    def read(self):
        s, cap = self.sift, max(self.cap, 1)
        return dict(result=self.res.to_numpy(s.AFFINE_RESULT_DTYPE, (1,))[0], out=self.out.to_numpy(s.DMATCH_DTYPE, (cap,)),
                    out_count=int(self.cnt.to_numpy(np.int32, (1,))[0]), mask=self.mask.to_numpy(np.uint8, (cap,)),
                    accepted=int(self.acc.to_numpy(np.int32, (1,))[0]))

    def verify(self, seed=0, max_error=ac.MAX_ERROR):
        self.v.verify_affine_device(*self.list_args(), self.res.value, self.out.value, self.cnt.value, self.mask.value,
                                    max_error, self.K, seed, *self.stride, similarity=self.similarity)
        samples, A, valid, counts = self.v.affine_hypotheses(self.similarity)  # synchronises
        return dict(self.read(), samples=samples, Hs=A, valid=valid, counts=counts)

    def refine(self, rounds=1, max_error=ac.MAX_ERROR, state=None):
        """refine_affine_device on what verify left on the device, or on the given (record, mask)."""
        if state is not None:
            self.res = dev(self.sift, np.array([state[0]], self.sift.AFFINE_RESULT_DTYPE))
            self.mask = dev(self.sift, np.r_[np.asarray(state[1], np.uint8), np.full(max(self.cap, 1), FILL, np.uint8)][:max(self.cap, 1)])
        self.fresh()
        self.v.refine_affine_device(*self.list_args(), self.res.value, self.mask.value, self.out.value, self.cnt.value,
                                    self.acc.value, max_error, rounds, *self.stride, similarity=self.similarity)
        self.sift._check(self.sift.lib().sift_hip_device_sync(), "sync")
        return self.read()


def verify(sift, similarity, matches, q_xy, t_xy, K, seed=0, max_error=ac.MAX_ERROR, **kw):
    return Job(sift, similarity, matches, q_xy, t_xy, K, **kw).verify(seed, max_error)


def check_against(got, ref, cap, buf):
    """Every output of a verify call against cv.ransac_affine of the records that count."""
    n = ref["matches"]
    assert got["samples"].shape == ref["samples"].shape and np.array_equal(got["samples"], ref["samples"])
    assert np.array_equal(got["valid"], ref["valid"]), np.flatnonzero(got["valid"] != ref["valid"])[:8]
    bad = np.flatnonzero((got["Hs"].view(np.uint32) != ref["Hs"].view(np.uint32)).any(1))
    assert got["Hs"].dtype == ref["Hs"].dtype and len(bad) == 0, (bad[:8], got["Hs"][bad[:1]], ref["Hs"][bad[:1]])
    assert np.array_equal(got["counts"], ref["counts"]), np.flatnonzero(got["counts"] != ref["counts"])[:8]
    check_record(got, ref, cap, buf)


def check_record(got, ref, cap, buf):
    """The record, the mask, the list and its count of a verify or refine call against the mirror's dict."""
    n = ref["matches"]
    r = got["result"]
    assert r["H"].tobytes() == ref["H"].tobytes(), (r["H"], ref["H"])
    assert (r["inliers"], r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
        (ref["inliers"], ref["hypothesis"], n, ref["valid_hypotheses"])
    assert got["out_count"] == ref["inliers"]
    assert got["out"][:ref["inliers"]].tobytes() == ref["list"].tobytes()
    assert got["out"][:ref["inliers"]].tobytes() == buf[:n][ref["mask"] != 0].tobytes()  # input records, input order
    assert (got["out"][ref["inliers"]:].view(np.uint8) == FILL).all()  # nothing behind the list is written
    assert np.array_equal(got["mask"][:n], ref["mask"])


@MODELS
@pytest.mark.parametrize("shape", ac.SHAPES + [ac.LARGE], ids=lambda s: "%d+%d" % s[:2])
def test_shapes(sift, similarity, shape):
    n_in, n_out, K = shape
    m, q_xy, t_xy, planted = ac.case(n_in, n_out, similarity)
    ref = ac.reference(n_in, n_out, K, similarity)
    if shape == ac.CAPPED:  # the list at the head of a larger buffer, its length on the device
        buf, cap, count = ac.capped(similarity), ac.CAP, len(m)
    else:
        buf, cap, count = m, len(m), None
    got = verify(sift, similarity, buf, q_xy, t_xy, K, count=count, cap=cap)
    print(shape, "winner", ref["hypothesis"], "inliers", ref["inliers"], "valid", ref["valid_hypotheses"])
    check_against(got, ref, cap, buf)
    assert not got["mask"][len(m):cap].any()  # the capped list's tail is not counted: every cap byte is written, zero
    if n_in + n_out < ac.sample_size(similarity):
        assert got["result"]["hypothesis"] == -1 and got["out_count"] == 0 and not got["result"]["H"].any()
        assert (got["samples"] == -1).all() and not got["valid"].any()
    elif shape == ac.LARGE:
        assert ref["inliers"] > 1024  # the list itself spans two chunks of the compaction


@MODELS
def test_degenerate_list(sift, similarity):
    from sift_amd import cv

    m, q_xy, t_xy, planted, _ = ac.degenerate(similarity)
    ref = cv.ransac_affine(m, q_xy, t_xy, ac.MAX_ERROR, ac.DEGENERATE_K, 0, similarity)
    got = verify(sift, similarity, m, q_xy, t_xy, ac.DEGENERATE_K)
    check_against(got, ref, len(m), m)
    assert 0 < got["result"]["valid_hypotheses"] < ac.DEGENERATE_K  # some samples were degenerate, on the device too


@MODELS
def test_two_runs_give_identical_bytes_and_seeds_differ(sift, similarity):
    n_in, n_out, K = ac.MAIN
    m, q_xy, t_xy, _ = ac.case(n_in, n_out, similarity)
    job = Job(sift, similarity, m, q_xy, t_xy, K)
    a, b = job.verify(), job.verify()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes() if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    c = job.verify(seed=1)
    assert not np.array_equal(c["samples"], a["samples"]) and c["Hs"].tobytes() != a["Hs"].tobytes()
    assert c["result"].tobytes() != a["result"].tobytes()
    check_against(c, ac.reference(n_in, n_out, K, similarity, 1), len(m), m)


@MODELS
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_recovery_on_the_device(sift, similarity, seed):
    """Asserted on the device's own mask, not through the mirror: >= 95 % of the 120 planted pairs, at most 10 of
    the 80 unrelated pairs."""
    n_in, n_out, K = ac.MAIN
    m, q_xy, t_xy, planted = ac.case(n_in, n_out, similarity)
    got = verify(sift, similarity, m, q_xy, t_xy, K, seed=seed)
    recall, false = ac.recovery(got["mask"][:len(m)], planted)
    print("seed", seed, "recall", recall, "false pairs", false, "valid", got["result"]["valid_hypotheses"])
    assert got["result"]["hypothesis"] >= 0 and got["result"]["inliers"] == got["out_count"]
    assert recall >= 0.95 and false <= 10


@MODELS
@pytest.mark.parametrize("strides", [(2, 2), (3, 3), (5, 2), (3, 5)])
def test_strides_give_identical_results(sift, similarity, strides):
    n_in, n_out, K = 24, 9, 128
    m, q_xy, t_xy, _ = ac.case(n_in, n_out, similarity)
    got = verify(sift, similarity, m, q_xy, t_xy, K, stride=strides)
    check_against(got, ac.reference(n_in, n_out, K, similarity), len(m), m)


def score(sift, matches, q_xy, t_xy, As, max_error, count=None, homography=False):
    As = np.ascontiguousarray(np.asarray(As, np.float32).reshape(-1, 9))
    v = sift.Verifier(max(len(matches), 1), len(As))
    dm, dq, dt, dA = dev(sift, matches), dev(sift, q_xy), dev(sift, t_xy), dev(sift, As)
    dc = dev(sift, np.int32([count])) if count is not None else None
    out = dev(sift, np.full(len(As), -77, np.int32))
    call = v.score_homography_device if homography else v.score_affine_device
    call(dm.value, dc.value if dc else 0, len(matches), dq.value, len(q_xy), dt.value, len(t_xy), dA.value, len(As),
         max_error, out.value, 2, 2)
    return out.to_numpy(np.int32, (len(As),))


@MODELS
def test_score_on_hand_made_models(sift, similarity):
    """score_affine_device equals the mirror, and score_homography_device on the same nine floats."""
    from sift_amd import cv

    n_in, n_out, K = ac.MAIN
    m, q_xy, t_xy, planted = ac.case(n_in, n_out, similarity)
    ref = ac.reference(n_in, n_out, K, similarity)
    At = ac.true_map(similarity).astype(np.float32).reshape(-1)
    shifted = At.copy()
    shifted[2] += 1.5
    nan = np.float32([np.nan, 0, 0, 0, 1, 0, 0, 0, 1])
    As = np.stack([At, shifted, nan, np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1]), ref["H"], ref["Hs"][5], ref["Hs"][6]])
    want = [int(cv.affine_inliers(m, q_xy, t_xy, a, ac.MAX_ERROR).sum()) for a in As]
    got = score(sift, m, q_xy, t_xy, As, ac.MAX_ERROR)
    assert got.tolist() == want
    assert want[0] == n_in and 0 < want[1] < n_in and want[2] == 0 and want[4] == ref["inliers"]
    assert score(sift, m, q_xy, t_xy, As, ac.MAX_ERROR, homography=True).tolist() == want
    head = score(sift, m, q_xy, t_xy, As[:1], ac.MAX_ERROR, count=50)  # a count on the device clamps the list
    assert head.tolist() == [int(cv.affine_inliers(m[:50], q_xy, t_xy, At, ac.MAX_ERROR).sum())]
    # the hand-written case: q = (7, 2), max_error 2; (9, 2) sits on the edge, dx dx == 4, and counts
    hm = np.zeros(3, sift.DMATCH_DTYPE)
    hm["trainIdx"] = [0, 1, 2]
    hq, ht = np.float32([[7, 2]]), np.float32([[9, 2], [9.25, 2], [7, 4]])
    eye = np.eye(3, dtype=np.float32).reshape(-1)
    assert score(sift, hm, hq, ht, [eye], 2.0).tolist() == [2]
    assert score(sift, hm[1:2], hq, ht, [eye], 2.0).tolist() == [0]


@MODELS
def test_bad_records_and_nan_positions_are_inliers_of_nothing(sift, similarity):
    from sift_amd import cv

    n_in, n_out, K = ac.MAIN
    m, q_xy, t_xy, _ = ac.case(n_in, n_out, similarity)
    bad = m.copy()
    rows = np.arange(0, len(m), 7)
    bad["queryIdx"][rows[0::3]] = -1
    bad["queryIdx"][rows[1::3]] = len(q_xy)
    bad["trainIdx"][rows[2::3]] = 2 ** 30
    ref = cv.ransac_affine(bad, q_xy, t_xy, ac.MAX_ERROR, K, 0, similarity)
    got = verify(sift, similarity, bad, q_xy, t_xy, K)
    check_against(got, ref, len(bad), bad)
    assert not got["mask"][rows].any() and ref["hypothesis"] >= 0
    hit = np.isin(got["samples"], rows).any(1)
    assert hit.any() and not got["valid"][hit].any()  # a hypothesis that samples one is invalid
    # the position arrays' declared lengths are the bound, not their allocations
    short = cv.ransac_affine(m, q_xy[:150], t_xy, ac.MAX_ERROR, K, 0, similarity)
    got = verify(sift, similarity, m, q_xy, t_xy, K, nq=150)
    check_against(got, short, len(m), m)
    assert not got["mask"][m["queryIdx"] >= 150].any()
    # NaN positions behave the same
    qn, tn = q_xy.copy(), t_xy.copy()
    qn[m["queryIdx"][rows[0::2]], 0] = np.nan
    tn[m["trainIdx"][rows[1::2]], 1] = np.nan
    ref = cv.ransac_affine(m, qn, tn, ac.MAX_ERROR, K, 0, similarity)
    got = verify(sift, similarity, m, qn, tn, K)
    check_against(got, ref, len(m), m)
    assert not got["mask"][rows].any() and ref["hypothesis"] >= 0
    assert not got["valid"][np.isin(got["samples"], rows).any(1)].any()


@MODELS
def test_count_clamps_and_short_lists_are_empty_results(sift, similarity):
    from sift_amd import cv

    n_in, n_out, K = 24, 9, 128
    m, q_xy, t_xy, _ = ac.case(n_in, n_out, similarity)
    ref = ac.reference(n_in, n_out, K, similarity)
    check_against(verify(sift, similarity, m, q_xy, t_xy, K, count=10 ** 6), ref, len(m), m)  # *count > cap clamps
    size = ac.sample_size(similarity)
    for count in (size, size - 1, 0, -3):
        n = max(count, 0)
        got = verify(sift, similarity, m, q_xy, t_xy, K, count=count)
        check_against(got, cv.ransac_affine(m[:n], q_xy, t_xy, ac.MAX_ERROR, K, 0, similarity), len(m), m)
        assert not got["mask"][n:len(m)].any()
        r = got["result"]
        if n < size:  # the empty result, status 0
            assert (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, n, 0)
            assert not r["H"].any() and got["out_count"] == 0 and not got["mask"][:len(m)].any()
        else:
            assert r["matches"] == n and r["inliers"] >= size
    # cap == 0 with null pointers
    v = sift.Verifier(16, 64)
    res, cnt = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    v.verify_affine_device(0, 0, 0, 0, 0, 0, 0, res.value, 0, cnt.value, 0, hypotheses=64, similarity=similarity)
    r = res.to_numpy(sift.AFFINE_RESULT_DTYPE, (1,))[0]
    assert (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, 0, 0) and not r["H"].any()
    assert int(cnt.to_numpy(np.int32, (1,))[0]) == 0
    A, inl, hyp = v.verify_affine_host(0, 0, 0, 0, 0, 0, 0, hypotheses=64, similarity=similarity)
    assert A.shape == (3, 3) and not A.any() and len(inl) == 0 and hyp == -1


@MODELS
def test_limits_of_a_real_verifier_and_the_host_forms(sift, similarity):
    n_in, n_out, K = 24, 9, 128
    m, q_xy, t_xy, _ = ac.case(n_in, n_out, similarity)
    ref, fit = ac.reference(n_in, n_out, K, similarity), ac.refined(n_in, n_out, K, similarity, 0, 2)
    v = sift.Verifier(len(m), K)
    dm, dq, dt = dev(sift, m), dev(sift, ec.with_stride(q_xy, 3)), dev(sift, ec.with_stride(t_xy, 3))
    res = dev(sift, np.full(52, FILL, np.uint8))
    args = (dq.value, len(q_xy), dt.value, len(t_xy))
    for kw, msg in ((dict(cap=len(m) + 1), "max_matches"), (dict(hypotheses=K + 1), "hypotheses"),
                    (dict(out_ptr=dm.value + 16), "alias"), (dict(max_error=0.0), "max_error")):
        call = dict(dict(cap=len(m), hypotheses=K), **kw)
        with pytest.raises(sift.SiftHipError, match=msg):
            v.verify_affine_device(dm.value, 0, call.pop("cap"), *args, res.value, similarity=similarity, **call)
    p = sift._VerifyParams(K, 0, ac.MAX_ERROR)
    import ctypes
    for model in (-1, 2):  # neither model: refused before anything is launched
        rc = sift.lib().sift_hip_verify_affine_device(v._v, model, dm.value, None, len(m), dq.value, 3, len(q_xy), dt.value,
                                                      3, len(t_xy), ctypes.byref(p), res.value, None, None, None, None)
        assert rc == -1
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    assert (res.to_numpy(np.uint8, (52,)) == FILL).all()
    A, inl, hyp = v.verify_affine_host(dm.value, 0, len(m), *args, hypotheses=K, similarity=similarity)
    assert A.dtype == np.float32 and A.tobytes() == ref["H"].tobytes() and hyp == ref["hypothesis"]
    assert inl.tobytes() == ref["list"].tobytes()
    rec, inl2, mask = v.verify_affine_host(dm.value, 0, len(m), *args, hypotheses=K, full=True, similarity=similarity)
    assert rec["valid_hypotheses"] == ref["valid_hypotheses"] and np.array_equal(mask, ref["mask"])
    assert inl2.tobytes() == inl.tobytes()
    rec2, inl3, mask2, accepted = v.refine_affine_host(dm.value, 0, len(m), *args, rec, mask, ac.MAX_ERROR, 2,
                                                       similarity=similarity)
    assert rec2["H"].tobytes() == fit["H"].tobytes() and rec2["inliers"] == fit["inliers"] and accepted == fit["accepted"]
    assert np.array_equal(mask2, fit["mask"]) and inl3.tobytes() == fit["list"].tobytes()
    assert rec["H"].tobytes() == ref["H"].tobytes()  # the caller's record is not changed
    # the one-shot function uploads the list itself
    A2, inl4, hyp2 = sift.verifyAffine(m, dq.value, dt.value, len(q_xy), len(t_xy), similarity, hypotheses=K)
    assert A2.tobytes() == A.tobytes() and inl4.tobytes() == inl.tobytes() and hyp2 == hyp
    A3, inl5, _ = sift.verifyAffine(m, dq.value, dt.value, len(q_xy), len(t_xy), similarity=similarity, hypotheses=K,
                                    refit=2)
    assert A3.tobytes() == fit["H"].reshape(3, 3).tobytes() and inl5.tobytes() == fit["list"].tobytes()


def test_each_getter_belongs_to_its_model_and_the_other_models_are_unchanged(sift):
    """The three getters answer only after a call of their own model (the affine getter: of its own of the two), and a
    verify_device and a verify_homography_device call on the same verifier, before and after affine calls, give their
    mirrors' bytes."""
    K = 256
    fm, fq, ft, _ = vc.case(*vc.MAIN[:2])
    hm, hq, ht, _ = hc.case(*hc.MAIN[:2])
    am, aq, at, _ = ac.case(*ac.MAIN[:2], False)
    sm, sq, st, _ = ac.case(*ac.MAIN[:2], True)
    v = sift.Verifier(max(len(fm), len(hm), len(am)), K)

    def fundamental():
        dm, dq, dt = dev(sift, fm), dev(sift, fq), dev(sift, ft)
        res, mask = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(len(fm), FILL, np.uint8))
        v.verify_device(dm.value, 0, len(fm), dq.value, len(fq), dt.value, len(ft), res.value, 0, 0, mask.value,
                        vc.MAX_ERROR, K, 0, 2, 2)
        samples, F, valid, counts = v.hypotheses()
        ref = vc.reference(*vc.MAIN[:2], K)
        assert np.array_equal(samples, ref["samples"]) and F.tobytes() == ref["Fs"].tobytes()
        assert np.array_equal(counts, ref["counts"]) and np.array_equal(valid, ref["valid"])
        r = res.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0]
        assert r["F"].tobytes() == ref["F"].tobytes() and (r["hypothesis"], r["inliers"]) == (ref["hypothesis"], ref["inliers"])
        assert np.array_equal(mask.to_numpy(np.uint8, (len(fm),)), ref["mask"])

    def homography():
        dm, dq, dt = dev(sift, hm), dev(sift, hq), dev(sift, ht)
        res, mask = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(len(hm), FILL, np.uint8))
        v.verify_homography_device(dm.value, 0, len(hm), dq.value, len(hq), dt.value, len(ht), res.value, 0, 0,
                                   mask.value, hc.MAX_ERROR, K, 0, 2, 2)
        samples, H, valid, counts = v.homography_hypotheses()
        ref = hc.reference(*hc.MAIN[:2], K)
        assert np.array_equal(samples, ref["samples"]) and H.tobytes() == ref["Hs"].tobytes()
        assert np.array_equal(counts, ref["counts"]) and np.array_equal(valid, ref["valid"])
        r = res.to_numpy(sift.HOMOGRAPHY_RESULT_DTYPE, (1,))[0]
        assert r["H"].tobytes() == ref["H"].tobytes() and (r["hypothesis"], r["inliers"]) == (ref["hypothesis"], ref["inliers"])
        assert np.array_equal(mask.to_numpy(np.uint8, (len(hm),)), ref["mask"])

    def refused(*getters):
        for g in getters:
            with pytest.raises(sift.SiftHipError):
                g()

    affine, similarity = (lambda: v.affine_hypotheses(False)), (lambda: v.affine_hypotheses(True))
    refused(v.hypotheses, v.homography_hypotheses, affine, similarity)  # no verify call has run
    fundamental()
    refused(v.homography_hypotheses, affine, similarity)
    homography()
    refused(v.hypotheses, affine, similarity)
    check_against(Job(sift, False, am, aq, at, K, v=v).verify(), ac.reference(*ac.MAIN[:2], K, False), len(am), am)
    refused(v.hypotheses, v.homography_hypotheses, similarity)
    check_against(Job(sift, True, sm, sq, st, K, v=v).verify(), ac.reference(*ac.MAIN[:2], K, True), len(sm), sm)
    refused(v.hypotheses, v.homography_hypotheses, affine)
    fundamental()
    homography()
    refused(v.hypotheses, affine, similarity)


@MODELS
@pytest.mark.parametrize("rounds", (1, 2))
def test_refit_accepted(sift, similarity, rounds):
    n_in, n_out, K = ac.MAIN
    m, q_xy, t_xy, planted = ac.case(n_in, n_out, similarity)
    job = Job(sift, similarity, m, q_xy, t_xy, K)
    before = job.verify()
    ref = ac.refined(n_in, n_out, K, similarity, 0, rounds)
    got = job.refine(rounds)
    check_record(got, ref, len(m), m)
    assert got["accepted"] == ref["accepted"] >= 1 and got["result"]["H"].tobytes() != before["result"]["H"].tobytes()
    assert ac.rms(got["result"]["H"], m, q_xy, t_xy, planted) < ac.rms(before["result"]["H"], m, q_xy, t_xy, planted)


@MODELS
@pytest.mark.parametrize("rounds", (1, 2))
def test_refit_rejected_changes_no_byte(sift, similarity, rounds):
    shape, max_error, seed = ac.REJECTED[similarity]
    m, q_xy, t_xy, _ = ac.case(*shape[:2], similarity)
    job = Job(sift, similarity, m, q_xy, t_xy, shape[2])
    before = job.verify(seed, max_error)
    check_against(before, ac.reference(*shape, similarity, seed, max_error), len(m), m)
    ref = ac.refined(*shape, similarity, seed, rounds, max_error)
    got = job.refine(rounds, max_error)
    check_record(got, ref, len(m), m)
    assert got["accepted"] == ref["accepted"] == 0
    assert got["result"].tobytes() == before["result"].tobytes() and got["mask"].tobytes() == before["mask"].tobytes()
    assert got["out"].tobytes() == before["out"].tobytes() and got["out_count"] == before["out_count"]


@MODELS
@pytest.mark.parametrize("rounds", (1, 2))
def test_refit_without_a_fit(sift, similarity, rounds):
    """A fit set below the minimum, and one on a line (affine) or at a point (similarity): no refit, the record and
    the mask stay, the list is the mask's; an empty record stays empty."""
    from sift_amd import cv

    m, q_xy, t_xy, planted, kind = ac.degenerate(similarity)
    ref = cv.ransac_affine(m, q_xy, t_xy, ac.MAX_ERROR, ac.DEGENERATE_K, 0, similarity)
    few = np.zeros(len(m), np.uint8)
    few[np.flatnonzero(planted)[: ac.sample_size(similarity) - 1]] = 1
    flat = (kind == (2 if similarity else 1)).astype(np.uint8)
    job = Job(sift, similarity, m, q_xy, t_xy, ac.DEGENERATE_K)
    for mask in (few, flat):
        rec = np.zeros(1, sift.AFFINE_RESULT_DTYPE)[0]
        rec["H"], rec["hypothesis"], rec["matches"], rec["valid_hypotheses"] = ref["H"], ref["hypothesis"], len(m), 7
        rec["inliers"] = int(mask.sum())
        state = dict(ref, mask=mask, inliers=int(mask.sum()), valid_hypotheses=7)
        want = cv.refine_affine(m, q_xy, t_xy, state, ac.MAX_ERROR, rounds, similarity)
        assert want["accepted"] == 0 and not cv.refit_affine(m, q_xy, t_xy, mask, similarity)[1]
        got = job.refine(rounds, state=(rec, mask))
        check_record(got, want, len(m), m)
        assert got["accepted"] == 0 and got["result"].tobytes() == rec.tobytes() and np.array_equal(got["mask"], mask)
    empty = np.zeros(1, sift.AFFINE_RESULT_DTYPE)[0]
    empty["hypothesis"], empty["matches"] = -1, len(m)
    got = job.refine(rounds, state=(empty, np.ones(len(m), np.uint8)))
    assert got["accepted"] == 0 and got["result"].tobytes() == empty.tobytes() and got["mask"].all()
    assert got["out_count"] == len(m) and got["out"].tobytes() == m.tobytes()


def batch_of(sift, similarity, P):
    """P lists with unequal caps: one empty pair, one pair below the sample size, one counted on the device inside a
    larger buffer."""
    size = ac.sample_size(similarity)
    parts = [("case", (24, 9)), ("empty", None), ("case", (size - 1, 0))]
    if P == 7:
        parts += [("capped", None), ("case", (120, 80)), ("case", (3, 0)), ("case", (60, 240))]
    pairs = []
    for what, shape in parts:
        if what == "empty":
            pairs.append(dict(buf=np.zeros(0, sift.DMATCH_DTYPE), n=0, q_xy=np.zeros((1, 2), np.float32),
                              t_xy=np.zeros((1, 2), np.float32)))  # the device gets null pointers and no rows
        elif what == "capped":
            m, q_xy, t_xy, _ = ac.case(*ac.CAPPED[:2], similarity)
            pairs.append(dict(buf=ac.capped(similarity), n=len(m), q_xy=q_xy, t_xy=t_xy))
        else:
            m, q_xy, t_xy, _ = ac.case(*shape, similarity)
            pairs.append(dict(buf=m, n=len(m), q_xy=q_xy, t_xy=t_xy))
    return pairs


@MODELS
@pytest.mark.parametrize("P", (3, 7))
def test_batched_equals_the_single_calls_and_the_rule(sift, similarity, P):
    """Pair p of verify_affine_batched_device and refine_affine_batched_device equals the single call with seed + p
    byte for byte, and the mirror; the _host forms agree with the device forms."""
    from sift_amd import cv

    K, seed, rounds = 64, 2 ** 32 - 2, 2  # the seed wraps inside the batch
    pairs = batch_of(sift, similarity, P)
    caps = [len(p["buf"]) for p in pairs]
    row0 = np.concatenate([[0], np.cumsum(caps)]).astype(int)
    rows = int(row0[-1])
    v = sift.Verifier(rows, K, P)
    dm = dev(sift, np.concatenate([p["buf"] for p in pairs]))
    dc = dev(sift, np.int32([p["n"] for p in pairs]))
    dxy = [(dev(sift, ec.with_stride(p["q_xy"], 3)), dev(sift, ec.with_stride(p["t_xy"], 2))) if len(p["buf"]) else None
           for p in pairs]
    table = [(d[0].value, len(p["q_xy"]), d[1].value, len(p["t_xy"]), cap) if d else (0, 0, 0, 0, 0)
             for p, d, cap in zip(pairs, dxy, caps)]

    def outputs():
        return dict(res=dev(sift, np.full(52 * (P + 1), FILL, np.uint8)), out=dev(sift, np.full(16 * (rows + 8), FILL, np.uint8)),
                    cnt=dev(sift, np.full(4 * (P + 1), FILL, np.uint8)), mask=dev(sift, np.full(rows + 8, FILL, np.uint8)),
                    acc=dev(sift, np.full(4 * (P + 1), FILL, np.uint8)))

    def read(o):
        sift._check(sift.lib().sift_hip_device_sync(), "sync")
        return dict(res=o["res"].to_numpy(sift.AFFINE_RESULT_DTYPE, (P + 1,)), out=o["out"].to_numpy(sift.DMATCH_DTYPE, (rows + 8,)),
                    cnt=o["cnt"].to_numpy(np.int32, (P + 1,)), mask=o["mask"].to_numpy(np.uint8, (rows + 8,)),
                    acc=o["acc"].to_numpy(np.int32, (P + 1,)))

    b = outputs()
    v.verify_affine_batched_device(dm.value, dc.value, table, b["res"].value, b["out"].value, b["cnt"].value,
                                   b["mask"].value, ac.MAX_ERROR, K, seed, 3, 2, similarity=similarity)
    verified = read(b)
    with pytest.raises(sift.SiftHipError):  # the scratch holds P pairs' hypotheses
        v.affine_hypotheses(similarity)
    host = v.verify_affine_batched_host(dm.value, dc.value, table, ac.MAX_ERROR, K, seed, 3, 2, True, similarity)
    b2 = outputs()
    s = outputs()
    for which, o in (("batched", b2), ("single", s)):
        # both refine what the same verify call left: a copy of its records and masks
        o["res"] = dev(sift, verified["res"])
        o["mask"] = dev(sift, verified["mask"])
    v.refine_affine_batched_device(dm.value, dc.value, table, b2["res"].value, b2["mask"].value, b2["out"].value,
                                   b2["cnt"].value, b2["acc"].value, ac.MAX_ERROR, rounds, 3, 2, similarity=similarity)
    refined = read(b2)
    host_refined = v.refine_affine_batched_host(dm.value, dc.value, table, host, ac.MAX_ERROR, rounds, 3, 2, similarity)
    # the single calls, laid out as the batch: verify into fresh outputs, refine on the batch's verified state
    sv = outputs()
    for p, (q, nq, t, nt, cap) in enumerate(table):
        a, sp = int(row0[p]), (seed + p) % 2 ** 32
        lst = (dm.value + 16 * a if cap else 0, dc.value + 4 * p, cap, q, nq, t, nt)
        v.verify_affine_device(*lst, sv["res"].value + 52 * p, sv["out"].value + 16 * a, sv["cnt"].value + 4 * p,
                               sv["mask"].value + a, ac.MAX_ERROR, K, sp, 3, 2, similarity=similarity)
        v.refine_affine_device(*lst, s["res"].value + 52 * p, s["mask"].value + a, s["out"].value + 16 * a,
                               s["cnt"].value + 4 * p, s["acc"].value + 4 * p, ac.MAX_ERROR, rounds, 3, 2,
                               similarity=similarity)
    single_verified, single_refined = read(sv), read(s)
    for key in ("res", "out", "cnt", "mask"):
        assert verified[key].tobytes() == single_verified[key].tobytes(), key
    for key in ("res", "out", "cnt", "mask", "acc"):
        assert refined[key].tobytes() == single_refined[key].tobytes(), key
    for p, pair in enumerate(pairs):
        a, cap, n = int(row0[p]), caps[p], pair["n"]
        ref = cv.ransac_affine(pair["buf"][:n], pair["q_xy"], pair["t_xy"], ac.MAX_ERROR, K, (seed + p) % 2 ** 32, similarity)
        fit = cv.refine_affine(pair["buf"][:n], pair["q_xy"], pair["t_xy"], ref, ac.MAX_ERROR, rounds, similarity)
        for got, want, hrec in ((verified, ref, host[p]), (refined, fit, host_refined[p])):
            r = got["res"][p]
            assert r["H"].tobytes() == want["H"].tobytes(), p
            assert (r["inliers"], r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
                (want["inliers"], want["hypothesis"], n, want["valid_hypotheses"]), p
            assert got["cnt"][p] == want["inliers"] and got["out"][a:a + want["inliers"]].tobytes() == want["list"].tobytes(), p
            assert (got["out"][a + want["inliers"]:a + cap].view(np.uint8) == FILL).all(), p
            assert np.array_equal(got["mask"][a:a + n], want["mask"]), p
            assert hrec[0].tobytes() == r.tobytes() and hrec[1].tobytes() == want["list"].tobytes(), p
            assert np.array_equal(hrec[2][:n], want["mask"]), p
        assert not verified["mask"][a + n:a + cap].any(), p  # a verify call writes every cap byte
        assert refined["acc"][p] == fit["accepted"] == host_refined[p][3], p
        if n < ac.sample_size(similarity):
            assert verified["res"][p]["hypothesis"] == -1 and refined["acc"][p] == 0, p
    for got in (verified, refined):  # nothing behind the batch's own entries and rows
        assert (got["res"][P:].view(np.uint8) == FILL).all() and (got["cnt"][P:].view(np.uint8) == FILL).all()
        assert (got["out"][rows:].view(np.uint8) == FILL).all() and (got["mask"][rows:] == FILL).all()
    assert (refined["acc"][P:].view(np.uint8) == FILL).all() and refined["acc"][:P].max() >= 1
    lists = sift.verifyAffineBatched([p["buf"][:p["n"]] for p in pairs], [(p["q_xy"], p["t_xy"]) for p in pairs],
                                     similarity, hypotheses=K, seed=seed, refit=rounds)
    for p, (A, recs, hyp) in enumerate(lists):
        assert A.tobytes() == refined["res"][p]["H"].tobytes() and hyp == refined["res"][p]["hypothesis"], p
        assert len(recs) == refined["cnt"][p], p


@MODELS
def test_chain_on_one_stream(sift, similarity):
    """match_list_device -> verify_affine_device (its count taken from the list's device counter) ->
    refine_affine_device -> project_homography_device (H = the result record's device address) ->
    match_list_guided_device on the projected positions, on one stream with no host synchronisation and no read-back
    between the calls.  Every stage equals the same step through the numpy mirrors."""
    import torch

    from sift_amd import cv

    q, t, q_xy, t_xy, planted = ac.chain_case(similarity, 65, 64)
    nq, nt, K, radius, rounds = len(q), len(t), 128, 2.0, 2
    up = lambda rows: dev(sift, rows.astype(np.float16).view(np.uint16))  # noqa: E731
    dq, dt, dqxy, dtxy = up(q), up(t), dev(sift, ec.with_stride(q_xy, 3)), dev(sift, ec.with_stride(t_xy, 3))
    m, v = sift.Matcher(max(nq, nt), max(nq, nt), max_pairs=2), sift.Verifier(nq, K)
    lst, cnt = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    res, mask = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(nq, FILL, np.uint8))
    inl, icnt, acc = (dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8)),
                      dev(sift, np.full(4, FILL, np.uint8)))
    proj = dev(sift, np.full(8 * nq, FILL, np.uint8))
    out2, cnt2 = dev(sift, np.full(16 * nq, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    warm, wcnt = dev(sift, np.zeros(16 * nq, np.uint8)), dev(sift, np.zeros(4, np.uint8))
    # the matcher's first list calls allocate: both kinds once, outside the chain
    m.match_list_device(dq.value, nq, dt.value, nt, warm.value, wcnt.value)
    m.match_list_guided_device(dq.value, nq, dt.value, nt, dqxy.value, dtxy.value, radius, warm.value, wcnt.value, 3, 3)
    sift.lib().sift_hip_device_sync()
    s = torch.cuda.Stream()
    st = s.cuda_stream
    m.match_list_device(dq.value, nq, dt.value, nt, lst.value, cnt.value, stream=st)
    v.verify_affine_device(lst.value, cnt.value, nq, dqxy.value, nq, dtxy.value, nt, res.value, 0, 0, mask.value,
                           ac.MAX_ERROR, K, 0, 3, 3, stream=st, similarity=similarity)
    v.refine_affine_device(lst.value, cnt.value, nq, dqxy.value, nq, dtxy.value, nt, res.value, mask.value, inl.value,
                           icnt.value, acc.value, ac.MAX_ERROR, rounds, 3, 3, stream=st, similarity=similarity)
    sift.project_homography_device(res.value, dqxy.value, nq, proj.value, 3, 2, stream=st)
    m.match_list_guided_device(dq.value, nq, dt.value, nt, proj.value, dtxy.value, radius, out2.value, cnt2.value, 2, 3,
                               stream=st)
    s.synchronize()
    # the mirrors
    every = np.ones((nq, nt), bool)
    fwd, rev = cv.mask_top2(q, t, every), cv.mask_top2(t, q, every.T)
    putative = cv.filter_matches(fwd[0], fwd[1], rev[0], rev[1])
    ver = cv.ransac_affine(putative, q_xy, t_xy, ac.MAX_ERROR, K, 0, similarity)
    ref = cv.refine_affine(putative, q_xy, t_xy, ver, ac.MAX_ERROR, rounds, similarity)
    assert ref["hypothesis"] >= 0 and len(putative) >= 16 and ref["inliers"] >= 16 and ref["accepted"] >= 1
    n1 = int(cnt.to_numpy(np.int32, (1,))[0])
    assert lst.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n1].tobytes() == putative.tobytes()
    r = res.to_numpy(sift.AFFINE_RESULT_DTYPE, (1,))[0]
    assert r["H"].tobytes() == ref["H"].tobytes() and r["hypothesis"] == ref["hypothesis"] and r["matches"] == n1
    assert r["inliers"] == ref["inliers"] and int(acc.to_numpy(np.int32, (1,))[0]) == ref["accepted"]
    assert np.array_equal(mask.to_numpy(np.uint8, (nq,))[:n1], ref["mask"])
    n2 = int(icnt.to_numpy(np.int32, (1,))[0])
    assert inl.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n2].tobytes() == ref["list"].tobytes()
    want_proj = cv.project_homography(ref["H"], q_xy)
    assert proj.to_numpy(np.float32, (nq, 2)).tobytes() == want_proj.tobytes()
    gf = cv.guided_top2(q, t, want_proj, t_xy, radius)
    gr = cv.guided_top2(t, q, t_xy, want_proj, radius)
    guided = cv.filter_matches(gf[0], gf[1], gr[0], gr[1])
    n3 = int(cnt2.to_numpy(np.int32, (1,))[0])
    assert out2.to_numpy(sift.DMATCH_DTYPE, (nq,))[:n3].tobytes() == guided.tobytes()
    # every planted pair comes back: its query, carried over by the map, lies inside its train row's window
    assert set(map(tuple, planted.tolist())) <= {(a, b) for a, b in zip(guided["queryIdx"], guided["trainIdx"])}


@MODELS
def test_batched_chain_on_one_stream(sift, similarity):
    """match_list_batched -> verify_affine_batched_device -> refine_affine_batched_device ->
    project_homography_batched_device reading the records at stride 52 -> match_list_guided_batched, on one stream
    with no read-back until the end: every pair equals the numpy chain."""
    import torch

    import test_gpu_match_guided_batched as gb
    from sift_amd import cv

    K, seed, radius, rounds = 128, 5, 2.0, 2
    views = lambda rng, k: ac.planted_pairs(rng, k, similarity)  # noqa: E731
    pairs = gb.chain_pairs(lambda nq, nt, s: gb.planted_pair(nq, nt, s, views), [(65, 64), (40, 48), (3, 3)])
    up = gb.Uploaded(sift, pairs, 3, 3)
    P, rows = len(pairs), up.rows
    m, v = sift.Matcher(65, 65, max_pairs=2 * P), sift.Verifier(rows, K, P)
    lst, cnt = gb.Guarded(sift, rows, sift.DMATCH_DTYPE), gb.Guarded(sift, P, np.int32)
    res, mask = gb.Guarded(sift, P, sift.AFFINE_RESULT_DTYPE), gb.Guarded(sift, (rows + 3) // 4, np.int32)
    acc = gb.Guarded(sift, P, np.int32)
    proj = [gb.Guarded(sift, n, np.float32, 2) for n in up.nq]
    out2, cnt2 = gb.Guarded(sift, rows, sift.DMATCH_DTYPE), gb.Guarded(sift, P, np.int32)
    warm, wcnt = dev(sift, np.zeros(16 * rows, np.uint8)), dev(sift, np.zeros(4 * P, np.uint8))
    m.match_list_batched(*up.sets(), warm.value, wcnt.value)  # the matcher's first list call allocates
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    vpairs = [(a, n, b, k, n) for a, n, b, k in up.positions()]
    s = torch.cuda.Stream()
    st = s.cuda_stream
    m.match_list_batched(*up.sets(), lst.value, cnt.value, stream=st)
    v.verify_affine_batched_device(lst.value, cnt.value, vpairs, res.value, 0, 0, mask.value, ac.MAX_ERROR, K, seed, 3, 3,
                                   stream=st, similarity=similarity)
    v.refine_affine_batched_device(lst.value, cnt.value, vpairs, res.value, mask.value, 0, 0, acc.value, ac.MAX_ERROR,
                                   rounds, 3, 3, stream=st, similarity=similarity)
    sift.project_homography_batched_device(res.value, [(a.value, n, o.value) for a, n, o in zip(up.qxy, up.nq, proj)],
                                           3, 2, 52, stream=st)
    pos = [(o.value, n, b.value, k) for o, n, b, k in zip(proj, up.nq, up.txy, up.nt)]
    m.match_list_guided_batched(*up.sets(), pos, radius, out2.value, cnt2.value, 2, 3, stream=st)
    s.synchronize()
    (r, ok1), (got_acc, ok2), (rec2, ok3), (n2, ok4), (mk, ok5) = res.read(), acc.read(), out2.read(), cnt2.read(), mask.read()
    assert ok1 and ok2 and ok3 and ok4 and ok5
    r, rec2, n2, mk = r.reshape(-1), rec2.reshape(-1), n2.reshape(-1), mk.reshape(-1).view(np.uint8)
    putative = gb.putative_lists(pairs)
    changed = 0
    for p, pair in enumerate(pairs):
        ver = cv.ransac_affine(putative[p], pair["q_xy"], pair["t_xy"], ac.MAX_ERROR, K, seed + p, similarity)
        ref = cv.refine_affine(putative[p], pair["q_xy"], pair["t_xy"], ver, ac.MAX_ERROR, rounds, similarity)
        changed += ref["accepted"] > 0
        assert r[p]["H"].tobytes() == ref["H"].tobytes() and r[p]["inliers"] == ref["inliers"], p
        assert got_acc.reshape(-1)[p] == ref["accepted"], p
        assert mk[up.row0[p]:up.row0[p] + len(putative[p])].tobytes() == ref["mask"].tobytes(), p
        want_proj = cv.project_homography(ref["H"], pair["q_xy"])
        got_proj, okp = proj[p].read()
        assert okp and got_proj.tobytes() == want_proj.tobytes(), p
        fwd = cv.guided_top2(pair["q"], pair["t"], want_proj, pair["t_xy"], radius)
        rev = cv.guided_top2(pair["t"], pair["q"], pair["t_xy"], want_proj, radius)
        want2 = cv.filter_matches(*fwd, *rev, img_idx=p)
        assert n2[p] == len(want2) and rec2[up.row0[p]:up.row0[p] + n2[p]].tobytes() == want2.tobytes(), p
    assert changed > 0  # at least one pair's model is the refit: the rematch read refined records
