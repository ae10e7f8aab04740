"""k nearest neighbours and capped radius lists on the GPU (sift_hip_match_knn_*, k_match_knn, k_knn_select).

The bar: the device tables equal sift_amd.cv.knn, and the lists sift_amd.cv.knn_records, as raw bytes (integer sets:
exact distances, ties to the lower train index at every rank); at k = 2 the tables are Matcher.match_device's idx2 / d2
on both paths; on the general path at k = 8 the entries keep items 1, 2, 4 and 7 of the general-path contract.
"""
import ctypes

import numpy as np
import pytest

import general_cases as gc
import knn_cases as kc
from test_gpu_match_list import top2, upload

pytestmark = pytest.mark.gpu

FILL = -7
FLT_MAX = kc.FLT_MAX


def same(a, b):
    """Raw-byte equality of two arrays, or of two sequences of arrays."""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def knn_dev(sift, m, qp, nq, tp, nt, k, **kw):
    """The tables of match_knn_device, (nq, k) each, over a fill pattern."""
    idx = sift.DeviceArray.from_numpy(np.full(max(nq * k, 1), FILL, np.int32))
    d2 = sift.DeviceArray.from_numpy(np.full(max(nq * k, 1), FILL, np.float32))
    m.match_knn_device(qp, nq, tp, nt, k, idx.value, d2.value, **kw)
    return idx.to_numpy(np.int32, (max(nq * k, 1),))[:nq * k].reshape(nq, k), \
        d2.to_numpy(np.float32, (max(nq * k, 1),))[:nq * k].reshape(nq, k)


def knn_rows(sift, q, t, k, m=None):
    m = m or sift.Matcher(max(len(q), 1), max(len(t), 1))
    dq, dt = upload(sift, q), upload(sift, t)
    return knn_dev(sift, m, dq.value, len(q), dt.value, len(t), k)


def knn_list(sift, m, qp, nq, tp, nt, k, max_distance):
    out = sift.DeviceArray.from_numpy(np.full(4 * max(nq * k, 1), FILL, np.int32))
    cnt = sift.DeviceArray.from_numpy(np.full(1, FILL, np.int32))
    m.match_knn_list_device(qp, nq, tp, nt, k, out.value, cnt.value, max_distance)
    n = int(cnt.to_numpy(np.int32, (1,))[0])
    assert 0 <= n <= nq * k, n
    return out.to_numpy(sift.DMATCH_DTYPE, (max(nq * k, 1),))[:n]


@pytest.mark.parametrize("nq,nt,k", kc.SHAPES)
def test_shapes(sift, nq, nt, k):
    q, t = kc.sets(nq, nt)
    ref = kc.reference(nq, nt, k)
    dq, dt = upload(sift, q), upload(sift, t)
    m = sift.Matcher(nq, nt)
    got = knn_dev(sift, m, dq.value, nq, dt.value, nt, k)
    assert same(got, ref), (nq, nt, k, np.flatnonzero((got[0] != ref[0]).any(1))[:8])
    if nt < k:
        assert (got[0][:, nt:] == -1).all() and (got[1][:, nt:] == FLT_MAX).all()
    # the column-prefix property, against the widest table of the shape
    wide = kc.reference(nq, nt, kc.KNN_MAX)
    assert same(got, (np.ascontiguousarray(wide[0][:, :k]), np.ascontiguousarray(wide[1][:, :k])))
    # k = 2 is match_device
    two = knn_dev(sift, m, dq.value, nq, dt.value, nt, 2)
    assert same(two, top2(sift, m, dq.value, nq, dt.value, nt)), (nq, nt)
    # only one output asked for
    idx = sift.DeviceArray.from_numpy(np.full(nq * k, FILL, np.int32))
    m.match_knn_device(dq.value, nq, dt.value, nt, k, idx.value, 0)
    assert np.array_equal(idx.to_numpy(np.int32, (nq, k)), ref[0])
    assert same(m.match_knn_host(dq.value, nq, dt.value, nt, k), ref)


def test_the_big_shape_splits(sift):
    assert sift.Matcher.knn_plan(*kc.BIG, 1, 8) >= 2


def test_split_case_and_determinism(sift):
    from sift_amd import cv

    nq, nt = kc.split_shape(sift.Matcher.knn_plan)
    S = sift.Matcher.knn_plan(nq, nt, 1, 8)
    print("split case", nq, nt, "S =", S)
    assert S >= 2 and nt < 8192
    q, t = kc.split_sets(nt)
    assert nt > 256 and np.array_equal(t[255], q[0]) and np.array_equal(t[256], q[0])  # a tie across the two splits
    for k in (3, 8):
        ref = cv.knn(q, t, k)
        m = sift.Matcher(nq, nt)
        dq, dt = upload(sift, q), upload(sift, t)
        a = knn_dev(sift, m, dq.value, nq, dt.value, nt, k)
        b = knn_dev(sift, m, dq.value, nq, dt.value, nt, k)  # the done counters were restored
        assert same(a, ref), k
        assert same(a, b), k
        assert same(a, knn_dev(sift, sift.Matcher(nq, nt), dq.value, nq, dt.value, nt, k)), k


def test_ties(sift):
    from sift_amd import cv

    q, t = kc.tie_sets()
    ref = cv.knn(q, t, 8)
    assert ref[0][0].tolist() == sorted(kc.TIE_ROWS)[:8] and not ref[1][0].any()
    got = knn_rows(sift, q, t, 8)
    assert got[0][0].tolist() == sorted(kc.TIE_ROWS)[:8] and not got[1][0].any()
    assert same(got, ref)
    assert same(knn_rows(sift, q, t, 4), cv.knn(q, t, 4))


def test_low_entropy(sift):
    from sift_amd import cv

    q, t = kc.low_entropy()
    ref = cv.knn(q, t, 8)
    assert (ref[1][:, 1:] == ref[1][:, :-1]).any(1).mean() > 0.5  # most rows hold a tie between adjacent ranks
    assert same(knn_rows(sift, q, t, 8), ref)


def test_key_range(sift):
    from sift_amd import cv

    f = gc.fullrange()
    ref = cv.knn(f.q, f.t, 8)
    assert same((np.ascontiguousarray(ref[0][:, :2]), np.ascontiguousarray(ref[1][:, :2])), f.fwd["none"])
    assert same(knn_rows(sift, f.q, f.t, 8), ref)
    rref = cv.knn(f.t, f.q, 8)
    assert same(knn_rows(sift, f.t, f.q, 8), rref)


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_general_path_k2_is_match_device(sift, family):
    c = gc.case(family)
    dq, dt = upload(sift, c.q), upload(sift, c.t)
    for pairs in (1, 4):
        m = sift.Matcher(gc.NT, gc.NT, pairs)
        assert same(knn_dev(sift, m, dq.value, gc.NQ, dt.value, gc.NT, 2), top2(sift, m, dq.value, gc.NQ, dt.value, gc.NT))
        assert same(knn_dev(sift, m, dt.value, gc.NT, dq.value, gc.NQ, 2), top2(sift, m, dt.value, gc.NT, dq.value, gc.NQ))


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_general_path_k8(sift, family):
    c = gc.case(family)
    D, B = c.fwd.D, c.fwd.B
    idx, d2 = knn_rows(sift, c.q, c.t, 8)
    rows = np.arange(gc.NQ)[:, None]
    assert (idx >= 0).all() and (idx < gc.NT).all()
    assert not np.isnan(d2).any() and (d2 >= 0).all()
    # sorted by (d2, idx)
    d_lo, d_hi, i_lo, i_hi = d2[:, :-1], d2[:, 1:], idx[:, :-1], idx[:, 1:]
    assert ((d_lo < d_hi) | ((d_lo == d_hi) & (i_lo < i_hi))).all()
    err = np.abs(d2.astype(np.float64) - D[rows, idx])
    print(family, "max |d2 - D| / B", float((err / B[rows, idx]).max()))
    assert (err <= B[rows, idx]).all()
    assert all(len(set(r)) == 8 for r in idx.tolist())
    # every candidate left out is no closer than the last one returned, within the bound
    Bq = B.max(1)
    rest = np.ones((gc.NQ, gc.NT), bool)
    rest[rows, idx] = False
    last = D[np.arange(gc.NQ), idx[:, -1]]
    assert (np.where(rest, D, np.inf).min(1) >= last - 2 * Bq).all()
    # the double duplicate: 7 before 900 with identical d2 bits, first of the row
    qd, (ta, tb) = gc.DUP_DOUBLE
    assert idx[qd, :2].tolist() == [ta, tb] and d2[qd, 0].tobytes() == d2[qd, 1].tobytes()
    # both kernel instantiations and the prefix property on the general path
    four = knn_rows(sift, c.q, c.t, 4)
    assert same(four, (np.ascontiguousarray(idx[:, :4]), np.ascontiguousarray(d2[:, :4])))


def test_general_path_special_values(sift):
    from sift_amd import cv

    c = gc.case("sift_unrounded")
    q, t = c.q.copy(), c.t.copy()
    q[10, 3] = np.nan
    t[gc.DUP_SINGLE[1], 9] = np.inf
    t[gc.NT - 3, 40] = -np.inf
    idx, d2 = knn_rows(sift, q, t, 8)
    assert (idx[10] == -1).all() and (d2[10] == FLT_MAX).all()
    assert not np.isin(idx, [gc.DUP_SINGLE[1], gc.NT - 3]).any()
    good = np.setdiff1d(np.arange(gc.NQ), [10])
    assert (idx[good] >= 0).all() and not np.isnan(d2).any() and (d2 >= 0).all()
    # an integer set with one -0.0 takes the general path and returns the integer path's bytes
    f = gc.fullrange()
    ref = cv.knn(f.q, f.t, 8)
    for side in ("query", "train"):
        qz, tz = f.q.copy(), f.t.copy()
        if side == "query":
            qz[gc.MINUS_ZERO_QUERY, 17] = -0.0
        else:
            tz[gc.MINUS_ZERO_TRAIN, 90] = -0.0
        assert np.signbit(qz).any() or np.signbit(tz).any()
        assert same(knn_rows(sift, qz, tz, 8), ref), side


def test_batched_codes_and_max_pairs(sift):
    import torch

    from sift_amd import multi

    q, t = kc.sets(*kc.BIG)
    q2, t2 = kc.sets(70, 300)
    dq, dt, dq2, dt2 = upload(sift, q), upload(sift, t), upload(sift, q2), upload(sift, t2)
    k = 5
    # three ragged pairs, one sharing a set with another, against the three single calls
    pairs = [(dq, 300, dt, 1100), (dq2, 70, dt2, 300), (dq, 257, dt2, 33)]
    m1, m4 = sift.Matcher(1100, 1100, 1), sift.Matcher(1100, 1100, 4)
    singles = [knn_dev(sift, m1, a.value, na, b.value, nb, k) for a, na, b, nb in pairs]
    assert same(singles, [knn_dev(sift, m4, a.value, na, b.value, nb, k) for a, na, b, nb in pairs])  # max_pairs 1 and 4
    tot = sum(p[1] for p in pairs)
    idx = sift.DeviceArray.from_numpy(np.full(tot * k, FILL, np.int32))
    d2 = sift.DeviceArray.from_numpy(np.full(tot * k, FILL, np.float32))
    m4.match_knn_batched([p[0].value for p in pairs], [p[1] for p in pairs], [p[2].value for p in pairs],
                         [p[3] for p in pairs], k, idx.value, d2.value)
    gi, gd = idx.to_numpy(np.int32, (tot, k)), d2.to_numpy(np.float32, (tot, k))
    off = 0
    for (si, sd), p in zip(singles, pairs):
        assert same((gi[off:off + p[1]], gd[off:off + p[1]]), (si, sd)), p[1:]
        off += p[1]
    # ready codes: both sets in one buffer (codes rows, then keys), against the fp16 call
    rows = torch.from_numpy(np.concatenate([q, t]).astype(np.float16).view(np.int16)).cuda()
    cq, kq = multi.codes_from_rows(rows[:300])
    ct, kt = multi.codes_from_rows(rows[300:])
    codes, keys = torch.cat([cq, ct]).contiguous(), torch.cat([kq, kt]).contiguous()
    ci = torch.full((300, k), FILL, dtype=torch.int32, device="cuda")
    cd = torch.full((300, k), float(FILL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m4.match_knn_codes_batched(codes.data_ptr(), keys.data_ptr(), [(0, 0, 300, 300, 300, 1100)], k, ci.data_ptr(),
                               cd.data_ptr())
    torch.cuda.synchronize()
    assert same((ci.cpu().numpy(), cd.cpu().numpy()), singles[0])


def test_lists(sift):
    from sift_amd import cv

    q, t = kc.sets(*kc.BIG)
    nq, nt = kc.BIG
    k = 4
    ref = kc.reference(nq, nt, k)
    dist = np.sqrt(ref[1])
    cap = float(np.median(dist))  # from the case: about half of the table
    dq, dt = upload(sift, q), upload(sift, t)
    m = sift.Matcher(nt, nt, 3)
    exp = cv.knn_records(*ref, max_distance=cap)
    assert 0 < len(exp) < nq * k
    assert same(knn_list(sift, m, dq.value, nq, dt.value, nt, k, cap), exp)
    whole = knn_list(sift, m, dq.value, nq, dt.value, nt, k, 0.0)
    assert len(whole) == nq * k and same(whole, cv.knn_records(*ref))
    assert same(m.match_knn_list_host(dq.value, nq, dt.value, nt, k, cap), exp)
    # three ragged pairs: imgIdx = p, pair p from row k * sum nq
    q2, t2 = kc.sets(70, 300)
    dq2, dt2 = upload(sift, q2), upload(sift, t2)
    pairs = [(dq, q, 300, dt, t, 1100), (dq2, q2, 70, dt2, t2, 300), (dq, q, 257, dt2, t2, 33)]
    tot = sum(p[2] for p in pairs)
    out = sift.DeviceArray.from_numpy(np.full(4 * tot * k, FILL, np.int32))
    cnt = sift.DeviceArray.from_numpy(np.full(3, FILL, np.int32))
    m.match_knn_list_batched([p[0].value for p in pairs], [p[2] for p in pairs], [p[3].value for p in pairs],
                             [p[5] for p in pairs], k, out.value, cnt.value, cap)
    counts, recs = cnt.to_numpy(np.int32, (3,)), out.to_numpy(sift.DMATCH_DTYPE, (tot * k,))
    off = 0
    for p, (_, qr, n, _, tr, ntp) in enumerate(pairs):
        e = cv.knn_records(*cv.knn(qr[:n], tr[:ntp], k), max_distance=cap, img_idx=p)
        assert counts[p] == len(e) and same(recs[k * off: k * off + len(e)], e), p
        off += n
    # nt == 0: a table of -1 / FLT_MAX and an empty list; nq == 0: nothing written, count 0
    gi, gd = knn_dev(sift, m, dq.value, 5, 0, 0, 3)
    assert (gi == -1).all() and (gd == FLT_MAX).all()
    assert len(knn_list(sift, m, dq.value, 5, 0, 0, 3, 0.0)) == 0
    assert len(knn_list(sift, m, 0, 0, dt.value, 5, 3, 0.0)) == 0
    m.match_knn_device(0, 0, dt.value, 5, 3, 0, 0)


def test_detector_buffers(sift):
    import os

    from sift_amd import cv

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera256.npz")
    img = np.load(gold)["camera256"].astype(np.float32)
    det = sift.Detector(sift.CudaSiftConfig(col_width=256, row_width=256, upscale=True, numFeatures=0), lanes=1)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(img)
    det.copyToHost(True)
    n0 = det.total_size
    d0 = det.descriptors.astype(np.float32).reshape(n0, 128).copy()
    det.detectAndCompute(np.ascontiguousarray(np.rot90(img)))
    det.copyToHost(True)
    n1 = det.total_size
    d1 = det.descriptors.astype(np.float32).reshape(n1, 128).copy()
    assert n0 > 100 and n1 > 100 and det.prev_size == n0
    qp, tp = det.prev_descriptor.data(), det.device_descriptor.data()
    cap = max(n0, n1)
    m, mc = sift.Matcher(cap, cap), sift.Matcher(cap, cap)
    mc.set_sidecars(False)
    assert same(knn_dev(sift, m, qp, n0, tp, n1, 2), top2(sift, m, qp, n0, tp, n1))
    ref = cv.knn(d0, d1, 8)
    side = knn_dev(sift, m, qp, n0, tp, n1, 8)
    assert same(side, ref)
    assert same(knn_dev(sift, mc, qp, n0, tp, n1, 8), ref)  # the converting path
    assert same(sift.knnMatch(det.prev_descriptor, n0, det.device_descriptor, n1, 8), ref)
    assert same(sift.matchKnnList(det.prev_descriptor, n0, det.device_descriptor, n1, 3, 200.0),
                cv.knn_records(*cv.knn(d0, d1, 3), max_distance=200.0))
    det.device_descriptor.mutable_data()  # the sidecar is stale: the rows are converted
    assert same(knn_dev(sift, m, qp, n0, tp, n1, 8), ref)


def test_into_the_verifier(sift):
    import torch

    import epipolar_cases as ec
    from sift_amd import cv

    q, t, q_xy, t_xy = ec.case(65, 64)[:4]
    nq, nt, K, k = len(q), len(t), 256, 3
    dev = lambda a: sift.DeviceArray.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    dq, dt = upload(sift, q), upload(sift, t)
    dqxy, dtxy = dev(ec.with_stride(q_xy, 3)), dev(ec.with_stride(t_xy, 3))
    m, v = sift.Matcher(max(nq, nt), max(nq, nt)), sift.Verifier(nq * k, K)
    lst, cnt = dev(np.full(4 * nq * k, FILL, np.int32)), dev(np.full(1, FILL, np.int32))
    res = dev(np.full(52, 0xCD, np.uint8))
    inl, icnt = dev(np.full(4 * nq * k, FILL, np.int32)), dev(np.full(1, FILL, np.int32))
    mask = dev(np.full(nq * k, 0xCD, np.uint8))
    m.match_knn_list_device(dq.value, nq, dt.value, nt, k, lst.value, cnt.value)  # the first k-NN call allocates
    sift.lib().sift_hip_device_sync()
    s = torch.cuda.Stream()
    m.match_knn_list_device(dq.value, nq, dt.value, nt, k, lst.value, cnt.value, stream=s.cuda_stream)
    v.verify_device(lst.value, cnt.value, nq * k, dqxy.value, nq, dtxy.value, nt, res.value, inl.value, icnt.value,
                    mask.value, ec.MAX_ERROR, K, 0, 3, 3, stream=s.cuda_stream)
    s.synchronize()
    n = int(cnt.to_numpy(np.int32, (1,))[0])
    recs = lst.to_numpy(sift.DMATCH_DTYPE, (nq * k,))[:n]
    assert n == nq * k and same(recs, cv.knn_records(*cv.knn(q, t, k)))
    ref = cv.ransac_fundamental(recs, q_xy, t_xy, ec.MAX_ERROR, K, 0)
    r = res.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0]
    assert ref["hypothesis"] >= 0 and r["hypothesis"] >= 0
    assert r["F"].tobytes() == ref["F"].tobytes()
    assert (r["inliers"], r["hypothesis"], r["matches"]) == (ref["inliers"], ref["hypothesis"], n)
    assert np.array_equal(mask.to_numpy(np.uint8, (nq * k,))[:n], ref["mask"])
    n2 = int(icnt.to_numpy(np.int32, (1,))[0])
    assert n2 == ref["inliers"] and inl.to_numpy(sift.DMATCH_DTYPE, (nq * k,))[:n2].tobytes() == ref["list"].tobytes()


def test_refusals_launch_nothing(sift):
    L = sift.lib()
    q, t = kc.sets(33, 31)
    dq, dt = upload(sift, q), upload(sift, t)
    m = sift.Matcher(40, 40, 2)
    idx = sift.DeviceArray.from_numpy(np.full(64 * 8, FILL, np.int32))
    d2 = sift.DeviceArray.from_numpy(np.full(64 * 8, FILL, np.float32))
    out = sift.DeviceArray.from_numpy(np.full(4 * 64 * 8, FILL, np.int32))
    cnt = sift.DeviceArray.from_numpy(np.full(1, FILL, np.int32))
    h = m._m
    one, big = (ctypes.c_int * 3)(33, 33, 33), (ctypes.c_int * 3)(41, 33, 33)
    ptrs = (ctypes.c_void_p * 3)(dq.value, dq.value, dq.value)
    bad = [
        L.sift_hip_match_knn_device(h, dq.value, 33, dt.value, 31, 0, idx.value, d2.value, None),
        L.sift_hip_match_knn_device(h, dq.value, 33, dt.value, 31, 9, idx.value, d2.value, None),
        L.sift_hip_match_knn_device(h, dq.value, 41, dt.value, 31, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_device(h, dq.value, 33, dt.value, 41, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_device(h, None, 33, dt.value, 31, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_device(h, dq.value, 33, None, 31, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_batched(h, 3, ptrs, one, ptrs, one, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_batched(h, 0, ptrs, one, ptrs, one, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_batched(h, 2, ptrs, big, ptrs, one, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_list_device(h, dq.value, 33, dt.value, 31, 2, 1.0, None, cnt.value, None),
        L.sift_hip_match_knn_list_device(h, dq.value, 33, dt.value, 31, 2, 1.0, out.value, None, None),
        L.sift_hip_match_knn_list_device(h, dq.value, 33, dt.value, 31, 2, float("nan"), out.value, cnt.value, None),
        L.sift_hip_match_knn_list_device(h, dq.value, 33, dt.value, 31, 9, 1.0, out.value, cnt.value, None),
    ]
    assert bad == [-1] * len(bad), bad
    assert L.sift_hip_last_error()
    L.sift_hip_device_sync()
    assert (idx.to_numpy(np.int32, (64 * 8,)) == FILL).all() and (d2.to_numpy(np.float32, (64 * 8,)) == FILL).all()
    assert (out.to_numpy(np.int32, (4 * 64 * 8,)) == FILL).all() and cnt.to_numpy(np.int32, (1,))[0] == FILL
    with pytest.raises(sift.SiftHipError):
        m.match_knn_device(dq.value, 33, dt.value, 31, 9, idx.value, d2.value)
