"""Gated k nearest neighbours on the GPU (sift_hip_match_knn_guided_* / *_epipolar_*, k_match_knn<K, Gate>).

The bar: the device tables equal sift_amd.cv.guided_knn / epipolar_knn, the lists sift_amd.cv.knn_records of those
tables, as raw bytes; without a gate the tables are Matcher.match_knn_device's, at k = 2 the gated top-2 calls'; pair p
of a batched call is the single-pair call.  Every comparison is byte for byte: the general-path inputs are multiples of
0.5, where fp32 does not round.
"""
import ctypes

import numpy as np
import pytest

import knn_cases as kc
import knn_gated_cases as kg
from test_gpu_match_knn import FILL, knn_dev, same
from test_gpu_match_list import top2, upload

pytestmark = pytest.mark.gpu

FLT_MAX = kc.FLT_MAX
INF = float("inf")


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


class Pair:
    """One pair on the device: fp16 rows and positions (rows of `stride` floats)."""

    def __init__(self, sift, q, t, q_xy, t_xy, stride=2):
        self.q, self.t, self.q_xy, self.t_xy = q, t, q_xy, t_xy
        self.nq, self.nt, self.stride = len(q), len(t), stride
        self.dq, self.dt = upload(sift, q) if len(q) else None, upload(sift, t) if len(t) else None
        self.dqxy = dev(sift, kg.with_stride(q_xy, stride)) if len(q) else None
        self.dtxy = dev(sift, kg.with_stride(t_xy, stride)) if len(t) else None

    def ptrs(self):
        return tuple(a.value if a is not None else 0 for a in (self.dq, self.dt, self.dqxy, self.dtxy))


def tables(sift, n, k, idx=True, d2=True):
    gi = dev(sift, np.full(max(n * k, 1), FILL, np.int32)) if idx else None
    gd = dev(sift, np.full(max(n * k, 1), FILL, np.float32)) if d2 else None
    return gi, gd


def read(gi, gd, n, k):
    out = []
    if gi is not None:
        out.append(gi.to_numpy(np.int32, (max(n * k, 1),))[:n * k].reshape(n, k))
    if gd is not None:
        out.append(gd.to_numpy(np.float32, (max(n * k, 1),))[:n * k].reshape(n, k))
    return tuple(out)


def gated(sift, m, gate, p, k, idx=True, d2=True, radius=None, F=kg.F, max_error=kg.MAX_ERROR, nq=None, nt=None):
    """The tables of the single-pair gated call on pair p: the window of RADIUS, or the band of F (no window)."""
    nq, nt = p.nq if nq is None else nq, p.nt if nt is None else nt
    gi, gd = tables(sift, nq, k, idx, d2)
    qp, tp, qxy, txy = p.ptrs()
    a, b = gi.value if gi else 0, gd.value if gd else 0
    if gate == "window":
        m.match_knn_guided_device(qp, nq, tp, nt, qxy, txy, kg.RADIUS if radius is None else radius, k, a, b,
                                  q_stride=p.stride, t_stride=p.stride)
    else:
        m.match_knn_epipolar_device(qp, nq, tp, nt, qxy, txy, F, max_error, k, a, b,
                                    radius=INF if radius is None else radius, q_stride=p.stride, t_stride=p.stride)
    return read(gi, gd, nq, k)


def gated_list(sift, m, gate, p, k, max_distance):
    out = dev(sift, np.full(4 * max(p.nq * k, 1), FILL, np.int32))
    cnt = dev(sift, np.full(1, FILL, np.int32))
    qp, tp, qxy, txy = p.ptrs()
    if gate == "window":
        m.match_knn_list_guided_device(qp, p.nq, tp, p.nt, qxy, txy, kg.RADIUS, k, out.value, cnt.value, max_distance,
                                       q_stride=p.stride, t_stride=p.stride)
    else:
        m.match_knn_list_epipolar_device(qp, p.nq, tp, p.nt, qxy, txy, kg.F, kg.MAX_ERROR, k, out.value, cnt.value,
                                         max_distance, q_stride=p.stride, t_stride=p.stride)
    n = int(cnt.to_numpy(np.int32, (1,))[0])
    assert 0 <= n <= p.nq * k, n
    recs = out.to_numpy(sift.DMATCH_DTYPE, (max(p.nq * k, 1),))
    assert (recs[n:p.nq * k].view(np.int32) == FILL).all()  # rows past the count are not written
    return recs[:n]


def prefix(table, k):
    return np.ascontiguousarray(table[0][:, :k]), np.ascontiguousarray(table[1][:, :k])


@pytest.fixture(scope="module")
def big(sift):
    return Pair(sift, *kc.sets(*kc.BIG), *kg.positions(*kc.BIG))


@pytest.mark.parametrize("gate", kg.GATES)
@pytest.mark.parametrize("nq,nt,k", kc.SHAPES)
def test_shapes(sift, gate, nq, nt, k):
    ref = kg.reference(gate, nq, nt, k)
    p = Pair(sift, *kc.sets(nq, nt), *kg.positions(nq, nt), stride=2 if nq % 2 else 5)
    m = sift.Matcher(nq, nt)
    got = gated(sift, m, gate, p, k)
    assert same(got, ref), (gate, nq, nt, k, np.flatnonzero((got[0] != ref[0]).any(1))[:8])
    assert same(gated(sift, m, gate, p, k, d2=False), ref[:1])
    assert same(gated(sift, m, gate, p, k, idx=False), ref[1:])
    qp, tp, qxy, txy = p.ptrs()
    if gate == "window":
        host = m.match_knn_guided_host(qp, nq, tp, nt, qxy, txy, kg.RADIUS, k, p.stride, p.stride)
    else:
        host = m.match_knn_epipolar_host(qp, nq, tp, nt, qxy, txy, kg.F, kg.MAX_ERROR, k, INF, p.stride, p.stride)
    assert same(host, ref)


def test_identities(sift, big):
    q, t = kc.sets(*kc.BIG)
    q_xy, t_xy = (np.nan_to_num(a, nan=1.0) for a in kg.positions(*kc.BIG))  # a NaN is a candidate of nothing
    clean = Pair(sift, q, t, q_xy, t_xy, stride=3)
    m = sift.Matcher(*kc.BIG)
    for k in (3, 8):  # both instantiations
        plain = knn_dev(sift, m, clean.dq.value, clean.nq, clean.dt.value, clean.nt, k)
        assert same(plain, kc.reference(*kc.BIG, k))
        assert same(gated(sift, m, "window", clean, k, radius=INF), plain), k
        assert same(gated(sift, m, "band", clean, k, max_error=1e30), plain), k
    # k = 2 is the gated top-2 calls' idx2 / d2
    qp, tp, qxy, txy = big.ptrs()
    for gate in kg.GATES:
        i2, e2 = tables(sift, big.nq, 2)
        if gate == "window":
            m.match_guided_device(qp, big.nq, tp, big.nt, qxy, txy, kg.RADIUS, 2, 2, idx2_ptr=i2.value, d2_ptr=e2.value)
        else:
            m.match_epipolar_device(qp, big.nq, tp, big.nt, qxy, txy, kg.F, kg.MAX_ERROR, INF, 2, 2, idx2_ptr=i2.value,
                                    d2_ptr=e2.value)
        assert same(gated(sift, m, gate, big, 2), read(i2, e2, big.nq, 2)), gate
        # the column prefix across every served k: both instantiations give one table
        wide = gated(sift, m, gate, big, 8)
        assert same(wide, kg.reference(gate, *kc.BIG, 8))
        for k in kg.KS:
            assert same(gated(sift, m, gate, big, k), prefix(wide, k)), (gate, k)
    # the band inside a window
    from sift_amd import cv

    both = gated(sift, m, "band", big, 5, radius=kg.RADIUS)
    assert same(both, cv.epipolar_knn(q, t, *kg.positions(*kc.BIG), kg.F, kg.MAX_ERROR, 5, radius=kg.RADIUS))


@pytest.mark.parametrize("gate", kg.GATES)
def test_ties_and_low_entropy(sift, gate):
    q, t = kc.tie_sets()
    m = sift.Matcher(*kc.BIG)
    for variant in ("a", "b"):
        q_xy, t_xy = kg.tie_positions(variant)
        p = Pair(sift, q, t, q_xy, t_xy)
        for k in (4, 8):
            got = gated(sift, m, gate, p, k)
            assert same(got, kg.mirror(gate, q, t, q_xy, t_xy, k)), (gate, variant, k)
        inside = sorted(kg.TIE_INSIDE[variant])
        assert got[0][0, :7].tolist() == inside and not got[1][0, :7].any() and got[1][0, 7] > 0
    q, t = kc.low_entropy()
    q_xy, t_xy = kg.positions(len(q), len(t))
    ref = kg.mirror(gate, q, t, q_xy, t_xy, 8)
    assert (ref[0] >= 0).sum() > len(q) and ((ref[1][:, 1:] == ref[1][:, :-1]) & (ref[0][:, 1:] >= 0)).any()
    assert same(gated(sift, sift.Matcher(len(q), len(t)), gate, Pair(sift, q, t, q_xy, t_xy), 8), ref)


@pytest.mark.parametrize("gate", kg.GATES)
def test_split_case_and_determinism(sift, gate):
    nq, nt = kc.split_shape(sift.Matcher.knn_plan)
    assert sift.Matcher.knn_plan(nq, nt, 1, 8) >= 2 and nt > 256
    q, t = kc.split_sets(nt)
    for variant in ("a", "b"):  # rows 255 / 256: the tie is cut by the key group, the split and the gate
        q_xy, t_xy = kg.tie_positions(variant)
        p = Pair(sift, q, t, q_xy, t_xy[:nt])
        m = sift.Matcher(nq, nt)
        for k in (3, 8):
            ref = kg.mirror(gate, q, t, q_xy, t_xy[:nt], k)
            a = gated(sift, m, gate, p, k)
            b = gated(sift, m, gate, p, k)  # the done counters were restored
            assert same(a, ref) and same(a, b), (gate, variant, k)
            assert same(a, gated(sift, sift.Matcher(nq, nt, 5), gate, p, k))
        assert (255 in a[0][0]) == (variant == "a") and (256 in a[0][0]) == (variant == "b")


@pytest.mark.parametrize("gate", kg.GATES)
def test_general_path(sift, gate):
    q, t = kg.half_sets()
    q_xy, t_xy = kg.positions(70, 300)
    m = sift.Matcher(70, 300)
    p = Pair(sift, q, t, q_xy, t_xy, stride=3)
    for k in (3, 8):
        assert same(gated(sift, m, gate, p, k), kg.mirror(gate, q, t, q_xy, t_xy, k)), (gate, k)
    # a query row with NaN, a train row with inf, NaN positions on both sides
    qs, ts, qx, tx = q.copy(), t.copy(), q_xy.copy(), t_xy.copy()
    qs[7, 3] = np.nan
    ts[40, 9] = np.inf
    qx[9, 1] = np.nan
    tx[3, 0] = np.nan
    ref = kg.mirror(gate, qs, ts, qx, tx, 8)
    assert (ref[0][[7, 9]] == -1).all() and not np.isin(ref[0], [3, 40]).any()
    assert same(gated(sift, m, gate, Pair(sift, qs, ts, qx, tx), 8), ref)
    # one half-valued set is enough to send the pair down the general path; the other set is integers
    qi = np.rint(q)
    assert same(gated(sift, m, gate, Pair(sift, qi, t, q_xy, t_xy), 4), kg.mirror(gate, qi, t, q_xy, t_xy, 4))


def batch_pairs(sift):
    """Three ragged pairs, the last one without train rows; pair 1 shares its train set's buffer with nobody."""
    a = Pair(sift, *kc.sets(*kc.BIG), *kg.positions(*kc.BIG), stride=3)
    b = Pair(sift, *kc.sets(70, 300), *kg.positions(70, 300), stride=3)
    q, q_xy = kc.sets(33, 31)[0], kg.positions(33, 31)[0]
    c = Pair(sift, q, q[:0], q_xy, q_xy[:0], stride=3)
    return [a, b, c]


def run_batched(sift, m, gate, pairs, k, geometry=None, stride=52, lists=None):
    """The batched table call (lists None) or list call (lists = max_distance) on `pairs`."""
    nqs, nts = [p.nq for p in pairs], [p.nt for p in pairs]
    ptrs = [p.ptrs() for p in pairs]
    args = ([x[0] for x in ptrs], nqs, [x[1] for x in ptrs], nts, [(x[2], x[3]) for x in ptrs])
    tot = sum(nqs)
    kw = dict(q_stride=pairs[0].stride, t_stride=pairs[0].stride)
    if lists is None:
        gi, gd = tables(sift, tot, k)
        if gate == "window":
            m.match_knn_guided_batched(*args, kg.RADIUS, k, gi.value, gd.value, **kw)
        else:
            m.match_knn_epipolar_batched(*args, geometry.value, kg.MAX_ERROR, k, gi.value, gd.value,
                                         geometry_stride=stride, **kw)
        idx, d2 = read(gi, gd, tot, k)
        offs = np.concatenate([[0], np.cumsum(nqs)])
        return [(idx[offs[i]:offs[i + 1]], d2[offs[i]:offs[i + 1]]) for i in range(len(pairs))]
    out = dev(sift, np.full(4 * max(tot * k, 1), FILL, np.int32))
    cnt = dev(sift, np.full(len(pairs), FILL, np.int32))
    if gate == "window":
        m.match_knn_list_guided_batched(*args, kg.RADIUS, k, out.value, cnt.value, lists, **kw)
    else:
        m.match_knn_list_epipolar_batched(*args, geometry.value, kg.MAX_ERROR, k, out.value, cnt.value, lists,
                                          geometry_stride=stride, **kw)
    counts = cnt.to_numpy(np.int32, (len(pairs),))
    recs = out.to_numpy(sift.DMATCH_DTYPE, (max(tot * k, 1),))
    res, off = [], 0
    for i, p in enumerate(pairs):
        assert 0 <= counts[i] <= p.nq * k
        assert (recs[k * off + counts[i]:k * (off + p.nq)].view(np.int32) == FILL).all()  # past the count: untouched
        res.append(recs[k * off:k * off + counts[i]])
        off += p.nq
    return res


def geometry(sift, Fs, stride):
    """Records of `stride` bytes: 36 packs the nine floats, 52 is a VERIFY_RESULT_DTYPE array as it lies."""
    if stride == 52:
        rec = np.zeros(len(Fs), sift.VERIFY_RESULT_DTYPE)
        rec["F"] = [np.asarray(f, np.float32).reshape(9) for f in Fs]
        rec["inliers"], rec["hypothesis"], rec["matches"], rec["valid_hypotheses"] = 0x7FC00123, -1, 7, 0x7FC00123
        return dev(sift, rec.view(np.uint8))
    rec = np.full((len(Fs), stride // 4), 0x7FC00123, np.uint32)
    for i, f in enumerate(Fs):
        rec[i, :9] = np.asarray(f, np.float32).reshape(9).view(np.uint32)
    return dev(sift, rec)


SCALES = (1.0, 3.0, 0.7)


@pytest.mark.parametrize("gate", kg.GATES)
def test_batched_is_the_single_pair_call(sift, gate):
    pairs = batch_pairs(sift)
    Fs = [kg.F * np.float32(s) for s in SCALES]
    k = 5
    m1 = sift.Matcher(1100, 1100, 1)
    singles = [gated(sift, m1, gate, p, k, F=f) for p, f in zip(pairs, Fs)]
    assert (singles[2][0] == -1).all() and (singles[2][1] == FLT_MAX).all()  # no train rows
    for p, s, f in zip(pairs[:2], singles, Fs):
        assert same(s, kg.mirror(gate, p.q, p.t, p.q_xy, p.t_xy, k, F=f))
    for max_pairs in (3, 8):
        m = sift.Matcher(1100, 1100, max_pairs)
        for stride in (36, 52) if gate == "band" else (52,):
            got = run_batched(sift, m, gate, pairs, k, geometry(sift, Fs, stride), stride)
            assert same([g[0] for g in got], [s[0] for s in singles]), (gate, max_pairs, stride)
            assert same([g[1] for g in got], [s[1] for s in singles]), (gate, max_pairs, stride)


def test_unusable_geometry_records(sift):
    from sift_amd import cv

    b = Pair(sift, *kc.sets(70, 300), *kg.positions(70, 300), stride=3)
    s = Pair(sift, *kc.sets(33, 31), *kg.positions(33, 31), stride=3)
    pairs, k = [b, s, b], 8
    m = sift.Matcher(300, 300, 4)
    good = gated(sift, m, "band", b, k)
    assert same(good, kg.reference("band", 70, 300, k))
    nan = kg.F.copy()
    nan[1, 1] = np.nan
    for bad in (np.zeros((3, 3), np.float32), nan):
        assert not cv.geometry_usable(bad)
        geo = geometry(sift, [kg.F, bad, kg.F], 52)
        got = run_batched(sift, m, "band", pairs, k, geo)
        assert same(got[0], good) and same(got[2], good)  # the neighbours are unaffected
        assert (got[1][0] == -1).all() and (got[1][1] == FLT_MAX).all()
        lst = run_batched(sift, m, "band", pairs, k, geo, lists=0.0)
        assert len(lst[1]) == 0 and same(lst[0], cv.knn_records(*good, img_idx=0)) \
            and same(lst[2], cv.knn_records(*good, img_idx=2))


def test_33_pairs_cross_the_launch_boundary(sift):
    shapes = [(33, 31), (5, 3)]
    base = [Pair(sift, *kc.sets(*s), *kg.positions(*s), stride=3) for s in shapes]
    pairs = [base[i % 2] for i in range(33)]
    m = sift.Matcher(40, 40, 33)
    k = 3
    for gate in kg.GATES:
        singles = [gated(sift, m, gate, p, k) for p in base]
        assert same(singles, [kg.mirror(gate, p.q, p.t, p.q_xy, p.t_xy, k) for p in base])
        got = run_batched(sift, m, gate, pairs, k, geometry(sift, [kg.F] * 33, 36), 36)
        for i, g in enumerate(got):
            assert same(g, singles[i % 2]), (gate, i)


@pytest.mark.parametrize("gate", kg.GATES)
def test_lists(sift, gate, big):
    from sift_amd import cv

    k = 4
    m = sift.Matcher(1100, 1100, 3)
    ref = kg.reference(gate, *kc.BIG, k)
    dist = np.sqrt(ref[1][ref[0] >= 0])
    cap = float(np.median(dist))  # from the case: about half of the entries
    exp = cv.knn_records(*ref, max_distance=cap)
    assert 0 < len(exp) < (ref[0] >= 0).sum() < big.nq * k
    assert same(gated_list(sift, m, gate, big, k, cap), exp)
    assert same(gated_list(sift, m, gate, big, k, 0.0), cv.knn_records(*ref))
    qp, tp, qxy, txy = big.ptrs()
    if gate == "window":
        host = m.match_knn_list_guided_host(qp, big.nq, tp, big.nt, qxy, txy, kg.RADIUS, k, cap, 2, 2)
    else:
        host = m.match_knn_list_epipolar_host(qp, big.nq, tp, big.nt, qxy, txy, kg.F, kg.MAX_ERROR, k, cap, INF, 2, 2)
    assert same(host, exp)
    # batched: imgIdx = p, pair p's records from row k * sum nq, the empty-train pair counts 0
    pairs = batch_pairs(sift)
    geo = geometry(sift, [kg.F] * 3, 52)
    for md in (0.0, cap):
        got = run_batched(sift, m, gate, pairs, k, geo, lists=md)
        for i, p in enumerate(pairs):
            e = cv.knn_records(*kg.mirror(gate, p.q, p.t, p.q_xy, p.t_xy, k), max_distance=md, img_idx=i)
            assert same(got[i], e), (gate, md, i)
        assert len(got[2]) == 0
    # nq == 0: nothing written, count 0
    empty = Pair(sift, big.q[:0], big.t[:5], big.q_xy[:0], big.t_xy[:5])
    assert len(gated_list(sift, m, gate, empty, 3, 0.0)) == 0


def test_detector_buffers(sift):
    """Two frames of a small detector, kpts3 passed as the positions with stride 3: the sidecar route equals the route
    after set_sidecars(off), and both the mirror on the host copies."""
    w, h, radius, max_error = 320, 240, 60.0, 2.0
    F = np.float32([[0, 0, 0], [0, 0, -1], [0, 1, 0]])  # a rectified pair: the band is |ty - qy| <= max_error sqrt(2)
    from sift_amd import cv

    det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h, upscale=True, numFeatures=0), lanes=1)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(sift.synth_frame(1, w, h))
    det.copyToHost(True)
    n0 = det.total_size
    k0, d0 = det.final_kpts.copy(), det.descriptors.astype(np.float32).reshape(n0, 128)
    prev_xy = sift.DeviceArray(n0 * 12)
    sift._check(sift.lib().sift_hip_memcpy_d2d(prev_xy.value, det.device_kpts.data(), n0 * 12, None), "d2d")
    det.detectAndCompute(sift.synth_frame(2, w, h))
    det.copyToHost(True)
    n1 = det.total_size
    k1, d1 = det.final_kpts.copy(), det.descriptors.astype(np.float32).reshape(n1, 128)
    assert n0 > 100 and n1 > 100 and det.prev_size == n0
    qd, td = det.prev_descriptor, det.device_descriptor
    k, cap = 5, max(n0, n1)
    refs = {"window": cv.guided_knn(d0, d1, k0, k1, radius, k),
            "band": cv.epipolar_knn(d0, d1, k0, k1, F, max_error, k, radius=radius)}
    counts = (refs["band"][0] >= 0).sum(1)
    assert (counts == 0).any() and (counts == k).any() and ((counts > 0) & (counts < k)).any()
    for sidecars in (True, False):
        m = sift.Matcher(cap, cap)
        m.set_sidecars(sidecars)
        gi, gd = tables(sift, n0, k)
        m.match_knn_guided_device(qd.data(), n0, td.data(), n1, prev_xy.value, det.device_kpts.data(), radius, k,
                                  gi.value, gd.value)
        assert same(read(gi, gd, n0, k), refs["window"]), sidecars
        gi, gd = tables(sift, n0, k)
        m.match_knn_epipolar_device(qd.data(), n0, td.data(), n1, prev_xy.value, det.device_kpts.data(), F, max_error, k,
                                    gi.value, gd.value, radius=radius)
        assert same(read(gi, gd, n0, k), refs["band"]), sidecars
    assert same(sift.knnMatchGuided(qd, n0, prev_xy.value, td, n1, det.device_kpts, radius, k), refs["window"])
    assert same(sift.knnMatchEpipolar(qd, n0, prev_xy.value, td, n1, det.device_kpts, F, max_error, k, radius),
                refs["band"])
    assert same([sift.matchKnnListGuided(qd, n0, prev_xy.value, td, n1, det.device_kpts, radius, k, 250.0)],
                [cv.knn_records(*refs["window"], max_distance=250.0)])
    assert same([sift.matchKnnListEpipolar(qd, n0, prev_xy.value, td, n1, det.device_kpts, F, max_error, k, 250.0,
                                           radius)], [cv.knn_records(*refs["band"], max_distance=250.0)])


def test_chain_without_read_back(sift):
    """match_list_device -> verify_device -> match_knn_list_epipolar_batched (P = 1, geometry = the result record on
    the device) -> verify_device on the k-NN list, all on one stream."""
    import torch

    import epipolar_cases as ec
    from sift_amd import cv

    q, t, q_xy, t_xy = ec.case(65, 64)[:4]
    nq, nt, K, k = len(q), len(t), 256, 3
    dq, dt = upload(sift, q), upload(sift, t)
    dqxy, dtxy = dev(sift, ec.with_stride(q_xy, 3)), dev(sift, ec.with_stride(t_xy, 3))
    cap = max(nq, nt)
    m, v = sift.Matcher(cap, cap, 2), sift.Verifier(nq * k, K)
    lst, cnt = dev(sift, np.full(4 * nq * k, FILL, np.int32)), dev(sift, np.full(1, FILL, np.int32))
    res, res2 = dev(sift, np.full(52, 0xCD, np.uint8)), dev(sift, np.full(52, 0xCD, np.uint8))
    inl, icnt = dev(sift, np.full(4 * nq * k, FILL, np.int32)), dev(sift, np.full(1, FILL, np.int32))
    klst, kcnt = dev(sift, np.full(4 * nq * k, FILL, np.int32)), dev(sift, np.full(1, FILL, np.int32))
    inl2, icnt2 = dev(sift, np.full(4 * nq * k, FILL, np.int32)), dev(sift, np.full(1, FILL, np.int32))
    mask = dev(sift, np.full(nq * k, 0xCD, np.uint8))
    # the first list and the first k-NN call allocate their scratch: not on the stream under test
    m.match_list_device(dq.value, nq, dt.value, nt, lst.value, cnt.value)
    m.match_knn_list_epipolar_batched([dq.value], [nq], [dt.value], [nt], [(dqxy.value, dtxy.value)], res.value,
                                      ec.MAX_ERROR, k, klst.value, kcnt.value)
    sift.lib().sift_hip_device_sync()
    s = torch.cuda.Stream()
    st = s.cuda_stream
    m.match_list_device(dq.value, nq, dt.value, nt, lst.value, cnt.value, stream=st)
    v.verify_device(lst.value, cnt.value, nq, dqxy.value, nq, dtxy.value, nt, res.value, inl.value, icnt.value,
                    mask.value, ec.MAX_ERROR, K, 0, 3, 3, stream=st)
    m.match_knn_list_epipolar_batched([dq.value], [nq], [dt.value], [nt], [(dqxy.value, dtxy.value)], res.value,
                                      ec.MAX_ERROR, k, klst.value, kcnt.value, stream=st)
    v.verify_device(klst.value, kcnt.value, nq * k, dqxy.value, nq, dtxy.value, nt, res2.value, inl2.value, icnt2.value,
                    mask.value, ec.MAX_ERROR, K, 0, 3, 3, stream=st)
    s.synchronize()
    r = res.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0]
    assert r["hypothesis"] >= 0 and cv.geometry_usable(r["F"])
    n = int(kcnt.to_numpy(np.int32, (1,))[0])
    recs = klst.to_numpy(sift.DMATCH_DTYPE, (nq * k,))[:n]
    exp = cv.knn_records(*cv.epipolar_knn(q, t, q_xy, t_xy, r["F"], ec.MAX_ERROR, k))
    assert n > 0 and same(recs, exp)
    assert (np.bincount(recs["queryIdx"]) > 1).any()  # some query keeps several candidates inside its band
    r2 = res2.to_numpy(sift.VERIFY_RESULT_DTYPE, (1,))[0]
    n2 = int(icnt2.to_numpy(np.int32, (1,))[0])
    assert r2["hypothesis"] >= 0 and r2["matches"] == n and 0 < n2 == r2["inliers"] <= n
    have = {x.tobytes() for x in recs}
    assert all(x.tobytes() in have for x in inl2.to_numpy(sift.DMATCH_DTYPE, (nq * k,))[:n2])


def test_other_calls_keep_their_bytes(sift, big):
    """The gated k-NN calls restore the counters they use: the other match calls return their usual bytes after."""
    m, fresh = sift.Matcher(1100, 1100, 3), sift.Matcher(1100, 1100, 3)
    qp, tp, qxy, txy = big.ptrs()

    def others(mm):
        i2, e2 = tables(sift, big.nq, 2)
        mm.match_guided_device(qp, big.nq, tp, big.nt, qxy, txy, kg.RADIUS, 2, 2, idx2_ptr=i2.value, d2_ptr=e2.value)
        return [top2(sift, mm, qp, big.nq, tp, big.nt), knn_dev(sift, mm, qp, big.nq, tp, big.nt, 8),
                read(i2, e2, big.nq, 2)]

    for gate in kg.GATES:
        gated(sift, m, gate, big, 8)
        gated_list(sift, m, gate, big, 3, 0.0)
    run_batched(sift, m, "band", batch_pairs(sift), 5, geometry(sift, [kg.F] * 3, 52))
    a, b = others(m), others(fresh)
    for x, y in zip(a, b):
        assert same(x, y)
    assert same(a[1], kc.reference(*kc.BIG, 8))


def test_refusals_launch_nothing(sift):
    L = sift.lib()
    p = Pair(sift, *kc.sets(33, 31), *kg.positions(33, 31))
    m = sift.Matcher(40, 40, 2)
    idx, d2 = tables(sift, 64, 8)
    out = dev(sift, np.full(4 * 64 * 8, FILL, np.int32))
    cnt = dev(sift, np.full(2, FILL, np.int32))
    h = m._m
    qp, tp, qxy, txy = p.ptrs()
    g = sift._MatchGate(qxy, 2, txy, 2, kg.RADIUS)
    e = sift._epipolar_gate(qxy, 2, txy, 2, INF, kg.F, kg.MAX_ERROR)
    gnull = sift._MatchGate(None, 2, txy, 2, kg.RADIUS)
    G, E = ctypes.byref(g), ctypes.byref(e)
    three, big3 = (ctypes.c_int * 3)(33, 33, 33), (ctypes.c_int * 3)(41, 33, 33)
    ptrs = (ctypes.c_void_p * 3)(qp, qp, qp)
    pos = (sift._MatchPositions * 3)(*[sift._MatchPositions(qxy, qxy)] * 3)
    geo = dev(sift, np.tile(kg.F.reshape(-1), 3))
    bad = [
        L.sift_hip_match_knn_guided_device(h, qp, 41, tp, 31, G, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_guided_device(h, qp, 33, tp, 41, G, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_guided_device(h, None, 33, tp, 31, G, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_guided_device(h, qp, 33, tp, 31, ctypes.byref(gnull), 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_epipolar_device(h, qp, 41, tp, 31, E, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_epipolar_device(h, qp, 33, None, 31, E, 2, idx.value, d2.value, None),
        L.sift_hip_match_knn_guided_batched(h, 3, ptrs, three, ptrs, three, pos, 2, 2, kg.RADIUS, 2, idx.value, d2.value,
                                            None),
        L.sift_hip_match_knn_guided_batched(h, 0, ptrs, three, ptrs, three, pos, 2, 2, kg.RADIUS, 2, idx.value, d2.value,
                                            None),
        L.sift_hip_match_knn_guided_batched(h, 2, ptrs, big3, ptrs, three, pos, 2, 2, kg.RADIUS, 2, idx.value, d2.value,
                                            None),
        L.sift_hip_match_knn_epipolar_batched(h, 2, ptrs, big3, ptrs, three, pos, 2, 2, INF, geo.value, 36, 2.0, 2,
                                              idx.value, d2.value, None),
        L.sift_hip_match_knn_epipolar_batched(h, 2, ptrs, three, ptrs, three, None, 2, 2, INF, geo.value, 36, 2.0, 2,
                                              idx.value, d2.value, None),
        L.sift_hip_match_knn_list_guided_device(h, qp, 33, tp, 31, G, 2, 1.0, None, cnt.value, None),
        L.sift_hip_match_knn_list_guided_device(h, qp, 33, tp, 31, G, 2, 1.0, out.value, None, None),
        L.sift_hip_match_knn_list_epipolar_device(h, qp, 33, tp, 31, E, 2, 1.0, out.value, None, None),
        L.sift_hip_match_knn_list_guided_batched(h, 2, ptrs, three, ptrs, three, pos, 2, 2, kg.RADIUS, 2, 1.0, None,
                                                 cnt.value, None),
        L.sift_hip_match_knn_list_epipolar_batched(h, 2, ptrs, three, ptrs, three, pos, 2, 2, INF, geo.value, 36, 2.0, 2,
                                                   1.0, out.value, None, None),
        L.sift_hip_match_knn_list_epipolar_batched(h, 2, ptrs, three, ptrs, three, pos, 2, 2, INF, geo.value, 34, 2.0, 2,
                                                   1.0, out.value, cnt.value, None),
    ]
    assert bad == [-1] * len(bad), bad
    assert L.sift_hip_last_error()
    L.sift_hip_device_sync()
    assert (idx.to_numpy(np.int32, (64 * 8,)) == FILL).all() and (d2.to_numpy(np.float32, (64 * 8,)) == FILL).all()
    assert (out.to_numpy(np.int32, (4 * 64 * 8,)) == FILL).all() and (cnt.to_numpy(np.int32, (2,)) == FILL).all()
    with pytest.raises(sift.SiftHipError):
        m.match_knn_guided_device(qp, 33, tp, 31, qxy, txy, kg.RADIUS, 9, idx.value, d2.value, q_stride=2, t_stride=2)
    # nq == 0: nothing is written
    m.match_knn_guided_device(0, 0, tp, 5, 0, txy, kg.RADIUS, 3, idx.value, d2.value, q_stride=2, t_stride=2)
    L.sift_hip_device_sync()
    assert (idx.to_numpy(np.int32, (64 * 8,)) == FILL).all()
