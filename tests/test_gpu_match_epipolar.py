"""The epipolar gate on the GPU (sift_hip_match_epipolar_*, k_match_epipolar): top-2 and match lists inside the band
round each query's epipolar line.

The bar: idx2, d2 and match from the device equal sift_amd.cv.epipolar_top2 (the rule of include/sift_hip.h in numpy
float32, exact integer distances) as raw bytes, for every query; lists equal sift_amd.cv.filter_matches applied to the
epipolar top-2 of both directions (the reverse under F transposed), byte for byte.  The inputs are
tests/epipolar_cases.py; tests/test_match_epipolar_abi.py checks on the CPU that they exercise the gate and that the
reference with every row a candidate is the CPU oracle.
"""
import ctypes

import numpy as np
import pytest

import epipolar_cases as ec

pytestmark = pytest.mark.gpu
INF = float("inf")


class Ptr:
    """A device pointer the detector owns, with the .value of a DeviceArray."""

    def __init__(self, value):
        self.value = value


def upload(sift, rows):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(rows.astype(np.float16)).view(np.uint16))


def upload_xy(sift, xy, stride=2):
    """Exactly len(xy) rows of `stride` floats: nothing lies behind the last row."""
    return sift.DeviceArray.from_numpy(ec.with_stride(xy, stride))


def epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, max_error, radius=INF, q_stride=2, t_stride=2, with_match=False):
    """idx2 / d2 (and match) of match_epipolar_device; the outputs start as a pattern the kernel has to overwrite."""
    idx2 = sift.DeviceArray.from_numpy(np.full(2 * max(nq, 1), -77, np.int32))
    d2 = sift.DeviceArray.from_numpy(np.full(2 * max(nq, 1), -77, np.float32))
    mt = sift.DeviceArray.from_numpy(np.full(max(nq, 1), -77, np.int32))
    m.match_epipolar_device(dq.value, nq, dt.value, nt, dqxy.value, dtxy.value, F, max_error, radius, q_stride, t_stride,
                            0.8, False, idx2.value, d2.value, mt.value)
    out = idx2.to_numpy(np.int32, (max(nq, 1), 2))[:nq], d2.to_numpy(np.float32, (max(nq, 1), 2))[:nq]
    return out + (mt.to_numpy(np.int32, (max(nq, 1),))[:nq],) if with_match else out


def ungated(sift, m, dq, nq, dt, nt):
    idx2, d2 = sift.DeviceArray(nq * 8), sift.DeviceArray(nq * 8)
    m.match_device(dq.value, nq, dt.value, nt, 0.8, False, idx2.value, d2.value, 0)
    return idx2.to_numpy(np.int32, (nq, 2)), d2.to_numpy(np.float32, (nq, 2))


def run_list(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, max_error, radius=INF, **f):
    out = sift.DeviceArray.from_numpy(np.full(4 * max(nq, 1), -1, np.int32))
    cnt = sift.DeviceArray.from_numpy(np.full(1, -1, np.int32))
    m.match_list_epipolar_device(dq.value, nq, dt.value, nt, dqxy.value, dtxy.value, F, max_error, out.value, cnt.value,
                                 radius, 2, 2, **f)
    n = int(cnt.to_numpy(np.int32, (1,))[0])
    assert 0 <= n <= nq, n
    return out.to_numpy(sift.DMATCH_DTYPE, (max(nq, 1),))[:n]


def same(got, ref):
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, ref))


def ratio_match(idx2, d2):
    """The `match` output (ratio 0.8 on distances) from a top-2."""
    from sift_amd import cv

    return np.where(cv._ratio_pass(idx2, d2, 0.8, False), idx2[:, 0], -1).astype(np.int32)


@pytest.mark.parametrize("nq,nt", ec.SHAPES)
def test_shapes(sift, nq, nt):
    q, t, q_xy, t_xy, F, fwd, rev, _ = ec.case(nq, nt)
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    cap = max(nq, nt)
    m = sift.Matcher(cap, cap)
    gi, gd, gm = epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR, with_match=True)
    print(f"{nq} x {nt}: {np.sum(fwd[0][:, 0] >= 0)} queries with a candidate, {np.sum(fwd[0][:, 1] >= 0)} with two, "
          f"S = {sift.Matcher.guided_plan(nq, nt)}")
    assert same((gi, gd), fwd), (nq, nt, np.flatnonzero((gi != fwd[0]).any(1))[:8])
    assert np.array_equal(gm, ratio_match(*fwd))  # one candidate matches it, none gives -1
    # the roles swapped, F transposed
    assert same(epipolar(sift, m, dt, nt, dq, nq, dtxy, dqxy, F.T, ec.MAX_ERROR), rev), (nt, nq)
    if nq >= 31 and nt >= 31:  # a kernel that ignores F cannot pass
        ui, _ = ungated(sift, m, dq, nq, dt, nt)
        has = fwd[0][:, 0] >= 0
        assert (fwd[0][has, 0] != ui[has, 0]).mean() > 0.5
    if (nq, nt) == (600, 1100):
        assert sift.Matcher.guided_plan(nq, nt) > 1 and sift.Matcher.guided_plan(nt, nq) > 1  # the split merge


def test_hand_case_inclusive_edge(sift):
    """r r == e2 (nq + nr) exactly for train row 0: a candidate.  The three rows' descriptors are at distances 3, 1, 2
    of the query's, so the top-2 shows which rows passed: rows 0 and 2, the nearer first."""
    from sift_amd import cv

    h = ec.HAND
    q = np.zeros((1, 128), np.float32)
    t = np.zeros((3, 128), np.float32)
    t[:, 5] = [3, 1, 2]
    ref = cv.epipolar_top2(q, t, h["q_xy"], h["t_xy"], h["F"], h["max_error"])
    assert ref[0].tolist() == [[2, 0]] and ref[1].tolist() == [[4, 9]]
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, h["q_xy"]), upload_xy(sift, h["t_xy"])
    m = sift.Matcher(3, 3)
    assert same(epipolar(sift, m, dq, 1, dt, 3, dqxy, dtxy, h["F"], h["max_error"]), ref)
    # the general (fp16) path on the same edge: halves are exact there
    dqh, dth = upload(sift, q + 0.5), upload(sift, t + 0.5)
    got = epipolar(sift, m, dqh, 1, dth, 3, dqxy, dtxy, h["F"], h["max_error"])
    assert same(got, ref)
    rref = cv.epipolar_top2(t, q, h["t_xy"], h["q_xy"], h["F"].T, h["max_error"])
    assert rref[0].tolist() == [[0, -1], [-1, -1], [0, -1]]
    assert same(epipolar(sift, m, dt, 3, dq, 1, dtxy, dqxy, h["F"].T, h["max_error"]), rref)


@pytest.mark.parametrize("nq,nt", [(33, 31), (257, 300), (600, 1100)])
def test_every_row_a_candidate_is_match_device(sift, nq, nt):
    q, t, q_xy, t_xy, F, _, _, _ = ec.case(nq, nt)
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    m = sift.Matcher(nq, nt)
    assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, 1e30), ungated(sift, m, dq, nq, dt, nt))
    if (nq, nt) == (257, 300):
        # Both sets halved (every product and sum stays exact in fp32): the epipolar and the ungated instantiation of
        # the one fp16 block, two splits and a second 32-query block, byte for byte.
        dq, dt = upload(sift, q * 0.5), upload(sift, t * 0.5)
        assert sift.Matcher.guided_plan(nq, nt) == 2
        ref = ungated(sift, m, dq, nq, dt, nt)
        assert np.any(ref[1] != np.rint(ref[1]))  # fractional distances: not the integer path
        assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, 1e30), ref)


def test_band_and_window(sift):
    """A finite radius: the band ANDed with the window, on the integer path and on the fp16 path, both directions and
    the list."""
    from sift_amd import cv

    nq, nt, radius = 257, 300, 40.0
    q, t, q_xy, t_xy, F, fwd, _, _ = ec.case(nq, nt)
    ref = cv.epipolar_top2(q, t, q_xy, t_xy, F, ec.MAX_ERROR, radius)
    rref = cv.epipolar_top2(t, q, t_xy, q_xy, F.T, ec.MAX_ERROR, radius)
    n_band, n_both = (fwd[0] >= 0).sum(), (ref[0] >= 0).sum()
    assert 0 < n_both < n_band and not same(ref, fwd)  # the window removes candidates of the band, not all of them
    assert not same(ref, cv.guided_top2(q, t, q_xy, t_xy, radius))  # and the band candidates of the window
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    m = sift.Matcher(nt, nt)
    assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR, radius), ref)
    assert same(epipolar(sift, m, dt, nt, dq, nq, dtxy, dqxy, F.T, ec.MAX_ERROR, radius), rref)
    assert same([run_list(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR, radius)], [cv.filter_matches(*ref, *rref)])
    dqh, dth = upload(sift, q * 0.5), upload(sift, t * 0.5)
    href = cv.epipolar_top2(q * 0.5, t * 0.5, q_xy, t_xy, F, ec.MAX_ERROR, radius)
    assert same(epipolar(sift, m, dqh, nq, dth, nt, dqxy, dtxy, F, ec.MAX_ERROR, radius), href)


def test_ties(sift):
    """Descriptors from {0, 1} on 4 of the 128 dimensions, as test_gpu_match_list.test_ties: 16 distinct rows among
    300 on each side and about 10 candidates per query, so nearly every guided top-2 is a tie among candidates."""
    from sift_amd import cv

    rng = np.random.default_rng(5)
    n, max_error = 300, 2.5
    q, t = np.zeros((n, 128), np.float32), np.zeros((n, 128), np.float32)
    dims = [3, 40, 77, 126]
    q[:, dims] = rng.integers(0, 2, (n, 4))
    t[:, dims] = rng.integers(0, 2, (n, 4))
    q_xy = (rng.integers(0, 800, (n, 2)) * 0.25).astype(np.float32)
    t_xy = (rng.integers(0, 800, (n, 2)) * 0.25).astype(np.float32)
    F = ec.fundamental()
    assert 6 < cv.epipolar_mask(q_xy, t_xy, F, max_error).sum(1).mean() < 14
    ref, rref = cv.epipolar_top2(q, t, q_xy, t_xy, F, max_error), cv.epipolar_top2(t, q, t_xy, q_xy, F.T, max_error)
    both = ref[0][:, 1] >= 0
    assert (ref[1][both, 0] == ref[1][both, 1]).mean() > 0.4  # exact ties among the candidates
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    m = sift.Matcher(n, n)
    assert same(epipolar(sift, m, dq, n, dt, n, dqxy, dtxy, F, max_error), ref)
    for f in (dict(ratio=0.0), dict(ratio=0.0, cross_check=False), dict()):
        assert same([run_list(sift, m, dq, n, dt, n, dqxy, dtxy, F, max_error, **f)],
                    [cv.filter_matches(*ref, *rref, **f)]), f


def test_strides_and_exact_size_position_arrays(sift):
    """Stride 2, 3 and 5 arrays of the same points give the same bytes; the arrays hold exactly n rows (the extra
    columns are NaN), with nt = 257 one row into a second key group and nq = 33 into a second 32-query block: no row
    past the end is needed for a correct result."""
    from sift_amd import cv

    nq, nt = 33, 257
    q, t, q_xy, t_xy, _ = ec.make_epipolar(nq, nt, seed=3)
    F = ec.fundamental()
    ref = cv.epipolar_top2(q, t, q_xy, t_xy, F, ec.MAX_ERROR)
    rref = cv.epipolar_top2(t, q, t_xy, q_xy, F.T, ec.MAX_ERROR)
    assert (ref[0][:, 0] >= 0).sum() > 5
    dq, dt = upload(sift, q), upload(sift, t)
    m = sift.Matcher(nt, nt)
    for qs, ts in ((2, 2), (3, 3), (2, 3), (5, 2)):
        dqxy, dtxy = upload_xy(sift, q_xy, qs), upload_xy(sift, t_xy, ts)
        assert dqxy.nbytes == nq * qs * 4 and dtxy.nbytes == nt * ts * 4
        assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR, INF, qs, ts), ref), (qs, ts)
        assert same(epipolar(sift, m, dt, nt, dq, nq, dtxy, dqxy, F.T, ec.MAX_ERROR, INF, ts, qs), rref), (ts, qs)


def test_nan_positions(sift):
    from sift_amd import cv

    nq, nt = 257, 300
    q, t, q_xy, t_xy, F, fwd, _, _ = ec.case(nq, nt)
    q_xy, t_xy = q_xy.copy(), t_xy.copy()
    with_cand = np.flatnonzero(fwd[0][:, 0] >= 0)
    qbad = with_cand[:6]
    q_xy[qbad[:3], 0] = np.nan
    q_xy[qbad[3:], 1] = np.nan
    tbad = np.unique(fwd[0][with_cand[6:30], 0])[:8]  # train rows that are somebody's guided best
    t_xy[tbad[:4], 0] = np.nan
    t_xy[tbad[4:], 1] = np.nan
    ref = cv.epipolar_top2(q, t, q_xy, t_xy, F, ec.MAX_ERROR)
    assert np.all(ref[0][qbad] == -1) and not np.isin(ref[0], tbad).any() and (ref[0][:, 0] >= 0).sum() > 20
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    m = sift.Matcher(nt, nt)
    got = epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR)
    assert same(got, ref)
    assert np.all(got[0][qbad] == -1) and np.all(got[1][qbad] == ec.FLT_MAX) and not np.isin(got[0], tbad).any()
    # with every finite row a candidate the NaN rows still are candidates of nothing, on both paths
    wide = cv.epipolar_top2(q, t, q_xy, t_xy, F, 1e30)
    assert np.all(wide[0][qbad] == -1) and not np.isin(wide[0], tbad).any()
    assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, 1e30), wide)
    dqh, dth = upload(sift, q * 0.5), upload(sift, t * 0.5)
    assert same(epipolar(sift, m, dqh, nq, dth, nt, dqxy, dtxy, F, ec.MAX_ERROR),
                cv.epipolar_top2(q * 0.5, t * 0.5, q_xy, t_xy, F, ec.MAX_ERROR))


@pytest.mark.parametrize("sides", ["query", "train", "both"])
def test_non_integer_sets(sift, sides):
    """Multiples of 0.5 in 0..127.5 on one side or both: the pair takes the gated fp16 path.  Every product, norm and
    fp32 sum is then a multiple of 0.25 below 2^24 quarter units, so the float64 reference is exact too."""
    from sift_amd import cv

    nq, nt = 257, 300
    q, t, q_xy, t_xy, F, fwd, _, _ = ec.case(nq, nt)
    if sides in ("query", "both"):
        q = q * 0.5
    if sides in ("train", "both"):
        t = t * 0.5
    for a in ((q,) if sides == "query" else (t,) if sides == "train" else (q, t)):
        assert a.max() <= 127.5 and np.any(a != np.rint(a)) and np.all(2 * a == np.rint(2 * a))
    ref = cv.epipolar_top2(q, t, q_xy, t_xy, F, ec.MAX_ERROR)
    rref = cv.epipolar_top2(t, q, t_xy, q_xy, F.T, ec.MAX_ERROR)
    assert np.array_equal(ref[0] >= 0, fwd[0] >= 0)
    assert np.any(ref[1][ref[0] >= 0] != np.rint(ref[1][ref[0] >= 0]))  # fractional distances: not the integer path
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    m = sift.Matcher(nt, nt)
    assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR), ref)
    assert same(epipolar(sift, m, dt, nt, dq, nq, dtxy, dqxy, F.T, ec.MAX_ERROR), rref)
    assert same([run_list(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR)], [cv.filter_matches(*ref, *rref)])


def test_detector_buffers(sift):
    """prev_descriptor x device_descriptor of two 320 x 240 frames with the device_kpts of both frames as the
    positions (stride 3), under the F of a rectified pair (x_t^T F x_q = ty - qy: the band is |ty - qy| <= max_error
    sqrt(2)) and a finite radius along the line; on the sidecar codes and with the sidecars off: both equal the
    reference computed from the host copies."""
    from sift_amd import cv

    w, h, radius, max_error = 320, 240, 60.0, 2.0
    F = np.float32([[0, 0, 0], [0, 0, -1], [0, 1, 0]])
    det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h, upscale=True, numFeatures=0), lanes=1)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(sift.synth_frame(1, w, h))
    det.copyToHost(True)
    n0 = det.total_size
    k0, d0 = det.final_kpts.copy(), det.descriptors.astype(np.float32).reshape(n0, 128)
    prev_xy = sift.DeviceArray(n0 * 12)  # the previous frame's positions, copied before the next frame replaces them
    sift._check(sift.lib().sift_hip_memcpy_d2d(prev_xy.value, det.device_kpts.data(), n0 * 12, None), "d2d")
    det.detectAndCompute(sift.synth_frame(2, w, h))
    det.copyToHost(True)
    n1 = det.total_size
    k1, d1 = det.final_kpts.copy(), det.descriptors.astype(np.float32).reshape(n1, 128)
    assert n0 > 100 and n1 > 100 and det.prev_size == n0
    ref = cv.epipolar_top2(d0, d1, k0, k1, F, max_error, radius)
    rref = cv.epipolar_top2(d1, d0, k1, k0, F.T, max_error, radius)
    ncand = cv.epipolar_mask(k0, k1, F, max_error, radius).sum(1)
    assert (ncand == 0).any() and (ncand >= 2).any()
    assert not same(ref, cv.guided_top2(d0, d1, k0, k1, radius))  # the band, not only the window
    qd, td = det.prev_descriptor, det.device_descriptor
    cap = max(n0, n1)
    lists = []
    for sidecars in (True, False):
        m = sift.Matcher(cap, cap)
        m.set_sidecars(sidecars)
        assert same(epipolar(sift, m, Ptr(qd.data()), n0, Ptr(td.data()), n1, prev_xy, Ptr(det.device_kpts.data()), F,
                             max_error, radius, 3, 3), ref), sidecars
        out = sift.DeviceArray.from_numpy(np.full(4 * n0, -1, np.int32))
        cnt = sift.DeviceArray.from_numpy(np.full(1, -1, np.int32))
        m.match_list_epipolar_device(qd.data(), n0, td.data(), n1, prev_xy.value, det.device_kpts.data(), F, max_error,
                                     out.value, cnt.value, radius)
        n = int(cnt.to_numpy(np.int32, (1,))[0])
        lists.append(out.to_numpy(sift.DMATCH_DTYPE, (n0,))[:n])
    expect = cv.filter_matches(*ref, *rref)
    assert 0 < len(expect) < n0
    assert same(lists, [expect, expect])
    assert same([sift.matchListEpipolar(qd, n0, prev_xy.value, td, n1, det.device_kpts, F, max_error, radius)], [expect])


@pytest.mark.parametrize("nq,nt", [(257, 300), (600, 1100)])
def test_lists(sift, nq, nt):
    from sift_amd import cv

    q, t, q_xy, t_xy, F, fwd, rev, _ = ec.case(nq, nt)
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    cap = max(nq, nt)
    m = sift.Matcher(cap, cap)
    for f in (dict(), dict(cross_check=False), dict(ratio_both_ways=True, max_distance=30.0)):
        ref = cv.filter_matches(*fwd, *rev, **f)
        print(f"{nq} x {nt} {f}: kept {len(ref)}")
        assert 0 < len(ref) < nq, (f, len(ref))
        assert same([run_list(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR, **f)], [ref]), f
        assert same([m.match_list_epipolar_host(dq.value, nq, dt.value, nt, dqxy.value, dtxy.value, F, ec.MAX_ERROR, INF,
                                                2, 2, **f)], [ref]), f
        ml = sift.matchListEpipolar(sift.DeviceBuffer(dq.value, nq * 128), nq, dqxy.value,
                                    sift.DeviceBuffer(dt.value, nt * 128), nt, sift.DeviceBuffer(dtxy.value, nt * 2), F,
                                    ec.MAX_ERROR, des_stride=2, src_stride=2, **f)
        assert same([ml], [ref]), f


def test_scratch_restored_after_a_split_call(sift, oracle):
    """After epipolar calls with S > 1 the matcher's merge scratch is idle again: match_device on the same matcher
    equals the CPU oracle, and a second epipolar call repeats the first."""
    nq, nt = 600, 1100
    q, t, q_xy, t_xy, F, fwd, _, _ = ec.case(nq, nt)
    assert sift.Matcher.guided_plan(nq, nt) > 1 and sift.Matcher.plan(nq, nt, 1)[0] > 1
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    m = sift.Matcher(nq, nt)
    assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR), fwd)
    oi, od = oracle.knn2(q, t)
    ui, ud = ungated(sift, m, dq, nq, dt, nt)
    assert np.array_equal(ui, oi) and np.array_equal(ud, np.rint(od.astype(np.float64) ** 2).astype(np.float32))
    assert same(epipolar(sift, m, dq, nq, dt, nt, dqxy, dtxy, F, ec.MAX_ERROR), fwd)


def test_argument_errors_and_empty_sets(sift):
    q, t, q_xy, t_xy, F, fwd, _, _ = ec.case(33, 31)
    dq, dt, dqxy, dtxy = upload(sift, q), upload(sift, t), upload_xy(sift, q_xy), upload_xy(sift, t_xy)
    L = sift.lib()
    m = sift.Matcher(33, 31)
    idx2 = sift.DeviceArray.from_numpy(np.full(66, -77, np.int32))
    d2 = sift.DeviceArray.from_numpy(np.full(66, -77, np.float32))
    nan = float("nan")

    def call(nq=33, nt=31, qxy=dqxy.value, txy=dtxy.value, qs=2, ts=2, radius=INF, dqp=dq.value, dtp=dt.value, f=F,
             max_error=ec.MAX_ERROR):
        g = sift._epipolar_gate(qxy, qs, txy, ts, radius, f, max_error)
        rc = L.sift_hip_match_epipolar_device(m._m, dqp, nq, dtp, nt, ctypes.byref(g), 0.8, 0, idx2.value, d2.value, None,
                                              None)
        return rc, L.sift_hip_last_error().decode()

    def untouched():
        sift._check(L.sift_hip_device_sync(), "sync")
        return np.all(idx2.to_numpy(np.int32, (66,)) == -77) and np.all(d2.to_numpy(np.float32, (66,)) == -77)

    bad_f = F.copy()
    bad_f[1, 1] = nan
    for kw, word in ((dict(nq=34), "limits"), (dict(nt=32), "limits"),  # over the matcher's limits
                     (dict(qxy=None), "position"), (dict(txy=None), "position"),  # a null position pointer
                     (dict(dqp=None), "descriptor"), (dict(dtp=None), "descriptor"),
                     (dict(qs=1), "stride"), (dict(ts=1), "stride"),
                     (dict(radius=0.0), "radius"), (dict(radius=nan), "radius"),
                     (dict(max_error=0.0), "max_error"), (dict(max_error=nan), "max_error"),
                     (dict(max_error=INF), "max_error"), (dict(f=bad_f), "F"), (dict(f=np.zeros(9)), "F")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    assert untouched()
    with pytest.raises(sift.SiftHipError):
        m.match_epipolar_device(dq.value, 33, dt.value, 31, dqxy.value, dtxy.value, F, -1.0, INF, 2, 2)
    # the reverse pair of a list does not fit this matcher (max_query 33 >= 31, but max_train 31 < 33)
    out, cnt = sift.DeviceArray.from_numpy(np.full(4 * 33, -1, np.int32)), sift.DeviceArray.from_numpy(np.full(1, -1, np.int32))
    with pytest.raises(sift.SiftHipError):
        m.match_list_epipolar_device(dq.value, 33, dt.value, 31, dqxy.value, dtxy.value, F, ec.MAX_ERROR, out.value,
                                     cnt.value, INF, 2, 2)
    m.match_list_epipolar_device(dq.value, 33, dt.value, 31, dqxy.value, dtxy.value, F, ec.MAX_ERROR, out.value, cnt.value,
                                 INF, 2, 2, cross_check=False)
    assert 0 < cnt.to_numpy(np.int32, (1,))[0] <= 33
    # nq == 0: the outputs are untouched; the empty train set may have null pointers: every query gets -1 / FLT_MAX
    assert call(nq=0, qxy=None, dqp=None)[0] == 0 and untouched()
    assert call(nt=0, txy=None, dtp=None)[0] == 0
    sift._check(L.sift_hip_device_sync(), "sync")
    assert np.all(idx2.to_numpy(np.int32, (66,)) == -1) and np.all(d2.to_numpy(np.float32, (66,)) == ec.FLT_MAX)
    big = sift.Matcher(40, 40)
    for nq, nt in ((0, 31), (33, 0)):
        big.match_list_epipolar_device(dq.value, nq, dt.value, nt, dqxy.value, dtxy.value, F, ec.MAX_ERROR, out.value,
                                       cnt.value, INF, 2, 2)
        assert cnt.to_numpy(np.int32, (1,))[0] == 0
    assert len(big.match_list_epipolar_host(dq.value, 0, dt.value, 31, dqxy.value, dtxy.value, F, ec.MAX_ERROR, INF, 2,
                                            2)) == 0
    assert len(sift.matchListEpipolar(sift.DeviceBuffer(dq.value, 0), 0, dqxy.value, sift.DeviceBuffer(dt.value, 0), 31,
                                      dtxy.value, F, ec.MAX_ERROR, INF, 2, 2)) == 0
    # the refused calls left the matcher usable
    assert same(epipolar(sift, m, dq, 33, dt, 31, dqxy, dtxy, F, ec.MAX_ERROR), fwd)
