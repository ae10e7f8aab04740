"""Match lists on the GPU (sift_hip_match_list_*, k_match_select): match -> filter -> ordered compaction.

The bar throughout: the records and the count equal sift_amd.cv.filter_matches (the rule of include/sift_hip.h in
numpy) applied to the idx2 / d2 that the existing Matcher.match_device returns for (Q, T) and for (T, Q) on the same
buffers, compared as raw bytes; for integer sets also the same filter applied to the CPU oracle's knn-2 of both
directions.

The oracle returns distances sqrtf(s) of exact integer sums s; the filter takes squared distances, recovered as
rint(dist^2) in float64 (exact while s < 2^22: the relative error of dist^2 is below 2^-23; the sets here stay below
2^20).
"""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 40), (40, 1), (33, 31), (257, 300), (300, 257), (1025, 1500), (2000, 2000)]
FLT_MAX = np.finfo(np.float32).max


def make_sets(nq, nt, seed=0):
    """Random integer descriptors (0..127 per dimension); half of the smaller set's size worth of train rows are
    copies of distinct query rows with per-copy noise of amplitude 1..8 (so a distance cap of 30 cuts some), at
    shuffled positions; an eighth of those query rows get a second query next to them (the reverse ratio test fails
    there and the cross check keeps one of the two).  The mutual list is neither empty nor full."""
    rng = np.random.default_rng(1000 * nq + nt + seed)
    q = rng.integers(0, 128, (nq, 128))
    t = rng.integers(0, 128, (nt, 128))
    k = min(nq, nt) // 2
    order = rng.permutation(nq)
    src, rest = order[:k], order[k:]
    dst = rng.permutation(nt)[:k]
    amp = rng.integers(1, 9, k)
    t[dst] = np.clip(q[src] + rng.integers(-amp[:, None], amp[:, None] + 1, (k, 128)), 0, 255)
    ndup = min(k // 8, len(rest))
    q[rest[:ndup]] = np.clip(q[src[:ndup]] + rng.integers(-2, 3, (ndup, 128)), 0, 255)
    return q.astype(np.float32), t.astype(np.float32)


def oracle_top2(oracle, q, t):
    idx, dist = oracle.knn2(q, t)
    d2 = np.rint(np.where(idx >= 0, dist, 0).astype(np.float64) ** 2).astype(np.float32)
    d2[idx < 0] = FLT_MAX
    return idx, d2


@functools.lru_cache(maxsize=None)
def case(nq, nt):
    """Host sets of a shape and the oracle's top-2 of both directions, computed once and shared."""
    import oracle_binding as oracle

    q, t = make_sets(nq, nt)
    for a in (q, t):
        a.setflags(write=False)
    return q, t, oracle_top2(oracle, q, t), oracle_top2(oracle, t, q)


def upload(sift, rows):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(rows.astype(np.float16)).view(np.uint16))


def top2(sift, m, qp, nq, tp, nt):
    """idx2 / d2 of the existing match_device."""
    idx2, d2 = sift.DeviceArray(nq * 8), sift.DeviceArray(nq * 8)
    m.match_device(qp, nq, tp, nt, 0.8, False, idx2.value, d2.value, 0)
    return idx2.to_numpy(np.int32, (nq, 2)), d2.to_numpy(np.float32, (nq, 2))


def both_top2(sift, m, qp, nq, tp, nt):
    return top2(sift, m, qp, nq, tp, nt) + top2(sift, m, tp, nt, qp, nq)


def run_list(sift, m, qp, nq, tp, nt, **f):
    """The records a list call returns (the first `count` rows of its output)."""
    out = sift.DeviceArray.from_numpy(np.full(4 * max(nq, 1), -1, np.int32))
    cnt = sift.DeviceArray.from_numpy(np.full(1, -1, np.int32))
    m.match_list_device(qp, nq, tp, nt, out.value, cnt.value, **f)
    n = int(cnt.to_numpy(np.int32, (1,))[0])
    assert 0 <= n <= nq, n
    return out.to_numpy(sift.DMATCH_DTYPE, (max(nq, 1),))[:n]


def same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nq,nt", SHAPES)
def test_shapes(sift, nq, nt):
    from sift_amd import cv

    q, t, ofwd, orev = case(nq, nt)
    dq, dt = upload(sift, q), upload(sift, t)
    cap = max(nq, nt)
    mref = sift.Matcher(cap, cap)
    tops = both_top2(sift, mref, dq.value, nq, dt.value, nt)
    for a, b in zip(tops, ofwd + orev):  # the premise: the existing matcher equals the oracle on these sets
        assert np.array_equal(a, b), (nq, nt)
    for f in (dict(), dict(cross_check=False), dict(ratio=0.0), dict(ratio_both_ways=True, max_distance=30.0)):
        ref = cv.filter_matches(*tops, **f)
        oref = cv.filter_matches(*ofwd, *orev, **f)
        print(f"{nq} x {nt} {f}: kept {len(ref)}")
        assert same(ref, oref), (nq, nt, f)
        if nq > 1 and nt > 1:
            assert 0 < len(ref) < nq, (nq, nt, f, len(ref))
        for pairs in (1, 2):  # two launches / one two-pair launch
            got = run_list(sift, sift.Matcher(cap, cap, max_pairs=pairs), dq.value, nq, dt.value, nt, **f)
            assert same(got, ref), (nq, nt, f, pairs, len(got), len(ref))
    if nq == 2000:  # the shapes above take more than one 1024-query chunk of the select kernel; this one a split plan
        assert sift.Matcher.plan(nq, nt, 1)[0] > 1 and sift.Matcher.plan(nq, nt, 2)[0] > 1


def test_ties(sift, oracle):
    """Descriptors from {0, 1} on 4 of the 128 dimensions: 16 distinct rows among 300 on each side, so every top-2
    is a tie -- the lower-index rule of both directions and d1 == d2 in the ratio test."""
    from sift_amd import cv

    rng = np.random.default_rng(5)
    n = 300
    q, t = np.zeros((n, 128), np.float32), np.zeros((n, 128), np.float32)
    dims = [3, 40, 77, 126]
    q[:, dims] = rng.integers(0, 2, (n, 4))
    t[:, dims] = rng.integers(0, 2, (n, 4))
    dq, dt = upload(sift, q), upload(sift, t)
    tops = both_top2(sift, sift.Matcher(n, n), dq.value, n, dt.value, n)
    otops = oracle_top2(oracle, q, t) + oracle_top2(oracle, t, q)
    for a, b in zip(tops, otops):
        assert np.array_equal(a, b)
    assert (tops[1][:, 0] == tops[1][:, 1]).mean() > 0.9  # exact ties nearly everywhere
    kept = {}
    for f in (dict(ratio=0.0), dict(ratio=0.0, cross_check=False), dict(), dict(ratio=1.0, ratio_on_squared=True),
              dict(ratio=0.0, ratio_both_ways=True), dict(ratio=0.0, max_distance=0.5)):
        ref = cv.filter_matches(*tops, **f)
        assert same(ref, cv.filter_matches(*otops, **f)), f
        for pairs in (1, 2):
            assert same(run_list(sift, sift.Matcher(n, n, max_pairs=pairs), dq.value, n, dt.value, n, **f), ref), (f, pairs)
        kept[tuple(f.items())] = len(ref)
    # the mutual list names the first row of each of the (at most 16) distinct values present on both sides
    assert 0 < kept[(("ratio", 0.0),)] <= 16 and kept[(("ratio", 0.0), ("cross_check", False))] == n


def test_every_filter_combination(sift):
    from sift_amd import cv

    nq, nt = 257, 300
    q, t, ofwd, orev = case(nq, nt)
    dq, dt = upload(sift, q), upload(sift, t)
    tops = both_top2(sift, sift.Matcher(nt, nt), dq.value, nq, dt.value, nt)
    m1, m2 = sift.Matcher(nt, nt, max_pairs=1), sift.Matcher(nt, nt, max_pairs=2)
    counts = set()
    for ratio, squared, maxd, cross, both in itertools.product((0.0, 0.8), (False, True), (0.0, 30.0), (False, True),
                                                               (False, True)):
        f = dict(ratio=ratio, ratio_on_squared=squared, max_distance=maxd, cross_check=cross, ratio_both_ways=both)
        ref = cv.filter_matches(*tops, **f)
        assert same(ref, cv.filter_matches(*ofwd, *orev, **f)), f
        for m in (m1, m2):
            assert same(run_list(sift, m, dq.value, nq, dt.value, nt, **f), ref), f
        counts.add(len(ref))
    assert len(counts) >= 6  # the options do change the list


def test_general_fp16_path(sift):
    """Sets holding non-integer fp16 values take the general path (float d2); the list consumes its top-2 as it is."""
    from sift_amd import cv

    nq, nt = 257, 300
    q, t, _, _ = case(nq, nt)
    q, t = q * 0.5 + 0.25, t * 0.5 + 0.25  # exact in fp16, no integers
    dq, dt = upload(sift, q), upload(sift, t)
    tops = both_top2(sift, sift.Matcher(nt, nt), dq.value, nq, dt.value, nt)
    assert np.any(tops[1][:, 0] != np.rint(tops[1][:, 0]))
    for f in (dict(), dict(ratio_both_ways=True, max_distance=15.0), dict(ratio=0.0)):
        ref = cv.filter_matches(*tops, **f)
        assert 0 < len(ref) < nq
        for pairs in (1, 2):
            assert same(run_list(sift, sift.Matcher(nt, nt, max_pairs=pairs), dq.value, nq, dt.value, nt, **f), ref), (f, pairs)
    # one integer set against one general set
    di = upload(sift, case(nq, nt)[0])
    tops = both_top2(sift, sift.Matcher(nt, nt), di.value, nq, dt.value, nt)
    for pairs in (1, 2):
        assert same(run_list(sift, sift.Matcher(nt, nt, max_pairs=pairs), di.value, nq, dt.value, nt, ratio=0.0),
                    cv.filter_matches(*tops, ratio=0.0)), pairs


def test_batched_ragged_pairs_sharing_a_set(sift):
    from sift_amd import cv

    q, t, _, _ = case(257, 300)
    da, db = upload(sift, q), upload(sift, t)
    # db in all three, once as the query set; pair 1 queries rows 50 .. 169 of da
    pairs = [(da.value, 257, db.value, 300), (da.value + 50 * 256, 120, db.value, 257), (db.value, 300, da.value, 257)]
    mref = sift.Matcher(300, 300)
    f = dict(ratio=0.9, max_distance=60.0)
    refs = [cv.filter_matches(*both_top2(sift, mref, a, na, b, nb), img_idx=p, **f)
            for p, (a, na, b, nb) in enumerate(pairs)]
    assert all(0 < len(r) < pr[1] for r, pr in zip(refs, pairs))
    tot = sum(p[1] for p in pairs)
    results = []
    for maxp in (3, 6):  # two 3-pair launches / one 6-pair launch
        m = sift.Matcher(300, 300, max_pairs=maxp)
        out = sift.DeviceArray.from_numpy(np.full(4 * tot, -1, np.int32))
        cnt = sift.DeviceArray.from_numpy(np.full(3, -1, np.int32))
        m.match_list_batched([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs],
                             [p[3] for p in pairs], out.value, cnt.value, **f)
        counts = cnt.to_numpy(np.int32, (3,))
        recs = out.to_numpy(sift.DMATCH_DTYPE, (tot,))
        off = 0
        for p, (ref, pr) in enumerate(zip(refs, pairs)):
            assert counts[p] == len(ref), (maxp, p)
            assert same(recs[off: off + counts[p]], ref), (maxp, p)
            assert np.all(recs[off: off + counts[p]]["imgIdx"] == p)
            # the rest of the pair's rows is not written
            assert np.all(recs[off + counts[p]: off + pr[1]].view(np.int32) == -1), (maxp, p)
            off += pr[1]
        results.append(recs.tobytes())
    assert results[0] == results[1]
    # the mutual list is symmetric: pair 2 is pair 0 with the roles swapped
    m = sift.Matcher(300, 300, max_pairs=2)
    ab = run_list(sift, m, da.value, 257, db.value, 300, ratio=0.0)
    ba = run_list(sift, m, db.value, 300, da.value, 257, ratio=0.0)
    order = np.argsort(ab["trainIdx"], kind="stable")
    assert np.array_equal(ba["queryIdx"], ab["trainIdx"][order]) and np.array_equal(ba["trainIdx"], ab["queryIdx"][order])
    assert np.array_equal(ba["distance"], ab["distance"][order])


@pytest.fixture(scope="module")
def frames(sift):
    """Three 752 x 480 frames through one detector: each frame's rows, sidecar codes and keys copied out; the last two
    frames stay current as prev_descriptor / device_descriptor."""
    import torch

    w, h = 752, 480
    det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h, numFeatures=2000), lanes=1)
    det.gpuWarmUpAndAllocate()
    sets = []
    for f in (30, 31, 32):
        det.detectAndCompute(sift.synth_frame(f, w, h))
        n = det.total_size
        cp, kp = det.results_sidecar()
        codes = torch.empty((n, 128), dtype=torch.int8, device="cuda")
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        rows = torch.empty((n, 128), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        for dst, src, nb in ((codes, cp, n * 128), (keys, kp, n * 4), (rows, det.device_descriptor.data(), n * 256)):
            sift._check(sift.lib().sift_hip_memcpy_d2d(dst.data_ptr(), src, nb, None), "d2d")
        torch.cuda.synchronize()
        sets.append((codes, keys, rows, n))
    return det, sets


def test_detector_buffers_sidecar_route(sift, frames):
    from sift_amd import cv

    det, _ = frames
    n0, n1 = det.prev_size, det.total_size
    assert n0 > 300 and n1 > 300
    q, t = det.prev_descriptor.data(), det.device_descriptor.data()
    cap = max(n0, n1)
    mc = sift.Matcher(cap, cap)
    mc.set_sidecars(False)
    m, m2c = sift.Matcher(cap, cap), sift.Matcher(cap, cap, max_pairs=2)
    m2c.set_sidecars(False)
    for nq, nt in ((n0, n1), (min(n0, n1) - 3, 257)):
        tops = both_top2(sift, mc, q, nq, t, nt)
        for f in (dict(), dict(ratio_both_ways=True, max_distance=250.0), dict(cross_check=False)):
            ref = cv.filter_matches(*tops, **f)
            assert 0 < len(ref) < nq, (f, len(ref))
            side = run_list(sift, m, q, nq, t, nt, **f)  # two direct launches on the sidecars
            assert same(side, run_list(sift, mc, q, nq, t, nt, **f)), f  # two converting single-pair launches
            assert same(side, run_list(sift, m2c, q, nq, t, nt, **f)), f  # one converting two-pair launch
            assert same(side, ref), f
    # matchList on the detector's buffers is the default filter's list
    ml = sift.matchList(det.prev_descriptor, n0, det.device_descriptor, n1)
    assert same(ml, cv.filter_matches(*both_top2(sift, mc, q, n0, t, n1)))
    mr = sift.matchList(det.prev_descriptor, n0, det.device_descriptor, n1, ratio=0.8, ratio_on_squared=True,
                        cross_check=False)
    mb = sift.matchBruteForce(det.prev_descriptor, n0, det.device_descriptor, n1)
    assert np.array_equal(mr["queryIdx"], np.flatnonzero(mb >= 0)) and np.array_equal(mr["trainIdx"], mb[mb >= 0])


def test_codes_batched_from_sidecars(sift, frames):
    """sift_hip_match_list_codes_batched on the frames' sidecars gathered into one buffer (multi.pack_codes, as
    multi.all_gather_codes lays them out) against the filter on match_device's top-2 of the fp16 rows."""
    import torch

    from sift_amd import cv, multi

    _, sets = frames
    n_pad = multi.code_block_rows(max(s[3] for s in sets))
    buf = torch.cat([multi.pack_codes(c, k, n_pad) for c, k, _, _ in sets])
    idx = ((0, 1), (1, 2), (2, 0))
    pairs = []
    for a, b in idx:
        qa, qk = multi.code_set(a, n_pad)
        ta, tk = multi.code_set(b, n_pad)
        pairs.append((qa, qk, sets[a][3], ta, tk, sets[b][3]))
    pairs.append(pairs[0][:5] + (300,))  # a ragged train set
    idx += ((0, 1),)
    cap = max(s[3] for s in sets)
    mref = sift.Matcher(cap, cap)
    f = dict(ratio=0.85, max_distance=300.0)
    refs = [cv.filter_matches(*both_top2(sift, mref, sets[a][2].data_ptr(), p[2], sets[b][2].data_ptr(), p[5]),
                              img_idx=k, **f) for k, ((a, b), p) in enumerate(zip(idx, pairs))]
    tot = sum(p[2] for p in pairs)
    blobs = []
    for maxp in (4, 8):  # two 4-pair launches / one 8-pair launch
        out = torch.full((tot, 4), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m = sift.Matcher(cap, cap, max_pairs=maxp)
        m.match_list_codes_batched(buf.data_ptr(), buf.data_ptr(), pairs, out.data_ptr(), cnt.data_ptr(), **f)
        torch.cuda.synchronize()
        counts, recs = cnt.cpu().numpy(), out.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)
        off = 0
        for k, (ref, p) in enumerate(zip(refs, pairs)):
            assert 0 < len(ref) < p[2]
            assert counts[k] == len(ref) and same(recs[off: off + counts[k]], ref), (maxp, k)
            off += p[2]
        blobs.append(recs.tobytes())
    assert blobs[0] == blobs[1]


def test_repeatable_and_scratch_restored(sift):
    from sift_amd import cv

    nq, nt = 2000, 2000
    q, t, ofwd, orev = case(nq, nt)
    dq, dt = upload(sift, q), upload(sift, t)
    for pairs in (1, 2):
        m = sift.Matcher(nq, nt, max_pairs=pairs)
        a = run_list(sift, m, dq.value, nq, dt.value, nt)
        b = run_list(sift, m, dq.value, nq, dt.value, nt)
        assert same(a, b) and same(a, cv.filter_matches(*ofwd, *orev))
        # the matcher's merge scratch is back in its idle state: a plain match on it equals the oracle
        gi, gd = top2(sift, m, dq.value, nq, dt.value, nt)
        assert np.array_equal(gi, ofwd[0]) and np.array_equal(gd, ofwd[1])
        assert same(run_list(sift, m, dq.value, nq, dt.value, nt), a)


def test_argument_errors_launch_nothing(sift):
    import ctypes

    q, t, _, _ = case(33, 31)
    dq, dt = upload(sift, q), upload(sift, t)
    L = sift.lib()
    m = sift.Matcher(20, 40, max_pairs=2)  # max_query 20 < max_train 40
    out = sift.DeviceArray.from_numpy(np.full(4 * 64, -1, np.int32))
    cnt = sift.DeviceArray.from_numpy(np.full(4, -1, np.int32))
    cross, plain = sift._match_filter(), sift._match_filter(cross_check=False)
    INVALID = -1

    def untouched():
        sift._check(L.sift_hip_device_sync(), "sync")
        return np.all(out.to_numpy(np.int32, (4 * 64,)) == -1) and np.all(cnt.to_numpy(np.int32, (4,)) == -1)

    # nt > max_query: the reverse pair does not fit -- refused with cross_check, accepted without
    assert L.sift_hip_match_list_device(m._m, dq.value, 20, dt.value, 31, ctypes.byref(cross), out.value, cnt.value,
                                        None) == INVALID
    assert untouched()
    # a null out, count or filter
    assert L.sift_hip_match_list_device(m._m, dq.value, 20, dt.value, 20, ctypes.byref(cross), None, cnt.value,
                                        None) == INVALID
    assert L.sift_hip_match_list_device(m._m, dq.value, 20, dt.value, 20, ctypes.byref(cross), out.value, None,
                                        None) == INVALID
    assert L.sift_hip_match_list_device(m._m, dq.value, 20, dt.value, 20, None, out.value, cnt.value, None) == INVALID
    assert untouched()
    # P > max_pairs
    qa, ta = (ctypes.c_void_p * 3)(*[dq.value] * 3), (ctypes.c_void_p * 3)(*[dt.value] * 3)
    na = (ctypes.c_int * 3)(*[20] * 3)
    assert L.sift_hip_match_list_batched(m._m, 3, qa, na, ta, na, ctypes.byref(plain), out.value, cnt.value,
                                         None) == INVALID
    assert untouched()
    with pytest.raises(sift.SiftHipError):
        m.match_list_device(dq.value, 20, dt.value, 31, out.value, cnt.value)
    # the same sizes without the reverse direction are a valid call; an empty set gives count 0
    m.match_list_device(dq.value, 20, dt.value, 31, out.value, cnt.value, cross_check=False)
    assert 0 <= cnt.to_numpy(np.int32, (4,))[0] <= 20
    for nq, nt in ((0, 20), (20, 0)):
        m.match_list_device(dq.value, nq, dt.value, nt, out.value, cnt.value)
        assert cnt.to_numpy(np.int32, (4,))[0] == 0
    assert len(m.match_list_host(dq.value, 0, dt.value, 20)) == 0
