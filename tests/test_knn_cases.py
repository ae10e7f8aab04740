"""sift_amd.cv.knn / knn_records -- the references tests/test_gpu_match_knn.py holds the device to -- on their own
terms, without a GPU: the brute-force rule on small sets, the CPU oracle's knn-2 at k = 2, the planted ties of
tests/knn_cases.py really being ties, and the order and cap of the record list.
"""
import numpy as np
import pytest

import knn_cases as kc
from test_gpu_match_list import make_sets

FLT_MAX = kc.FLT_MAX


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("nq,nt,k", [s for s in kc.SHAPES if s[0] * s[1] <= 70 * 300])
def test_knn_is_the_brute_force_rule(sift, nq, nt, k):
    from sift_amd import cv

    q, t = kc.sets(nq, nt)
    got = cv.knn(q, t, k)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == got[1].shape == (nq, k)
    assert same(got, kc.brute_force(q, t, k))
    if nt < k:
        assert (got[0][:, nt:] == -1).all() and (got[1][:, nt:] == FLT_MAX).all()


def test_knn_hand_cases(sift):
    from sift_amd import cv

    d = lambda rows: np.pad(np.float32(rows), ((0, 0), (0, 126)))  # noqa: E731
    q, t = d([[5, 5], [20, 1]]), d([[5, 6], [5, 6], [20, 0], [5, 5], [20, 0], [5, 5]])
    idx, d2 = cv.knn(q, t, 4)
    assert idx.tolist() == [[3, 5, 0, 1], [2, 4, 3, 5]]  # ties to the lower index at every rank
    assert d2.tolist() == [[0, 0, 1, 1], [1, 1, 241, 241]]
    for k in range(1, 9):  # the column-prefix property
        a = cv.knn(q, t, k)
        assert same(a, (np.ascontiguousarray(cv.knn(q, t, 8)[0][:, :k]), np.ascontiguousarray(cv.knn(q, t, 8)[1][:, :k])))
    e = cv.knn(q, t[:0], 3)
    assert (e[0] == -1).all() and (e[1] == FLT_MAX).all() and e[0].shape == (2, 3)
    assert cv.knn(q[:0], t, 3)[0].shape == (0, 3)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            cv.knn(q, t, bad)
    # the general path's rule: a non-finite train row is nobody's neighbour, a non-finite query has none
    qf, tf = q.copy() + 0.5, t.copy()
    tf[3, 7] = np.inf
    qf[1, 0] = np.nan
    idx, d2 = cv.knn(qf, tf, 6)
    assert idx[0].tolist() == [0, 1, 5, 2, 4, -1] and d2[0, -1] == FLT_MAX
    assert (idx[1] == -1).all() and (d2[1] == FLT_MAX).all()


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 40), (40, 1), (33, 31), (257, 300)])
def test_k2_is_the_oracle(sift, oracle, nq, nt):
    from sift_amd import cv

    q, t = make_sets(nq, nt)
    idx, dist = oracle.knn2(q, t)
    d2 = np.rint(np.where(idx >= 0, dist, 0).astype(np.float64) ** 2).astype(np.float32)
    d2[idx < 0] = FLT_MAX
    got = cv.knn(q, t, 2)
    assert np.array_equal(got[0], idx) and np.array_equal(got[1], d2)


def test_planted_ties_are_ties(sift):
    from sift_amd import cv

    q, t = kc.tie_sets()
    assert len(kc.TIE_ROWS) == 12 and len(set(kc.TIE_ROWS)) == 12
    d0 = ((t - q[0]) ** 2).sum(1)
    assert np.flatnonzero(d0 == 0).tolist() == sorted(kc.TIE_ROWS)  # more than k rows at distance 0
    rows = sorted(kc.TIE_ROWS)
    assert rows[0] // 32 == rows[1] // 32 and (rows[0] % 8) // 4 != (rows[1] % 8) // 4  # one tile, the two lane halves
    assert 40 // 32 == 1 and 255 // 256 == 0 and 256 // 256 == 1 and 600 // 256 == 2
    assert rows[-1] == len(t) - 1 and len(t) % 32 != 0  # the last tile is partial
    assert len({r // 32 for r in rows}) >= 10  # the others lie in other tiles
    idx, d2 = cv.knn(q, t, 8)
    assert idx[0].tolist() == rows[:8] and not d2[0].any()
    # the split case keeps a tie on each side of the first key group's end
    qs, ts = kc.split_sets(257)
    assert np.array_equal(ts[255], qs[0]) and np.array_equal(ts[256], qs[0])
    # low entropy: most rows hold equal distances at adjacent ranks, and the order there is the index order
    ql, tl = kc.low_entropy()
    assert ql.shape == (257, 128) and tl.shape == (600, 128) and ql.max() == 3 and tl.max() == 3
    idx, d2 = cv.knn(ql, tl, 8)
    tie = d2[:, 1:] == d2[:, :-1]
    assert tie.any(1).mean() > 0.5
    assert (idx[:, 1:][tie] > idx[:, :-1][tie]).all()
    assert same((idx[:16], d2[:16]), kc.brute_force(ql[:16], tl, 8))


def test_knn_records_order_and_cap(sift):
    from sift_amd import cv

    idx = np.int32([[4, 2, -1], [7, -1, -1], [-1, -1, -1], [1, 0, 3]])
    d2 = np.float32([[0, 9, FLT_MAX], [16, FLT_MAX, FLT_MAX], [FLT_MAX] * 3, [4, 4, 25]])
    whole = cv.knn_records(idx, d2)
    assert whole.dtype == sift.DMATCH_DTYPE
    assert [tuple(r) for r in whole.tolist()] == [(0, 4, 0, 0.0), (0, 2, 0, 3.0), (1, 7, 0, 4.0), (3, 1, 0, 2.0),
                                                  (3, 0, 0, 2.0), (3, 3, 0, 5.0)]
    cap = cv.knn_records(idx, d2, max_distance=3.0, img_idx=2)  # inclusive, float32
    assert [tuple(r) for r in cap.tolist()] == [(0, 4, 2, 0.0), (0, 2, 2, 3.0), (3, 1, 2, 2.0), (3, 0, 2, 2.0)]
    assert len(cv.knn_records(idx, d2, max_distance=-1.0)) == 6
    assert len(cv.knn_records(idx[:0], d2[:0])) == 0
    with pytest.raises(ValueError):
        cv.knn_records(idx, d2, max_distance=float("nan"))
    with pytest.raises(ValueError):
        cv.knn_records(idx, d2[:2])
    # on a case of the GPU test: neither empty nor full at the median distance
    ref = kc.reference(*kc.BIG, 4)
    n = len(cv.knn_records(*ref, max_distance=float(np.median(np.sqrt(ref[1])))))
    assert 0 < n < kc.BIG[0] * 4
